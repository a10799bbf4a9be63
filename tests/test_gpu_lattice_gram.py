"""GPU: lattice observations -- fluid_observation_gram_lattice (include/fluid_amd.h, "lattice observations").

Every expected value comes from the header's definition written in numpy on what download_members showed before the call:
`define_obs` and `operands` as tests/test_gpu_observe.py has them, and `weights`, rule 2 in float64 operation by operation
(Horner's rule).  On dyadic data with every point either on a node (w = 1) or outside every support the results are compared
with `==` against integer arithmetic; on general data, per node, against math.fsum of the products within
    gamma(P_b + 3) * sum |products|  +  sum dw |a_k a_m|,      gamma(n) = n u / (1 - n u), u = 2^-53,
P_b the points with r < 2: a recursive double sum of P_b terms in any order, the reference's own rounded products and final
rounding, the once-rounded w a_k -- and dw = 2^-24 w + 1e-13, the tolerance tests/test_gpu_local.py derives for the taper
(one rounding to float on top of the double evaluation of a polynomial whose terms stay below 32).  Derived, not measured."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = np.float32
COARSE = np.array([-1, -0.5, -0.25, 0.0, -0.0, 0.25, 0.5, 1], F32)
MAIN = ("u", "v", "dens", "u_prev", "v_prev", "dens_prev")
COUNTS = ("sweeps", "solves", "jacobi_launches", "jacobi_field_launches", "pressure_sweeps")
MEMBERS = [1, 2, 3, 9, 17, 32, 33, 64]
DT = 0.016
U = 2.0 ** -53


def F():
    import fluidsimulationcuda_amd as f
    return f


def solver(n, members, storage=0, **kw):
    return F().FluidSolver(n, members=members, storage=storage, **kw)


# ---- the definition ------------------------------------------------------------------------------------------------------
def stencil(x, cols, rows):
    """the four taps (M, P) each and the four weights (P,) of the header's definition, all float32"""
    c, r = np.asarray(cols, F32), np.asarray(rows, F32)
    j0, i0 = c.astype(np.int64), r.astype(np.int64)
    s1 = c - j0.astype(F32)
    s0 = F32(1) - s1
    t1 = r - i0.astype(F32)
    t0 = F32(1) - t1
    x = np.asarray(x, F32)
    return (x[:, i0, j0], x[:, i0 + 1, j0], x[:, i0, j0 + 1], x[:, i0 + 1, j0 + 1]), (s0, s1, t0, t1)


def define_obs(x, cols, rows):
    """x: (M, W, W) float32, what the pack shows.  h[m][p], float32, operation by operation."""
    (q00, q01, q10, q11), (s0, s1, t0, t1) = stencil(x, cols, rows)       # q[col][row]
    with np.errstate(all="ignore"):
        a = t0 * q00 + t1 * q01
        e = t0 * q10 + t1 * q11
        h = s0 * a + s1 * e
    assert h.dtype == F32
    return h


def operands(h, obs, inv_sigma, centre):
    """a_k (M, P) and d (P,) (None without obs) of the header, float64"""
    hd = np.asarray(h, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        mean = None
        if centre:
            s = hd[0].copy()
            for m in range(1, hd.shape[0]):               # member order
                s = s + hd[m]
            mean = s / np.float64(hd.shape[0])
        a = hd - mean if centre else hd
        d = None
        if obs is not None:
            d = np.asarray(obs, F32).astype(np.float64)
            if centre:
                d = d - mean
        if inv_sigma is not None:
            sg = np.asarray(inv_sigma, F32).astype(np.float64)
            a = a * sg
            if d is not None:
                d = d * sg
    return a, d


def node_positions(shape, origin, step):
    return origin[0] + step * np.arange(shape[0]), origin[1] + step * np.arange(shape[1])


def weights(cols, rows, shape, origin, step, c):
    """rule 2, in float64 operation by operation: (w, r, g), each (nodes_row, nodes_col, P); w = (double)(float)g"""
    nrow, ncol = node_positions(shape, origin, step)
    x, y = np.asarray(cols, F32).astype(np.float64), np.asarray(rows, F32).astype(np.float64)
    dx = x[None, None, :] - ncol.astype(np.float64)[None, :, None]
    dy = y[None, None, :] - nrow.astype(np.float64)[:, None, None]
    r = np.sqrt(dx * dx + dy * dy) / np.float64(F32(c))
    with np.errstate(all="ignore"):
        g = -0.25 * r + 0.5
        g = g * r + 0.625
        g = g * r - 5.0 / 3.0
        g = g * r
        near = g * r + 1.0
        g = (1.0 / 12.0) * r - 0.5
        g = g * r + 0.625
        g = g * r + 5.0 / 3.0
        g = g * r - 5.0
        g = g * r + 4.0
        far = g - (2.0 / 3.0) / r
    g = np.clip(np.where(r <= 1.0, near, np.where(r < 2.0, far, 0.0)), 0.0, 1.0)
    return g.astype(F32).astype(np.float64), r, g


def gamma(n):
    return n * U / (1 - n * U)


def stack(a, d):
    return a if d is None else np.vstack([a, d[None]])


def exact_node(a, d, idx, bits=14):
    """the (M [+ 1]) x (M [+ 1]) matrix of exact sums over the points idx, all of weight 1, for operands that are multiples of
    2^-bits: integer arithmetic"""
    rows = stack(a, d)[:, idx]
    i = np.ldexp(rows, bits)
    assert (i == np.rint(i)).all() and (i.size == 0 or np.abs(i).max() < 2 ** 22)
    i = i.astype(np.int64)
    full = i @ i.T
    assert np.abs(full).max(initial=0) < 2 ** 53
    return np.ldexp(full.astype(np.float64), -2 * bits)


def node_reference(a, d, w, inside):
    """(math.fsum of the products, of their magnitudes, the taper term of the bound) as (M [+ 1]) x (M [+ 1]) matrices"""
    rows = stack(a, d)
    idx = np.nonzero(w)[0]
    left, right = rows[:, idx] * w[idx], rows[:, idx]
    k = rows.shape[0]
    want, mag = np.zeros((k, k)), np.zeros((k, k))
    for i in range(k):
        for j in range(i, k):
            p = left[i] * right[j]                       # (w a_k) a_m, (w a_k) d, (w d) d
            want[i, j] = want[j, i] = math.fsum(p)
            mag[i, j] = mag[j, i] = math.fsum(np.abs(p))
    near = np.abs(rows[:, inside])
    return want, mag, (near * (2.0 ** -24 * w[inside] + 1e-13)) @ near.T


def pack_node(m, gram, rhs, dd):
    if rhs is None:
        return gram
    out = np.empty((m + 1, m + 1), np.float64)
    out[:m, :m], out[:m, m], out[m, :m], out[m, m] = gram, rhs, rhs, dd
    return out


def call(s, field, lat, c, obs=None, inv_sigma=None, centre=True):
    """(gram, rhs, dd, counts), rhs and dd None without obs"""
    got = s.observation_gram_lattice(field, lat[0], lat[1], lat[2], c, obs=obs, inv_sigma=inv_sigma, centre=centre)
    if obs is None:
        assert len(got) == 2
        return got[0], None, None, got[1]
    assert len(got) == 4
    return got


def check_shapes(got, lat, m):
    gram, rhs, dd, counts = got
    nr, nc = lat[0]
    assert gram.shape == (nr, nc, m, m) and gram.dtype == np.float64 and counts.shape == (nr, nc) and counts.dtype == np.int32
    if rhs is not None:
        assert rhs.shape == (nr, nc, m) and dd.shape == (nr, nc) and rhs.dtype == dd.dtype == np.float64


def flat(got):
    return np.concatenate([v.ravel() for v in got[:3] if v is not None])


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    view = np.uint32 if got.dtype == F32 else np.uint64
    ok = np.where(np.isnan(want), np.isnan(got), got.view(view) == want.view(view))
    if not ok.all():
        at = tuple(np.argwhere(~ok)[0])
        raise AssertionError("%s: %d of %d values differ; first at %s: got %r want %r" % (what, int((~ok).sum()), ok.size, at, got[at], want[at]))


def equal(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(want).all(), what
    ok = got == want
    if not ok.all():
        at = tuple(np.argwhere(~ok)[0])
        raise AssertionError("%s: %d of %d entries differ; first at %s: got %r want %r" % (what, int((~ok).sum()), ok.size, at, got[at], want[at]))


def symmetric(g, what):
    g = np.ascontiguousarray(g)
    assert np.array_equal(g.view(np.uint64), np.ascontiguousarray(g.T).view(np.uint64)), "%s: not bit-symmetric" % what


def plus_zero(got, a, b, what):
    for v in got[:3]:
        if v is not None:
            assert not np.ascontiguousarray(v[a, b]).view(np.uint64).any(), "%s: node (%d, %d) sees no point and is not +0.0" % (what, a, b)


def network(n, count, rng, quarter=False):
    """`count` points: the corners, points on the four walls, every cell centre, positions with s1 or t1 equal to 0, random
    positions -- all of the special ones when they fit, a random choice of them otherwise.  quarter: multiples of 1/4 only."""
    lo, hi = 0.5, n + 0.5
    k = np.arange(1, n + 1, dtype=np.float64)
    pts = [(lo, lo), (hi, lo), (lo, hi), (hi, hi)]
    pts += [(lo, v) for v in k] + [(hi, v) for v in k] + [(v, lo) for v in k] + [(v, hi) for v in k]
    pts += [(c, r) for r in k for c in k]
    free = (lambda size: np.round(rng.uniform(lo, hi, size) * 4) / 4) if quarter else (lambda size: rng.uniform(lo, hi, size))
    zero = max(4, 2 * n)
    pts += list(zip(rng.choice(k, zero), free(zero))) + list(zip(free(zero), rng.choice(k, zero)))
    pts = np.array(pts, np.float64)
    if count <= len(pts):
        pts = pts[rng.permutation(len(pts))[:count]]
    else:
        extra = count - len(pts)
        pts = np.vstack([pts, np.stack([free(extra), free(extra)], axis=1)])
    cols, rows = pts[:, 0].astype(F32), pts[:, 1].astype(F32)
    assert cols.min() >= lo and cols.max() <= hi and rows.min() >= lo and rows.max() <= hi
    return cols, rows


def dyadic_network(n, count, lat, rng):
    """`count` points at multiples of 1/4: about half on the nodes that lie on cell centres of the array, the others at
    least 2.5 from every node -- with c = 1 a point has r = 0 (g = 1 exactly) or takes part nowhere"""
    nrow, ncol = node_positions(*lat)
    on = np.array([(c, r) for r in nrow for c in ncol if 1 <= r <= n and 1 <= c <= n], np.float64).reshape(-1, 2)
    q = np.arange(2, 4 * n + 3) / 4.0                                     # 0.5 .. n + 0.5
    grid = np.array([(c, r) for r in q for c in q])
    far = np.ones(len(grid), bool)
    for r in nrow:
        for c in ncol:
            far &= (grid[:, 0] - c) ** 2 + (grid[:, 1] - r) ** 2 >= 2.5 ** 2
    away = grid[far]
    assert len(away)
    k = min(count, (count + 1) // 2) if len(on) else 0
    pts = np.vstack([on[rng.integers(0, len(on), k)] if k else np.empty((0, 2)), away[rng.integers(0, len(away), count - k)]])
    pts = pts[rng.permutation(count)]
    return pts[:, 0].astype(F32), pts[:, 1].astype(F32)


# ---- 1. exact on dyadic data ---------------------------------------------------------------------------------------------------
# (N, P, (shape, origin, step)): every size, point count and lattice shape; origins that put nodes off the array
DYADIC = [(6, 1, ((1, 1), (3, 3), 8)), (6, 64, ((1, 3), (3, -5), 8)), (13, 65, ((3, 2), (-3, 2), 8)), (13, 513, ((5, 5), (-10, -9), 8)),
          (30, 5000, ((5, 5), (-1, -1), 8)), (30, 513, ((3, 2), (7, 9), 8)), (30, 65, ((1, 3), (40, 40), 8))]


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", MEMBERS)
def test_exact_on_dyadic_data(members, storage):
    rng = np.random.default_rng(1000 + 100 * storage + members)
    for n, p, lat in DYADIC:
        x = rng.choice(COARSE, size=(members, n + 2, n + 2)).astype(F32)
        cols, rows = dyadic_network(n, p, lat, rng)
        y = (rng.integers(-8, 9, p) / 4.0).astype(F32)
        sg = rng.choice(np.array([0.5, 1.0, 2.0], F32), p)
        w, r, _ = weights(cols, rows, *lat, 1.0)
        assert (((r == 0) & (w == 1)) | ((r >= 2.5) & (w == 0))).all()
        with solver(n, members, storage) as a, solver(n, members, storage) as b:
            for s in (a, b):
                s.upload_members(dens=x)
                s.set_observation_points(cols, rows)
            h = define_obs(x, cols, rows)                  # multiples of 2^-6, exact in float32
            assert np.array_equal(a.observe("dens"), h)
            for centre in (False, True):
                if centre and members & (members - 1):    # a power of two: the mean, the anomalies and the products are exact
                    continue
                for obs, sigma in ((None, None), (y, None), (None, sg), (y, sg)):
                    what = "M=%d storage=%d N=%d P=%d lattice %s centre=%s obs=%s sigma=%s" % (members, storage, n, p, lat, centre, obs is not None,
                                                                                              sigma is not None)
                    got = call(a, "dens", lat, 1.0, obs, sigma, centre)
                    check_shapes(got, lat, members)
                    gram, rhs, dd, counts = got
                    am, d = operands(h, obs, sigma, centre)
                    for ia in range(lat[0][0]):
                        for ib in range(lat[0][1]):
                            idx = np.nonzero(w[ia, ib])[0]
                            assert counts[ia, ib] == len(idx), what
                            want = exact_node(am, d, idx)
                            equal(pack_node(members, gram[ia, ib], None if obs is None else rhs[ia, ib], None if obs is None else dd[ia, ib]),
                                  want, "%s node (%d, %d)" % (what, ia, ib))
                            symmetric(gram[ia, ib], what)
                            if len(idx) == 0:
                                plus_zero(got, ia, ib, what)
                    same_bits(flat(call(a, "dens", lat, 1.0, obs, sigma, centre)), flat(got), what + ": two calls in a row")
                    again = call(b, "dens", lat, 1.0, obs, sigma, centre)
                    same_bits(flat(again), flat(got), what + ": a second context")
                    assert np.array_equal(again[3], counts)
                    if sigma is None:                      # a null inv_sigma gives the bits that all ones give
                        same_bits(flat(call(a, "dens", lat, 1.0, obs, np.ones(p, F32), centre)), flat(got), what + ": all ones")
            assert np.array_equal(a.download_members("dens").view(np.uint32), x.view(np.uint32)), "the call changed the field"


# ---- 2. one node, every point on it: fluid_observation_gram ----------------------------------------------------------------------
@pytest.mark.parametrize("members", [1, 3, 8, 64])
def test_one_node_with_every_point_on_it_is_the_observation_gram(members):
    n = 13
    rng = np.random.default_rng(2000 + members)
    lat = ((1, 1), (5, 7), 8)
    with solver(n, members) as s:
        for p in (1, 65, 513):
            x = rng.choice(COARSE, size=(members, n + 2, n + 2)).astype(F32)
            y = (rng.integers(-8, 9, p) / 4.0).astype(F32)
            sg = rng.choice(np.array([0.5, 1.0, 2.0], F32), p)
            s.upload_members(dens=x)
            s.set_observation_points(np.full(p, 7.0, F32), np.full(p, 5.0, F32))
            for centre in (False, True):
                if centre and members & (members - 1):
                    continue
                for obs, sigma in ((None, None), (y, None), (None, sg), (y, sg)):
                    what = "M=%d P=%d centre=%s obs=%s sigma=%s" % (members, p, centre, obs is not None, sigma is not None)
                    gram, rhs, dd, counts = call(s, "dens", lat, 1.0, obs, sigma, centre)
                    want = s.observation_gram("dens", obs=obs, inv_sigma=sigma, centre=centre)
                    assert counts[0, 0] == p
                    if obs is None:
                        same_bits(gram[0, 0], want, what)
                    else:
                        same_bits(gram[0, 0], want[0], what)
                        same_bits(rhs[0, 0], want[1], what + ": rhs")
                        same_bits(dd[0, 0], np.float64(want[2]), what + ": dd")


# ---- 3. general data within the summation bound ----------------------------------------------------------------------------------
def check_general(got, h, obs, sg, centre, lat, c, cols, rows, what):
    gram, rhs, dd, counts = got
    m = h.shape[0]
    check_shapes(got, lat, m)
    a, d = operands(h, obs, sg, centre)
    w, r, g = weights(cols, rows, *lat, c)
    worst = 0.0
    for ia in range(lat[0][0]):
        for ib in range(lat[0][1]):
            inside = r[ia, ib] < 2.0
            lo, hi = int((g[ia, ib] > 1e-13).sum()), int(inside.sum())
            assert lo <= counts[ia, ib] <= hi, "%s node (%d, %d): count %d outside [%d, %d]" % (what, ia, ib, counts[ia, ib], lo, hi)
            want, mag, taper = node_reference(a, d, w[ia, ib], inside)
            bound = gamma(hi + 3) * mag + taper
            err = np.abs(pack_node(m, gram[ia, ib], None if obs is None else rhs[ia, ib], None if obs is None else dd[ia, ib]) - want)
            assert (err <= bound).all(), "%s node (%d, %d): %d entries outside the bound (largest ratio %.3g)" % (
                what, ia, ib, int((err > bound).sum()), float((err / np.maximum(bound, 1e-300)).max()))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            symmetric(gram[ia, ib], what)
            if counts[ia, ib] == 0:
                plus_zero(got, ia, ib, what)
    print("%s: largest error / bound = %.4f, counts %d .. %d" % (what, worst, counts.min(), counts.max()))
    return counts


GENERAL = [(30, 9, 5000, ((3, 2), (-3, 2), 8)), (13, 33, 513, ((3, 2), (-3, 2), 8)), (30, 64, 257, ((1, 3), (15, -1), 16)),
           (6, 3, 65, ((1, 1), (3, 3), 8)), (13, 1, 64, ((3, 2), (2, 2), 8)), (30, 2, 1, ((1, 3), (14, 9), 8)), (13, 3, 257, ((5, 5), (-9, -40), 16)),
           (13, 32, 513, ((3, 2), (-3, 2), 8))]


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n,members,p,lat", GENERAL)
def test_general_data_within_the_bound(n, members, p, lat, storage):
    rng = np.random.default_rng(3000 * storage + 10 * n + members)
    w = n + 2
    cols, rows = network(n, p, rng)
    step = lat[2]
    seen = set()
    with solver(n, members, storage) as s:
        s.set_observation_points(cols, rows)
        for c in (0.3, 1.0, float(step), 4.0 * step):     # nodes with no points, some points, all points
            for centre in (False, True):
                x = rng.uniform(0.25, 1.0, (members, w, w)) * rng.choice([-1.0, 1.0], (members, w, w))
                if centre:
                    x = x + 50
                s.upload_members(v=x.astype(F32))
                before = s.download_members("v")
                h = define_obs(before, cols, rows)
                assert np.isfinite(h).all()
                y = (rng.normal(size=p) + (50 if centre else 0)).astype(F32)
                sg = rng.uniform(0.5, 20.0, p).astype(F32)
                what = "n=%d M=%d P=%d lattice %s storage=%d c=%g centre=%s" % (n, members, p, lat, storage, c, centre)
                counts = check_general(call(s, "v", lat, c, y, sg, centre), h, y, sg, centre, lat, c, cols, rows, what)
                if not centre:
                    check_general(call(s, "v", lat, c, None, None, centre), h, None, None, centre, lat, c, cols, rows, what + ": gram alone")
                seen.update(("none",) if (counts == 0).any() else ())
                seen.update(("all",) if (counts == p).any() else ())
                seen.update(("some",) if ((counts > 0) & (counts < p)).any() else ())
                assert np.array_equal(s.download_members("v").view(np.uint32), before.view(np.uint32)), "the call changed the field"
    if p >= 64 and lat[0] != (1, 1):
        assert seen == {"none", "some", "all"}, (seen, "the values of c do not cover empty, partial and full nodes")


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_general_data_after_a_velocity_step(storage):
    """u_prev after vel_step: with fp16 storage the pressure, held scaled"""
    n, members, p, lat = 30, 9, 513, ((3, 2), (-3, 2), 8)
    rng = np.random.default_rng(3500 + storage)
    w = n + 2
    cols, rows = network(n, p, rng)
    y, sg = rng.normal(size=p).astype(F32) * F32(0.01), rng.uniform(0.5, 20.0, p).astype(F32)
    with solver(n, members, storage) as s:
        s.upload_members(dens=rng.uniform(-4.0, 4.0, (members, w, w)).astype(F32), u=rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32),
                         v=rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32))
        s.vel_step()
        s.set_observation_points(cols, rows)
        for field in ("u_prev", "dens"):
            before = s.download_members(field)
            h = define_obs(before, cols, rows)
            assert np.isfinite(h).all() and np.abs(h).max() > 0
            for centre in (False, True):
                what = "storage=%d %s centre=%s" % (storage, field, centre)
                check_general(call(s, field, lat, 8.0, y, sg, centre), h, y, sg, centre, lat, 8.0, cols, rows, what)
            assert np.array_equal(s.download_members(field).view(np.uint32), before.view(np.uint32)), "the call changed the field"


# ---- 4. every point is seen, and only where it belongs ---------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_every_point_is_seen_and_only_where_it_belongs(storage):
    n, members, p, lat, c, planted = 30, 3, 513, ((3, 2), (-3, 2), 8), 8.0, 1
    rng = np.random.default_rng(4000 + storage)
    w = n + 2
    cols, rows = network(n, p, rng)
    x = rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32)
    wt, _, _ = weights(cols, rows, *lat, c)
    j0, i0 = cols.astype(np.int64), rows.astype(np.int64)
    with solver(n, members, storage) as s:
        s.set_observation_points(cols, rows)
        s.upload_members(dens=x)
        clean = call(s, "dens", lat, c, centre=False)
        changed_somewhere = kept_somewhere = False
        (_, _, _, _), (s0, s1, t0, t1) = stencil(x, cols, rows)
        for at in (0, 63, 64, p - 1):                     # across the chunks of 64 points
            di, dj = int(t1[at] > t0[at]), int(s1[at] > s0[at])         # the tap of the largest weight (at least 1/4) of point `at`
            ci, cj = i0[at] + di, j0[at] + dj
            xp = x.copy()
            xp[planted, ci, cj] = 1000.0
            s.upload_members(dens=xp)
            got = call(s, "dens", lat, c, centre=False)
            check_general(got, define_obs(s.download_members("dens"), cols, rows), None, None, False, lat, c, cols, rows, "storage=%d point %d" % (storage, at))
            touched = ((i0 == ci) | (i0 == ci - 1)) & ((j0 == cj) | (j0 == cj - 1))     # the points whose stencil holds the cell
            assert touched[at]
            for ia in range(lat[0][0]):
                for ib in range(lat[0][1]):
                    what = "storage=%d point %d node (%d, %d)" % (storage, at, ia, ib)
                    if wt[ia, ib, at] > 1e-6:
                        assert got[0][ia, ib, planted, planted] > clean[0][ia, ib, planted, planted] + 1e4 * wt[ia, ib, at], what + ": not seen"
                        changed_somewhere = True
                    elif not (wt[ia, ib][touched] != 0).any():
                        same_bits(got[0][ia, ib], clean[0][ia, ib], what + ": a node that does not see the point changed")
                        kept_somewhere = True
            assert np.array_equal(got[3], clean[3])
        assert changed_somewhere and kept_somewhere


# ---- 5. poisoning -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_poisoning(storage):
    """a NaN tap and a NaN y_p at a point inside the supports of nodes 0 and 1 and outside node 2's"""
    n, members, p, bad, at = 30, 5, 513, 2, 100
    lat, c = ((1, 3), (15, -1), 16), 8.0                  # nodes on row 15, columns -1, 15, 31; supports of radius 16
    rng = np.random.default_rng(5000 + storage)
    w = n + 2
    x = rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32)
    cols, rows = network(n, p, rng)
    cols[at], rows[at] = 8.25, 15.5
    y = rng.normal(size=p).astype(F32)
    sg = rng.uniform(0.5, 2.0, p).astype(F32)
    wt, r, _ = weights(cols, rows, *lat, c)
    assert wt[0, 0, at] != 0 and wt[0, 1, at] != 0 and r[0, 2, at] > 2.5
    j0, i0 = cols.astype(np.int64), rows.astype(np.int64)
    touched = ((i0 == 15) | (i0 == 14)) & ((j0 == 8) | (j0 == 7))          # the points whose stencil holds cell (15, 8)
    assert touched[at] and (r[0, 2][touched] > 2.5).all()
    keep = np.ones((members, members), bool)
    keep[bad] = keep[:, bad] = False
    with solver(n, members, storage) as s:
        s.upload_members(u=x)
        s.set_observation_points(cols, rows)
        clean = {centre: call(s, "u", lat, c, y, sg, centre) for centre in (False, True)}
        assert all(np.isfinite(v).all() for centre in clean for v in clean[centre][:3])
        ybad = y.copy()
        ybad[at] = np.nan
        for centre in (False, True):                       # a non-finite observed value: rhs and dd of the nodes that see it
            gram, rhs, dd, counts = call(s, "u", lat, c, ybad, sg, centre)
            same_bits(gram, clean[centre][0], "a NaN in y, centre=%s: the matrices" % centre)
            assert np.isnan(rhs[0, :2]).all() and np.isnan(dd[0, :2]).all()
            same_bits(rhs[0, 2], clean[centre][1][0, 2], "a NaN in y: rhs of the node that does not see it")
            same_bits(dd[0, 2], clean[centre][2][0, 2], "a NaN in y: dd of the node that does not see it")
            assert np.array_equal(counts, clean[centre][3])
        x[bad, 15, 8] = np.nan                             # a non-finite observation of member 2
        s.upload_members(u=x)
        assert np.isnan(s.observe("u")[bad, at])
        gram, rhs, dd, counts = call(s, "u", lat, c, y, sg, False)
        for node in (0, 1):
            g = gram[0, node]
            assert np.isnan(g[bad]).all() and np.isnan(g[:, bad]).all() and np.isnan(rhs[0, node, bad])
            assert np.array_equal(g.view(np.uint64)[keep], clean[False][0][0, node].view(np.uint64)[keep]), "a NaN in member 2 changed another entry"
            assert np.array_equal(np.delete(rhs[0, node], bad).view(np.uint64), np.delete(clean[False][1][0, node], bad).view(np.uint64))
            same_bits(dd[0, node], clean[False][2][0, node], "dd")
        for v, ref in zip((gram, rhs, dd), clean[False][:3]):
            same_bits(v[0, 2], ref[0, 2], "centre=False: the node that does not see the point")
        gram, rhs, dd, counts = call(s, "u", lat, c, y, sg, True)
        assert np.isnan(gram[0, :2]).all() and np.isnan(rhs[0, :2]).all() and np.isnan(dd[0, :2]).all()
        for v, ref in zip((gram, rhs, dd), clean[True][:3]):
            same_bits(v[0, 2], ref[0, 2], "centre=True: the node that does not see the point")
        assert np.array_equal(counts, clean[True][3])


# ---- 6. empty nodes ----------------------------------------------------------------------------------------------------------------
def test_a_lattice_off_the_array_is_all_zeros():
    n, members, p = 13, 9, 257
    rng = np.random.default_rng(6)
    x = rng.uniform(-1.0, 1.0, (members, n + 2, n + 2)).astype(F32)
    cols, rows = network(n, p, rng)
    y = rng.normal(size=p).astype(F32)
    with solver(n, members) as s:
        s.upload_members(dens=x)
        s.set_observation_points(cols, rows)
        for lat in (((5, 5), (100, 100), 8), ((3, 2), (-4000, 3), 16)):
            for obs in (None, y):
                got = call(s, "dens", lat, 0.3, obs, None, True)
                check_shapes(got, lat, members)
                assert not got[3].any()
                for v in got[:3]:
                    if v is not None:
                        assert not np.ascontiguousarray(v).view(np.uint64).any(), "an empty node is not +0.0"
        assert np.array_equal(s.download_members("dens").view(np.uint32), x.view(np.uint32)), "the call changed the field"


# ---- 7. lazy state and side effects --------------------------------------------------------------------------------------------------
def prepared(n, members, storage, fields, case):
    """a context in one of the lazy states, and the field the state is about (as in tests/test_gpu_observe.py)"""
    s = solver(n, members, storage)
    s.timing_enable(True)
    s.upload_members(**fields)
    s.step(use_sources=True)
    if case == "scaled":                   # fp16 storage: the pressure of a step (u_prev) is held scaled
        return s, "u_prev"
    s.computeDivergenceAndPressure("u", "v", "dens_prev", "tmp0")       # dens_prev: zero by definition, marked, not written
    if case == "zeros":
        return s, "dens_prev"
    s.add_source("dens", "dens_prev", DT)  # ... and adding such a source is deferred: dens owes itself an increment
    return s, "dens"


@pytest.mark.parametrize("storage,case", [(0, "pending"), (0, "zeros"), (1, "scaled"), (1, "pending"), (1, "zeros")])
def test_lazy_state_is_settled_and_nothing_is_altered(storage, case):
    from fluidsimulationcuda_amd import capi
    members, n, p, lat, c = 3, 30, 257, ((3, 2), (-3, 2), 8), 8.0
    rng = np.random.default_rng(7000 * storage + len(case))
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    cols, rows = network(n, p, rng)
    y = np.zeros(p, F32)
    a, f = prepared(n, members, storage, fields, case)
    b, _ = prepared(n, members, storage, fields, case)
    with a, b:
        a.set_observation_points(cols, rows)
        got = call(a, f, lat, c, y, None, False)
        shown = a.download_members(f)
        if case == "zeros":
            assert not shown.view(np.uint32).any() and not got[0].view(np.uint64).any()
        else:
            assert np.abs(shown[:, 1:-1, 1:-1]).max() > 0
        check_general(got, define_obs(shown, cols, rows), y, None, False, lat, c, cols, rows, "storage=%d %s" % (storage, case))
        for name in capi.FIELD_NAMES:          # every field of every member, against the twin that never called
            assert np.array_equal(a.download_members(name).view(np.uint32), b.download_members(name).view(np.uint32)), name
        ta, tb = a.timing_read(reset=False), b.timing_read(reset=False)
        assert {k: ta[k] for k in COUNTS} == {k: tb[k] for k in COUNTS}
        for s in (a, b):
            s.step(use_sources=True)
        for name in ("u", "v", "dens"):
            assert np.array_equal(a.download_members(name).view(np.uint32), b.download_members(name).view(np.uint32)), name + " a step later"
        ta, tb = a.timing_read(reset=False), b.timing_read(reset=False)
        assert {k: ta[k] for k in ta if not k.endswith("_ms")} == {k: tb[k] for k in tb if not k.endswith("_ms")}


# ---- 8. the cache of point lists --------------------------------------------------------------------------------------------------------
def test_the_lists_follow_the_network_and_c():
    n, members, p, lat = 13, 3, 513, ((3, 2), (-3, 2), 8)
    rng = np.random.default_rng(8)
    x = rng.uniform(-1.0, 1.0, (members, n + 2, n + 2)).astype(F32)
    y, sg = rng.normal(size=p).astype(F32), rng.uniform(0.5, 2.0, p).astype(F32)
    first, moved, fewer = network(n, p, rng), network(n, p, rng), network(n, 65, rng)
    with solver(n, members) as s:
        s.upload_members(dens=x)
        s.set_observation_points(*first)
        h = define_obs(x, *first)
        one = call(s, "dens", lat, 4.0, y, sg, True)
        check_general(one, h, y, sg, True, lat, 4.0, *first, "the first network")
        same_bits(flat(call(s, "dens", lat, 4.0, y, sg, True)), flat(one), "the kept lists")
        s.set_observation_points(*moved)                   # the same count, the same lattice, the same c: the lists must not survive
        check_general(call(s, "dens", lat, 4.0, y, sg, True), define_obs(x, *moved), y, sg, True, lat, 4.0, *moved, "the moved points")
        check_general(call(s, "dens", lat, 1.5, y, sg, True), define_obs(x, *moved), y, sg, True, lat, 1.5, *moved, "another c")
        other = ((3, 2), (-3, 3), 8)                       # another origin
        check_general(call(s, "dens", other, 1.5, y, sg, True), define_obs(x, *moved), y, sg, True, other, 1.5, *moved, "another origin")
        check_general(call(s, "dens", lat, 32.0, y, sg, True), define_obs(x, *moved), y, sg, True, lat, 32.0, *moved, "longer lists")
        s.set_observation_points(*fewer)                   # a smaller network: shorter lists in the same buffers
        check_general(call(s, "dens", lat, 32.0, y[:65], sg[:65], True), define_obs(x, *fewer), y[:65], sg[:65], True, lat, 32.0, *fewer, "fewer points")


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(9)
    n, members, p = 13, 5, 65
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    cols, rows = network(n, p, rng)
    dp, fp, ip = C.POINTER(C.c_double), capi._MF, C.POINTER(C.c_int)
    nodes = 25
    gram, rhs, dd = np.full((nodes, members, members), 7.0), np.full((nodes, members), 7.0), np.full(nodes, 7.0)
    counts = np.full(nodes, 7, np.int32)
    ones = np.ones(p, F32)
    sig = ones.copy()
    sig[17] = np.inf
    g = lambda a: a.ctypes.data_as(dp)
    f = lambda a: a.ctypes.data_as(fp)
    cn = counts.ctypes.data_as(ip)
    name = b"fluid_observation_gram_lattice"

    def refused(rc, *words):
        assert rc == capi.E_INVALID
        msg = L.fluid_last_error()
        assert all(word in msg for word in (name,) + words), msg

    def lattice(hnd, field=2, obs=None, sigma=None, shape=(5, 5), origin=(-1, -1), step=8, c=8.0, out=True, r=None, d=None):
        return L.fluid_observation_gram_lattice(hnd, field, 1, obs, sigma, shape[0], shape[1], origin[0], origin[1], step, c,
                                                g(gram) if out else None, r, d, cn)

    with solver(n, members) as s, solver(n, members) as twin:
        for c in (s, twin):
            c.timing_enable(True)
            c.upload_members(**fields)
            c.step(use_sources=True)
            c.add_source("dens", "dens_prev", DT)                      # a lazy state that must survive the refusals
        refused(lattice(s._h), b"no observation network")
        s.set_observation_points(cols, rows)                           # (host work and one copy: no launch)
        refused(lattice(s._h, out=False), b"gram")
        refused(lattice(s._h, r=g(rhs)), b"rhs", b"obs")
        refused(lattice(s._h, sigma=f(ones), d=g(dd)), b"dd", b"obs")
        refused(lattice(None), b"null context")
        for field in (12, -1):
            refused(lattice(s._h, field=field), b"bad field id %d" % field)
        refused(lattice(s._h, shape=(0, 5)), b"nodes_row = 0 is below 1")
        refused(lattice(s._h, shape=(5, -2)), b"nodes_col = -2 is below 1")
        refused(lattice(s._h, shape=(64, 65)), b"4160", b"FLUID_LATTICE_MAX_NODES = 4096")
        refused(lattice(s._h, shape=(1 << 20, 1 << 20)), b"FLUID_LATTICE_MAX_NODES = 4096")
        for step in (0, -8, 4, 12, 7):
            refused(lattice(s._h, step=step), b"step = %d is not a positive multiple of 8" % step)
        for c in (0.0, -1.0, np.nan, np.inf):
            refused(lattice(s._h, c=c), b"c = ", b"not finite or not above 0")
        refused(lattice(s._h, obs=f(ones), sigma=f(sig), r=g(rhs), d=g(dd)), b"inv_sigma[17]")
        # more (point, node) pairs than FLUID_LATTICE_GRAM_MAX_ENTRIES: 2^20 points, each inside all 25 supports
        big = capi.OBSERVE_MAX_POINTS
        s.set_observation_points(rng.uniform(0.5, n + 0.5, big).astype(F32), rng.uniform(0.5, n + 0.5, big).astype(F32))
        refused(lattice(s._h, c=1e6), b"%d" % (25 * big), b"FLUID_LATTICE_GRAM_MAX_ENTRIES = %d" % capi.LATTICE_GRAM_MAX_ENTRIES)
        assert 25 * big > capi.LATTICE_GRAM_MAX_ENTRIES == 1 << 24
        assert (gram == 7.0).all() and (rhs == 7.0).all() and (dd == 7.0).all() and (counts == 7).all()
        ta, tb = s.timing_read(reset=False), twin.timing_read(reset=False)
        assert ta == {**tb, **{k: ta[k] for k in ta if k.endswith("_ms")}}             # every count; the times are times
        for fname in capi.FIELD_NAMES:
            assert np.array_equal(s.download_members(fname).view(np.uint32), twin.download_members(fname).view(np.uint32)), fname
        for c in (s, twin):
            c.step(use_sources=True)
        for fname in ("u", "v", "dens"):
            assert np.array_equal(s.download_members(fname).view(np.uint32), twin.download_members(fname).view(np.uint32)), fname
        s.set_observation_points(cols, rows)
        assert lattice(s._h, obs=f(ones), sigma=f(ones), r=g(rhs), d=g(dd)) == capi.OK     # the context is usable, the arrays are written
        assert not (gram == 7.0).any() and not (counts == 7).all()
    # the member cap: one member too many
    big = capi.TRANSFORM_MAX_MEMBERS + 1
    with solver(2, big) as s:
        s.upload_members(u=rng.uniform(-1.0, 1.0, (big, 4, 4)).astype(F32))
        s.set_observation_points([1.5], [2.25])
        out = np.full((big, big), 7.0)
        refused(L.fluid_observation_gram_lattice(s._h, 0, 1, None, None, 1, 1, 1, 1, 8, 1.0, g(out), None, None, None), b"65", b"64")
        assert (out == 7.0).all()
    # row slabs
    with F().FluidSolver(n, rank=0, nranks=2) as s:
        d1 = np.full(1, 7.0)
        refused(L.fluid_observation_gram_lattice(s._h, 0, 0, None, None, 1, 1, 1, 1, 8, 1.0, g(d1), None, None, None), b"slab")
        assert d1[0] == 7.0


# ---- 10. one LETKF cycle, end to end ----------------------------------------------------------------------------------------------------
def test_one_letkf_cycle():
    n, members, p, shape, origin, step, c = 30, 8, 200, (5, 5), (-1, -1), 8, 8.0
    rng = np.random.default_rng(10)
    w = n + 2
    k = np.arange(w)
    bump = lambda cx, cy, r: np.exp(-((k[None, :] - cx) ** 2 + (k[:, None] - cy) ** 2) / (2.0 * r * r))
    start = lambda: {"dens": (bump(rng.uniform(8, 22), rng.uniform(8, 22), rng.uniform(3, 6)) * rng.uniform(0.5, 2.0)).astype(F32),
                     "u": rng.uniform(-1.0, 1.0, (w, w)).astype(F32), "v": rng.uniform(-1.0, 1.0, (w, w)).astype(F32)}
    spread = [start() for _ in range(members)]
    truth = start()
    cols, rows = network(n, p, rng)
    inv_sigma = rng.uniform(5.0, 20.0, p).astype(F32)
    with solver(n, 1) as t:                               # the ninth simulation: where the observed values come from
        t.upload(**truth)
        t.step(3)
        t.set_observation_points(cols, rows)
        y = t.observe("dens")[0]
    with solver(n, members) as s, solver(n, members) as twin:
        s.upload_members(**{f: np.stack([m[f] for m in spread]) for f in ("dens", "u", "v")})
        s.step(3)
        s.set_observation_points(cols, rows)
        before = s.download_members("dens")
        yk = s.observe("dens")
        gram, rhs, dd, counts = s.observation_gram_lattice("dens", shape, origin, step, c, obs=y, inv_sigma=inv_sigma, centre=True)
        check_general((gram, rhs, dd, counts), yk, y, inv_sigma, True, (shape, origin, step), c, cols, rows, "the cycle")
        assert (counts > 0).any()
        # per node the ETKF in ensemble space, on the host: Pa = [(M - 1) I + C_b]^-1, mean weights Pa rhs_b, W = sqrt((M - 1) Pa);
        # D_b = T_b - I, and 0 at a node that sees no point
        eye = np.eye(members)
        anom = eye - np.ones((members, members)) / members
        incr = np.zeros(shape + (members, members), F32)
        for ia in range(shape[0]):
            for ib in range(shape[1]):
                if counts[ia, ib] == 0:
                    continue
                lam, vec = np.linalg.eigh((members - 1) * eye + gram[ia, ib])
                assert lam.min() >= (members - 1) - 1e-9 * lam.max()
                wmean = vec @ ((vec.T @ rhs[ia, ib]) / lam)
                wpert = vec @ np.diag(np.sqrt((members - 1) / lam)) @ vec.T
                tmat = np.ones((members, members)) / members + anom @ (wpert + wmean[:, None])
                incr[ia, ib] = (tmat - eye).astype(F32)
        assert np.isfinite(incr).all() and incr.any()
        s.transform_lattice(incr, origin, step, ("dens",))
        after = s.download_members("dens")
        # rule 5 of the lattice update: a cell on a node gets exactly that node's transform_local result
        twin.upload_members(dens=before)
        nrow, ncol = node_positions(shape, origin, step)
        on = [(ia, ib) for ia in range(shape[0]) for ib in range(shape[1]) if 0 <= nrow[ia] < w and 0 <= ncol[ib] < w]
        assert len(on) == 16
        for ia, ib in on:
            twin.transform_local(incr[ia, ib], box=(nrow[ia], nrow[ia] + 1, ncol[ib], ncol[ib] + 1), fields=("dens",))
        local = twin.download_members("dens")
        for ia, ib in on:
            same_bits(after[:, nrow[ia], ncol[ib]], local[:, nrow[ia], ncol[ib]], "the cell on node (%d, %d)" % (ia, ib))
        # the misfit of the ensemble mean at the points does not grow.  The observations are linear in the cells, and every cell's
        # transform is a convex combination of its corner nodes' I + D_b: new_obs = sum_k T[k][m] taps up to one float rounding of
        # each new cell and at most six in each interpolation on either side, 13 * 2^-24 < 2^-20 relative to sum_k |T[k][m]| max
        # |taps of member k at p| with |T| <= the largest |I + D_b| over the nodes -- the slack of tests/test_gpu_observe.py
        new = s.observe("dens")
        same_bits(new, define_obs(after, cols, rows), "the observations after")
        taps, _ = stencil(before, cols, rows)
        tapmax = np.max(np.abs(np.stack(taps)).astype(np.float64), axis=0)           # (M, P)
        tabs = np.abs(incr.astype(np.float64) + eye).max(axis=(0, 1))
        bound = 2.0 ** -20 * (tabs.T @ tapmax)
        sg = inv_sigma.astype(np.float64)
        misfit = lambda obs: math.sqrt(math.fsum((((y.astype(np.float64) - obs.astype(np.float64).mean(axis=0)) * sg) ** 2)))
        slack = math.sqrt(math.fsum((bound.mean(axis=0) * sg) ** 2))
        print("misfit of the mean: %.6g before, %.6g after (slack %.3g)" % (misfit(yk), misfit(new), slack))
        assert misfit(new) <= misfit(yk) + slack
