"""GPU: observing ensembles -- fluid_set_observation_points, fluid_observe_members(_host), fluid_observation_gram
(include/fluid_amd.h, "observing ensembles").

Every expected value comes from the header's definition written in numpy: `define_obs`, the float32 bilinear sample operation
by operation on what download_members (the pack) showed before the call, and `operands`, the float64 chain -- the
member-order mean, its subtraction, the multiplication by 1 / sigma.  Observations are compared bit for bit.  The Gram
results are compared with `==` on dyadic data, where every partial sum is representable, and on general data against the
textbook bound of a recursive double sum of P terms in any order, gamma = (P + 2) u / (1 - (P + 2) u) times the sum of the
|products|, u = 2^-53 (the + 2: the reference's own rounded products and final rounding) -- derived, not measured."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZES = [1, 6, 13, 30, 61]
MEMBERS = [1, 2, 3, 9, 64]
POINTS = [1, 2, 63, 64, 65, 257, 5000]      # around a wave and a block of lanes, several blocks
GRAM_MEMBERS = [1, 2, 3, 5, 8, 9, 17, 32, 33, 64]   # every padded count and the counts just past one
GRAM_POINTS = [1, 64, 65, 513, 5000]        # less than a chunk of 64 points, a chunk and one more, more blocks than fold lanes
COARSE = np.array([-1, -0.5, -0.25, 0.0, -0.0, 0.25, 0.5, 1], F32)
MAIN = ("u", "v", "dens", "u_prev", "v_prev", "dens_prev")
COUNTS = ("sweeps", "solves", "jacobi_launches", "jacobi_field_launches", "pressure_sweeps")
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


def exact_sums(a, d, bits):
    """(gram, rhs, dd) as exact sums for operands that are multiples of 2^-bits: integer arithmetic, a sample of entries held
    against math.fsum of the exact products"""
    m = a.shape[0]
    rows = a if d is None else np.vstack([a, d[None]])
    i = np.ldexp(rows, bits)
    assert (i == np.rint(i)).all() and np.abs(i).max() < 2 ** 22
    i = i.astype(np.int64)
    full = i @ i.T
    assert np.abs(full).max() < 2 ** 53
    g = np.ldexp(full.astype(np.float64), -2 * bits)
    for k, j in {(0, 0), (0, m - 1), (m - 1, m - 1), (m // 2, m // 3), (rows.shape[0] - 1, 0), (rows.shape[0] - 1, rows.shape[0] - 1)}:
        assert g[k, j] == math.fsum(rows[k] * rows[j])
    if d is None:
        return g, None, None
    return g[:m, :m], g[:m, m], g[m, m]


def fsum_all(a, d, absolute=False):
    rows = a if d is None else np.vstack([a, d[None]])
    k = rows.shape[0]
    g = np.empty((k, k), np.float64)
    for i in range(k):
        for j in range(i, k):
            p = rows[i] * rows[j]
            g[i, j] = g[j, i] = math.fsum(np.abs(p) if absolute else p)
    return g


def gamma(p):
    return (p + 2) * U / (1 - (p + 2) * U)


def pack_results(m, got):
    """(gram, rhs, dd) or gram as one (M + 1, M + 1) / (M, M) symmetric matrix, as fsum_all lays them out"""
    if not isinstance(got, tuple):
        return got
    g, rhs, dd = got
    out = np.empty((m + 1, m + 1), np.float64)
    out[:m, :m], out[:m, m], out[m, :m], out[m, m] = g, rhs, rhs, dd
    return out


def within_bound(got, a, d, what):
    m, p = a.shape
    want, mag = fsum_all(a, d), fsum_all(a, d, absolute=True)
    bound = gamma(p) * mag
    err = np.abs(pack_results(m, got) - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: largest error / bound = %.4f" % (what, ratio))
    assert (err <= bound).all(), "%s: %d entries outside the summation bound (largest ratio %.3g)" % (what, int((err > bound).sum()), ratio)


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
    assert np.array_equal(g.view(np.uint64), g.T.view(np.uint64)), "%s: not bit-symmetric" % what


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


def hip_runtime():
    """the HIP runtime this process already holds (the one libfluid_amd.so runs on)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            lib = C.CDLL(line.split()[-1])
            lib.hipMalloc.argtypes, lib.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
            lib.hipFree.argtypes, lib.hipFree.restype = [C.c_void_p], C.c_int
            return lib
    raise RuntimeError("no HIP runtime is loaded")


def arbitrary(rng, shape):
    return (rng.normal(size=shape) * 10.0 ** rng.uniform(-3, 3, size=shape)).astype(F32)


# ---- 1. observation values, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n", SIZES)
def test_observation_values_bit_for_bit(n, storage):
    rng = np.random.default_rng(100 * n + storage)
    w = n + 2
    nets = {p: network(n, p, rng) for p in POINTS}
    for members in MEMBERS:
        with solver(n, members, storage) as s:
            s.upload_members(dens=arbitrary(rng, (members, w, w)) if storage == 0 else rng.uniform(-4.0, 4.0, (members, w, w)).astype(F32),
                             u=rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32), v=rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32))
            s.vel_step()                               # fp16 storage: u_prev, the pressure, is held scaled
            for field in ("dens", "u_prev"):
                before = s.download_members(field)
                for p in POINTS:
                    cols, rows = nets[p]
                    s.set_observation_points(cols, rows)
                    assert s.observation_points() == p
                    what = "n=%d M=%d storage=%d %s P=%d" % (n, members, storage, field, p)
                    got = s.observe(field)
                    same_bits(got, define_obs(before, cols, rows), what)
                    dev = s.observe_device(field)
                    assert tuple(dev.shape) == (members, p)
                    same_bits(dev.cpu().numpy(), got, what + ": observe_device against observe")
                assert np.array_equal(s.download_members(field).view(np.uint32), before.view(np.uint32)), "the call changed the field"


def test_a_cell_centre_returns_the_cell():
    n, members = 13, 3
    rng = np.random.default_rng(11)
    x = arbitrary(rng, (members, n + 2, n + 2))
    k = np.arange(1, n + 1)
    cols, rows = np.meshgrid(k, k)
    with solver(n, members) as s:
        s.upload_members(v=x)
        s.set_observation_points(cols.ravel(), rows.ravel())
        got = s.observe("v").reshape(members, n, n)
        assert np.array_equal(got, x[:, 1:-1, 1:-1])


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_a_non_finite_tap_reaches_its_stencils_only(storage):
    n, members, bad = 13, 5, 2
    rng = np.random.default_rng(12 + storage)
    x = rng.uniform(-1.0, 1.0, (members, n + 2, n + 2)).astype(F32)
    cols, rows = network(n, 5000, rng)
    with solver(n, members, storage) as s:
        s.upload_members(dens=x)
        s.set_observation_points(cols, rows)
        clean = s.observe("dens")
        assert np.isfinite(clean).all()
        x[bad, 7, 4] = np.nan                          # row 7, column 4
        x[bad, 0, 9] = np.inf                          # the ghost ring is read like any cell
        s.upload_members(dens=x)
        got = s.observe("dens")
        same_bits(got, define_obs(s.download_members("dens"), cols, rows), "with a NaN and an inf")
        j0, i0 = cols.astype(np.int64), rows.astype(np.int64)
        hit = (((i0 == 7) | (i0 == 6)) & ((j0 == 4) | (j0 == 3))) | ((i0 == 0) & ((j0 == 9) | (j0 == 8)))
        assert hit.any() and not np.isfinite(got[bad][hit]).any(), "a zero weight must not hide a non-finite tap"
        keep = np.ones_like(got, bool)
        keep[bad, hit] = False
        assert np.array_equal(got.view(np.uint32)[keep], clean.view(np.uint32)[keep]), "a non-finite tap changed another value"


def test_member_stride_leaves_the_floats_in_between():
    import torch
    n, members, p = 13, 9, 257
    rng = np.random.default_rng(13)
    cols, rows = network(n, p, rng)
    stride = p + 7
    with solver(n, members) as s:
        s.upload_members(u=arbitrary(rng, (members, n + 2, n + 2)))
        s.set_observation_points(cols, rows)
        want = s.observe("u")
        out = torch.full((members * stride + 5,), 7.0, dtype=torch.float32, device="cuda")
        assert s.observe_device("u", out=out, member_stride=stride) is out
        host = out.cpu().numpy()
        body = host[:members * stride].reshape(members, stride)
        same_bits(np.ascontiguousarray(body[:, :p]), want, "strided")
        assert (body[:, p:] == 7.0).all() and (host[members * stride:] == 7.0).all()
        exact = torch.full((members * p,), 7.0, dtype=torch.float32, device="cuda")
        s.observe_device("u", out=exact, member_stride=p)
        same_bits(exact.cpu().numpy().reshape(members, p), want, "stride = P")


# ---- 2. lazy state ---------------------------------------------------------------------------------------------------------
def prepared(n, members, storage, fields, case):
    """a context in one of the lazy states, and the field the state is about (as in tests/test_gpu_gram.py)"""
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
    members, n = 3, 30
    rng = np.random.default_rng(2000 * storage + len(case))
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    cols, rows = network(n, 257, rng)
    a, f = prepared(n, members, storage, fields, case)
    b, _ = prepared(n, members, storage, fields, case)
    with a, b:
        a.set_observation_points(cols, rows)
        got = a.observe_device(f).cpu().numpy()
        gram, rhs, dd = a.observation_gram(f, obs=np.zeros(257, F32), centre=False)
        shown = a.download_members(f)
        if case == "zeros":
            assert not shown.view(np.uint32).any() and not got.view(np.uint32).any() and not gram.view(np.uint64).any()
        else:
            assert np.abs(shown[:, 1:-1, 1:-1]).max() > 0
        want = define_obs(shown, cols, rows)
        same_bits(got, want, "storage=%d %s" % (storage, case))
        same_bits(a.observe(f), want, "storage=%d %s: the host call" % (storage, case))
        within_bound((gram, rhs, dd), *operands(want, np.zeros(257, F32), None, False), "storage=%d %s" % (storage, case))
        for name in capi.FIELD_NAMES:          # every field of every member, against the twin that never observed
            assert np.array_equal(a.download_members(name).view(np.uint32), b.download_members(name).view(np.uint32)), name
        ta, tb = a.timing_read(reset=False), b.timing_read(reset=False)
        assert {k: ta[k] for k in COUNTS} == {k: tb[k] for k in COUNTS}
        for s in (a, b):
            s.step(use_sources=True)
        for name in ("u", "v", "dens"):
            assert np.array_equal(a.download_members(name).view(np.uint32), b.download_members(name).view(np.uint32)), name + " a step later"
        ta, tb = a.timing_read(reset=False), b.timing_read(reset=False)
        assert {k: ta[k] for k in ta if not k.endswith("_ms")} == {k: tb[k] for k in tb if not k.endswith("_ms")}


# ---- 3. the member index in the grid ---------------------------------------------------------------------------------------
def test_21845_members():
    from fluidsimulationcuda_amd import capi
    members, n = capi.MAX_MEMBERS, 6
    assert members == 21845
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.0, 1.0, (members, n + 2, n + 2)).astype(F32)
    cols = np.array([0.5, 6.5, 3.0, 2.25, 5.75], F32)
    rows = np.array([0.5, 6.5, 4.0, 6.125, 1.5], F32)
    with solver(n, members) as s:
        s.upload_members(v=x)
        s.set_observation_points(cols, rows)
        want = define_obs(x, cols, rows)
        got = s.observe("v")
        same_bits(got, want, "M=21845")
        same_bits(s.observe_device("v").cpu().numpy(), want, "M=21845 on the device")


# ---- 4. the network: replacing, clearing, refusing -------------------------------------------------------------------------
def test_replacing_and_clearing_the_network():
    from fluidsimulationcuda_amd import capi
    n, members = 13, 3
    rng = np.random.default_rng(4)
    x = arbitrary(rng, (members, n + 2, n + 2))
    with solver(n, members) as s:
        s.upload_members(dens=x)
        assert s.observation_points() == 0
        with pytest.raises(capi.FluidError, match="fluid_observe_members_host.*no observation network"):
            s.observe("dens")
        first, second = network(n, 65, rng), network(n, 5000, rng)
        s.set_observation_points(*first)
        same_bits(s.observe("dens"), define_obs(x, *first), "the first network")
        assert s.observation_gram("dens").shape == (members, members)
        s.set_observation_points(*second)                     # larger: the Gram scratch grows with it
        assert s.observation_points() == 5000
        same_bits(s.observe("dens"), define_obs(x, *second), "the second network")
        a, _ = operands(define_obs(x, *second), None, None, True)
        within_bound(s.observation_gram("dens"), a, None, "after the network grew")
        s.set_observation_points(first[0][:3], first[1][:3])
        same_bits(s.observe("dens"), define_obs(x, first[0][:3], first[1][:3]), "the third network")
        # a refused network leaves the old one in place; the message names the point
        for bad, word in ((np.nan, b"col"), (0.49, b"col"), (n + 0.51, b"col"), (np.inf, b"col")):
            cols = np.array([1.0, 2.0, bad], F32)
            with pytest.raises(capi.FluidError, match="fluid_set_observation_points: point 2: col"):
                s.set_observation_points(cols, np.ones(3, F32))
            with pytest.raises(capi.FluidError, match="fluid_set_observation_points: point 1: row"):
                s.set_observation_points(np.ones(3, F32), np.array([1.0, bad, 2.0], F32))
        assert s.observation_points() == 3
        same_bits(s.observe("dens"), define_obs(x, first[0][:3], first[1][:3]), "after the refusals")
        s.set_observation_points([], [])
        assert s.observation_points() == 0
        with pytest.raises(capi.FluidError, match="fluid_observation_gram.*no observation network"):
            s.observation_gram("dens")
        assert np.array_equal(s.download_members("dens").view(np.uint32), x.view(np.uint32))


def test_refusals_change_nothing():
    import torch
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(5)
    n, members, p = 6, 5, 65
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    cols, rows = network(n, p, rng)
    dp, fp = C.POINTER(C.c_double), capi._MF
    gram, rhs, dd = np.full((members, members), 7.0), np.full(members, 7.0), np.full(1, 7.0)
    host = np.full((members, p), 7.0, F32)
    dev = torch.full((members * p,), 7.0, dtype=torch.float32, device="cuda")
    hip = hip_runtime()
    exact, size = C.c_void_p(), 1 << 20
    assert hip.hipMalloc(C.byref(exact), C.c_size_t(size)) == 0
    fits = exact.value + size - members * p * 4         # an array of all members that ends with its allocation
    short = fits + 4                                    # ... and one that is one float too short
    ones = np.ones(p, F32)
    sig = ones.copy()
    sig[17] = np.inf

    def refused(rc, *words):
        assert rc == capi.E_INVALID
        msg = L.fluid_last_error()
        assert all(word in msg for word in words), msg

    with solver(n, members) as s, solver(n, members) as twin:
        for c in (s, twin):
            c.timing_enable(True)
            c.upload_members(**fields)
            c.step(use_sources=True)
            c.add_source("dens", "dens_prev", DT)                      # a lazy state that must survive the refusals
        g = lambda a: a.ctypes.data_as(dp)
        f = lambda a: a.ctypes.data_as(fp)
        # no network yet
        refused(L.fluid_observe_members(s._h, 2, dev.data_ptr(), 0), b"fluid_observe_members", b"no observation network")
        refused(L.fluid_observe_members_host(s._h, 2, f(host)), b"fluid_observe_members_host", b"no observation network")
        refused(L.fluid_observation_gram(s._h, 2, 1, None, None, g(gram), None, None), b"fluid_observation_gram", b"no observation network")
        # the network itself
        refused(L.fluid_set_observation_points(s._h, f(cols), f(rows), -1), b"fluid_set_observation_points", b"npoints -1")
        big = np.ones(capi.OBSERVE_MAX_POINTS + 1, F32)
        refused(L.fluid_set_observation_points(s._h, f(big), f(big), big.size), b"fluid_set_observation_points", b"1048577")
        refused(L.fluid_set_observation_points(s._h, None, f(rows), p), b"fluid_set_observation_points", b"col")
        refused(L.fluid_observation_points(s._h, None), b"fluid_observation_points", b"npoints")
        count = C.c_int(-1)
        assert L.fluid_observation_points(s._h, C.byref(count)) == capi.OK and count.value == 0
        s.set_observation_points(cols, rows)                           # (host work and one copy: no launch)
        for field in (12, -1):
            word = b"bad field id %d" % field
            refused(L.fluid_observe_members(s._h, field, dev.data_ptr(), 0), b"fluid_observe_members", word)
            refused(L.fluid_observe_members_host(s._h, field, f(host)), b"fluid_observe_members_host", word)
            refused(L.fluid_observation_gram(s._h, field, 1, None, None, g(gram), None, None), b"fluid_observation_gram", word)
        refused(L.fluid_observe_members(s._h, 2, None, 0), b"fluid_observe_members", b"out_dev")
        refused(L.fluid_observe_members(s._h, 2, dev.data_ptr(), p - 1), b"fluid_observe_members", b"member_stride 64", b"65")
        refused(L.fluid_observe_members(s._h, 2, short, 0), b"fluid_observe_members", b"out_dev", b"allocation ends")
        refused(L.fluid_observe_members(s._h, 2, dev.data_ptr(), 1 << 40), b"fluid_observe_members", b"out_dev", b"allocation ends")
        refused(L.fluid_observe_members(s._h, 2, host.ctypes.data, 0), b"fluid_observe_members", b"not device memory")
        refused(L.fluid_observe_members_host(s._h, 2, None), b"fluid_observe_members_host", b"host")
        refused(L.fluid_observation_gram(s._h, 2, 1, None, None, None, None, None), b"fluid_observation_gram", b"gram")
        refused(L.fluid_observation_gram(s._h, 2, 1, None, None, g(gram), g(rhs), None), b"fluid_observation_gram", b"rhs", b"obs")
        refused(L.fluid_observation_gram(s._h, 2, 1, None, f(ones), g(gram), None, g(dd)), b"fluid_observation_gram", b"dd", b"obs")
        refused(L.fluid_observation_gram(s._h, 2, 1, f(ones), f(sig), g(gram), g(rhs), g(dd)), b"fluid_observation_gram", b"inv_sigma[17]")
        assert (gram == 7.0).all() and (rhs == 7.0).all() and (dd == 7.0).all() and (host == 7.0).all()
        assert (dev.cpu().numpy() == 7.0).all()
        ta, tb = s.timing_read(reset=False), twin.timing_read(reset=False)
        assert ta == {**tb, **{k: ta[k] for k in ta if k.endswith("_ms")}}             # every count; the times are times
        for name in capi.FIELD_NAMES:
            assert np.array_equal(s.download_members(name).view(np.uint32), twin.download_members(name).view(np.uint32)), name
        for c in (s, twin):
            c.step(use_sources=True)
        for name in ("u", "v", "dens"):
            assert np.array_equal(s.download_members(name).view(np.uint32), twin.download_members(name).view(np.uint32)), name
        assert L.fluid_observe_members(s._h, 2, fits, 0) == capi.OK        # ends with its allocation
        s.synchronize()
    assert hip.hipFree(exact) == 0
    # the cap of the Gram call: one member too many; the observations themselves have no such cap
    big = capi.TRANSFORM_MAX_MEMBERS + 1
    with solver(2, big) as s:
        x = rng.uniform(-1.0, 1.0, (big, 4, 4)).astype(F32)
        s.upload_members(u=x)
        s.set_observation_points([1.5], [2.25])
        out = np.full((big, big), 7.0)
        for centre in (0, 1):
            refused(L.fluid_observation_gram(s._h, 0, centre, None, None, out.ctypes.data_as(dp), None, None), b"fluid_observation_gram", b"65", b"64")
        assert (out == 7.0).all()
        same_bits(s.observe("u"), define_obs(x, [1.5], [2.25]), "65 members")
    # row slabs: all five calls
    with F().FluidSolver(n, rank=0, nranks=2) as s:
        one, count = np.full(1, 1.5, F32), C.c_int(7)
        d1 = np.full(1, 7.0)
        refused(L.fluid_set_observation_points(s._h, f(one), f(one), 1), b"fluid_set_observation_points", b"slab")
        refused(L.fluid_observation_points(s._h, C.byref(count)), b"fluid_observation_points", b"slab")
        refused(L.fluid_observe_members(s._h, 0, dev.data_ptr(), 0), b"fluid_observe_members", b"slab")
        refused(L.fluid_observe_members_host(s._h, 0, f(one)), b"fluid_observe_members_host", b"slab")
        refused(L.fluid_observation_gram(s._h, 0, 0, None, None, g(d1), None, None), b"fluid_observation_gram", b"slab")
        assert count.value == 7 and one[0] == 1.5 and d1[0] == 7.0


# ---- 5. the Gram matrix on dyadic data: exact --------------------------------------------------------------------------------
def dyadic_case(rng, n, members, p):
    x = rng.choice(COARSE, size=(members, n + 2, n + 2)).astype(F32)
    cols, rows = network(n, p, rng, quarter=True)
    y = (rng.integers(-8, 9, p) / 4.0).astype(F32)
    sg = rng.choice(np.array([0.5, 1.0, 2.0], F32), p)
    return x, cols, rows, y, sg


def check_dyadic(a, b, x, cols, rows, y, sg, members, what):
    """every combination of centre / obs / inv_sigma on context a, exact; the same bits again and on context b"""
    h = define_obs(x, cols, rows)                  # multiples of 2^-6, exact in float32
    assert np.array_equal(a.observe("dens"), h)
    for centre in (False, True):
        if centre and members & (members - 1):    # a power of two: the mean, the anomalies and the products are exact
            continue
        for obs, sigma in ((None, None), (y, None), (None, sg), (y, sg)):
            w = "%s centre=%s obs=%s sigma=%s" % (what, centre, obs is not None, sigma is not None)
            got = a.observation_gram("dens", obs=obs, inv_sigma=sigma, centre=centre)
            am, d = operands(h, obs, sigma, centre)
            gram, rhs, dd = exact_sums(am, d, 14)
            first = pack_results(members, got)
            equal(got[0] if obs is not None else got, gram, w)
            symmetric(got[0] if obs is not None else got, w)
            if obs is not None:
                equal(got[1], rhs, w + ": rhs")
                equal(got[2], dd, w + ": dd")
            same_bits(pack_results(members, a.observation_gram("dens", obs=obs, inv_sigma=sigma, centre=centre)), first, w + ": two calls in a row")
            same_bits(pack_results(members, b.observation_gram("dens", obs=obs, inv_sigma=sigma, centre=centre)), first, w + ": a second context")
            if sigma is None:                      # a null inv_sigma gives the bits that all ones give
                ones = a.observation_gram("dens", obs=obs, inv_sigma=np.ones(len(cols), F32), centre=centre)
                same_bits(pack_results(members, ones), first, w + ": all ones")


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", GRAM_MEMBERS)
def test_gram_exact_on_dyadic_data(members, storage):
    rng = np.random.default_rng(5000 + 100 * storage + members)
    n = 13
    with solver(n, members, storage) as a, solver(n, members, storage) as b:
        for p in GRAM_POINTS:
            x, cols, rows, y, sg = dyadic_case(rng, n, members, p)
            for c in (a, b):
                c.upload_members(dens=x)
                c.set_observation_points(cols, rows)
            check_dyadic(a, b, x, cols, rows, y, sg, members, "M=%d storage=%d P=%d" % (members, storage, p))
            assert np.array_equal(a.download_members("dens").view(np.uint32), x.view(np.uint32)), "the call changed the field"


@pytest.mark.parametrize("members", [2, 32, 64])
def test_gram_exact_with_several_chunks_per_block(members):
    """more chunks of 64 points than the grid has blocks (512 at 64 members, 1024 below): a block strides over its chunks"""
    rng = np.random.default_rng(5500 + members)
    n, p = 13, 70000
    assert p > 64 * 1024
    x, cols, rows, y, sg = dyadic_case(rng, n, members, p)
    with solver(n, members) as a:
        a.upload_members(dens=x)
        a.set_observation_points(cols, rows)
        h = define_obs(x, cols, rows)
        for centre in (False, True):
            got = a.observation_gram("dens", obs=y, inv_sigma=sg, centre=centre)
            gram, rhs, dd = exact_sums(*operands(h, y, sg, centre), 14)
            what = "M=%d P=%d centre=%s" % (members, p, centre)
            equal(got[0], gram, what)
            equal(got[1], rhs, what + ": rhs")
            equal(got[2], dd, what + ": dd")
            symmetric(got[0], what)
            same_bits(pack_results(members, a.observation_gram("dens", obs=y, inv_sigma=sg, centre=centre)), pack_results(members, got), what)


# ---- 6. general data within the summation bound --------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n,members,p", [(61, 5, 513), (30, 9, 5000), (13, 33, 257), (13, 32, 257), (30, 64, 513), (6, 3, 65), (13, 1, 64)])
def test_gram_general_data_within_the_summation_bound(n, members, p, storage):
    rng = np.random.default_rng(6000 * storage + 10 * n + members)
    w = n + 2
    cols, rows = network(n, p, rng)
    with solver(n, members, storage) as s:
        s.set_observation_points(cols, rows)
        for scale in (1e-3, 1.0, 1e3):
            for centre in (False, True):
                x = rng.uniform(0.25, 1.0, (members, w, w)) * rng.choice([-1.0, 1.0], (members, w, w)) * scale
                if centre:
                    x = x + 50 * scale
                s.upload_members(v=x.astype(F32))
                before = s.download_members("v")
                h = define_obs(before, cols, rows)
                assert np.isfinite(h).all()
                y = (rng.normal(size=p) * scale + (50 * scale if centre else 0)).astype(F32)
                sg = (rng.uniform(0.5, 20.0, p) / scale).astype(F32)
                what = "n=%d M=%d P=%d storage=%d scale=%g centre=%s" % (n, members, p, storage, scale, centre)
                got = s.observation_gram("v", obs=y, inv_sigma=sg, centre=centre)
                within_bound(got, *operands(h, y, sg, centre), what)
                symmetric(got[0], what)
                alone = s.observation_gram("v", centre=centre)
                within_bound(alone, *operands(h, None, None, centre), what + ": gram alone")
                symmetric(alone, what)


# ---- 7. one member; non-finite values ---------------------------------------------------------------------------------------------
def test_one_member():
    n, p = 13, 513
    rng = np.random.default_rng(7)
    x, cols, rows, y, sg = dyadic_case(rng, n, 1, p)
    with solver(n, 1) as s:
        s.upload_members(dens=x)
        s.set_observation_points(cols, rows)
        h = define_obs(x, cols, rows).astype(np.float64)[0]
        g, rhs, dd = s.observation_gram("dens", obs=y, centre=False)
        assert g.shape == (1, 1) and g[0, 0] == math.fsum(h * h) and rhs[0] == math.fsum(h * y) and dd == math.fsum(y.astype(np.float64) ** 2)
        g, rhs, dd = s.observation_gram("dens", obs=y, centre=True)         # the one anomaly is zero
        assert g[0, 0] == 0 and rhs[0] == 0 and dd == math.fsum((y - h) ** 2)


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_poisoning(storage):
    members, n, p, bad = 5, 13, 513, 2
    rng = np.random.default_rng(70 + storage)
    w = n + 2
    x = rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32)
    cols, rows = network(n, p, rng)
    y = rng.normal(size=p).astype(F32)
    sg = rng.uniform(0.5, 2.0, p).astype(F32)
    with solver(n, members, storage) as s:
        s.upload_members(u=x)
        s.set_observation_points(cols, rows)
        clean = s.observation_gram("u", obs=y, inv_sigma=sg, centre=False)
        assert all(np.isfinite(v).all() for v in clean)
        # a non-finite observed value: rhs and dd only
        ybad = y.copy()
        ybad[100] = np.nan
        for centre in (False, True):
            ref = s.observation_gram("u", obs=y, inv_sigma=sg, centre=centre)
            g, rhs, dd = s.observation_gram("u", obs=ybad, inv_sigma=sg, centre=centre)
            same_bits(g, ref[0], "a NaN in y, centre=%s: the matrix" % centre)
            assert np.isnan(rhs).all() and np.isnan(dd)
        # a non-finite observation of member 2
        x[bad, 7, 4] = np.nan
        s.upload_members(u=x)
        assert np.isnan(s.observe("u")[bad]).any()
        g, rhs, dd = s.observation_gram("u", obs=y, inv_sigma=sg, centre=False)
        assert np.isnan(g[bad]).all() and np.isnan(g[:, bad]).all() and np.isnan(rhs[bad])
        keep = np.ones((members, members), bool)
        keep[bad] = keep[:, bad] = False
        assert np.array_equal(g.view(np.uint64)[keep], clean[0].view(np.uint64)[keep]), "a NaN in member 2 changed another entry"
        assert np.array_equal(np.delete(rhs, bad).view(np.uint64), np.delete(clean[1], bad).view(np.uint64))
        assert np.float64(dd).view(np.uint64) == np.float64(clean[2]).view(np.uint64)
        g, rhs, dd = s.observation_gram("u", obs=y, inv_sigma=sg, centre=True)
        assert np.isnan(g).all() and np.isnan(rhs).all() and np.isnan(dd)


# ---- 8. one assimilation cycle, end to end ----------------------------------------------------------------------------------------
def test_one_etkf_cycle():
    n, members, p = 30, 8, 40
    rng = np.random.default_rng(8)
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
    with solver(n, members) as s:
        s.upload_members(**{f: np.stack([m[f] for m in spread]) for f in ("dens", "u", "v")})
        s.step(3)
        s.set_observation_points(cols, rows)
        before = s.download_members("dens")
        yk = s.observe("dens")                            # (M, P): the observations before the update
        same_bits(yk, define_obs(before, cols, rows), "the observations before")
        c, rhs, dd = s.observation_gram("dens", obs=y, inv_sigma=inv_sigma, centre=True)
        assert np.isfinite(c).all() and c.any() and dd > 0
        # the ETKF in ensemble space, on the host: Pa = [(M - 1) I + C]^-1, mean weights Pa rhs, W = sqrt((M - 1) Pa)
        lam, vec = np.linalg.eigh((members - 1) * np.eye(members) + c)
        assert lam.min() >= (members - 1) - 1e-9 * lam.max()
        wmean = vec @ ((vec.T @ rhs) / lam)
        wpert = vec @ np.diag(np.sqrt((members - 1) / lam)) @ vec.T
        anom = np.eye(members) - np.ones((members, members)) / members
        tmat = (np.ones((members, members)) / members + anom @ (wpert + wmean[:, None])).astype(F32)
        s.transform(tmat, ("dens",))
        new = s.observe("dens")
        same_bits(new, define_obs(s.download_members("dens"), cols, rows), "the observations after")
        # H is linear: new_obs[m][p] = sum_k T[k][m] Y[k][p] up to one float rounding of each new cell (2^-24) and at most six in
        # each interpolation, on either side: 13 * 2^-24 < 2^-20, relative to sum_k |T[k][m]| max |taps of member k at p|
        taps, _ = stencil(before, cols, rows)
        tapmax = np.max(np.abs(np.stack(taps)).astype(np.float64), axis=0)           # (M, P)
        t64 = tmat.astype(np.float64)
        want = t64.T @ yk.astype(np.float64)                                          # [m][p]
        bound = 2.0 ** -20 * (np.abs(t64).T @ tapmax)
        err = np.abs(new.astype(np.float64) - want)
        print("linearity: largest error / bound = %.4f" % float((err / bound).max()))
        assert (err <= bound).all()
        # the scaled misfit of the ensemble mean in observation space does not grow: I - HK = (I + Y Y^T / (M - 1))^-1
        sg = inv_sigma.astype(np.float64)
        misfit = lambda obs: math.sqrt(math.fsum((((y.astype(np.float64) - obs.astype(np.float64).mean(axis=0)) * sg) ** 2)))
        slack = math.sqrt(math.fsum((bound.mean(axis=0) * sg) ** 2))
        print("misfit of the mean: %.6g before, %.6g after (slack %.3g)" % (misfit(yk), misfit(new), slack))
        assert abs(misfit(yk) - math.sqrt(dd)) <= 1e-9 * math.sqrt(dd)
        assert misfit(new) <= misfit(yk) + slack
