"""GPU: lattice updates -- fluid_transform_members_lattice (include/fluid_amd.h, "lattice updates"): increment matrices
given at the nodes of a coarse lattice, blended bilinearly to every cell, every product on the old ensemble, in place:
X' = X + sum_b phi_b o (X D_b).

Every expected value comes from `define_lattice` below, rules 2 to 7 of the header in numpy: integer axis weights, up to
four corners in row-major node order, per corner the member-order node sum over the non-zero increments in double, the
blend s = phi * t, then s = s + phi * t, each rounded on its own, y = x_m + s rounded once, one rounding to float --
applied to what download_members (the pack) showed before the call -- then `narrow` (fp16 storage: one more rounding to
nearest even).  A (cell, member) no corner takes part in keeps what it held.  Everything is compared bit for bit; a NaN
is a NaN, its sign and payload are not compared.  There is no tolerance anywhere."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = np.float32
MEMBERS = [1, 2, 3, 5, 8, 9, 17, 32, 33, 64]   # every padded count 1, 2, 4 .. 64, and the counts just past a power of two
MAIN = ("u", "v", "dens", "u_prev", "v_prev", "dens_prev")
DT = 0.016
# (N, (nodes_row, nodes_col), step, (row0, col0)): W = 3, 8, 15, 32, 63 -- no multiple of a patch side but 8 and 32, one and
# several blocks of four patches; origins negative, inside and past the array on either side; with the 3 x 4 lattices inside
# the array all three branches of rule 2 occur on both axes
CASES = [
    (1, (1, 1), 8, (0, 0)),
    (1, (2, 2), 8, (-3, 1)),
    (6, (1, 3), 8, (2, -9)),
    (6, (3, 1), 16, (-20, 3)),
    (13, (2, 2), 8, (3, 4)),
    (13, (3, 4), 8, (-5, -10)),
    (30, (3, 4), 8, (4, 2)),
    (30, (2, 2), 16, (40, -40)),
    (30, (1, 1), 24, (-7, 50)),
    (61, (3, 4), 16, (7, 5)),
    (61, (2, 2), 24, (20, 13)),
    (61, (1, 3), 24, (100, -3)),
    (61, (3, 1), 8, (-7, 70)),
]


def F():
    import fluidsimulationcuda_amd as f
    return f


def solver(n, members, storage=0, **kw):
    return F().FluidSolver(n, members=members, storage=storage, **kw)


# ---- the definition ------------------------------------------------------------------------------------------------------
def axis_weights(w, nodes, origin, step):
    """rule 2 along one axis, per index 0 .. w-1: (a, t0, t1); integers in int64, one division and one subtraction in double"""
    q = np.arange(w, dtype=np.int64) - np.int64(origin)
    last = np.int64(nodes - 1) * np.int64(step)
    low = (q <= 0) | (nodes == 1)
    high = ~low & (q >= last)
    a = np.where(low, 0, np.where(high, nodes - 2, q // step))
    t1 = np.where(low, 0.0, np.where(high, 1.0, (q - a * step).astype(np.float64) / np.float64(step)))
    return a, 1.0 - t1, t1


def plain_blend(s, phi, t):
    return s + phi * t                        # numpy: the product rounded, then the sum rounded


def fused_blend(s, phi, t):
    """fma(phi, t, s): ONE rounding, emulated exactly -- what the contract forbids (finite values only)"""
    return np.array([float(Fraction(float(a)) + Fraction(float(b)) * Fraction(float(c))) for a, b, c in zip(s, phi, t)], np.float64)


def define_lattice(x, d, origin, step, corners=(0, 1, 2, 3), blend=plain_blend):
    """x: (M, W, W) float32, what the pack shows before the call; d: (nodes_row, nodes_col, M, M) float32, d[a, b, k, m] the
    weight of OLD member k in the INCREMENT of new member m at node (a, b); origin: (row0, col0).  The new members,
    float32.  `corners`: the order the corners are blended in (the contract: 0, 1, 2, 3 = row-major); `blend`: how a
    further corner joins the sum (the contract: product and sum rounded one after the other)."""
    x, d = np.asarray(x, F32), np.asarray(d, F32)
    members, w = x.shape[0], x.shape[-1]
    nr, nc = d.shape[:2]
    xd = x.astype(np.float64)
    a, t0, t1 = axis_weights(w, nr, origin[0], step)
    b, u0, u1 = axis_weights(w, nc, origin[1], step)
    s = np.zeros((members, w, w), np.float64)
    has = np.zeros((members, w, w), bool)                      # a corner has taken part
    with np.errstate(all="ignore"):
        for c in corners:
            da, db = c >> 1, c & 1
            na, nb = (a + da)[:, None] + np.zeros(w, np.int64)[None, :], (b + db)[None, :] + np.zeros(w, np.int64)[:, None]
            phi = (t1 if da else t0)[:, None] * (u1 if db else u0)[None, :]          # one multiplication, rounded once
            takes = (na < nr) & (nb < nc) & (phi != 0)         # the corner exists and weighs
            for ia in range(nr):
                for ib in range(nc):
                    cells = takes & (na == ia) & (nb == ib)
                    if not cells.any():
                        continue
                    dn = d[ia, ib]
                    xc = xd[:, cells]                          # (M, cells)
                    t = np.zeros((members, xc.shape[1]), np.float64)
                    exists = np.zeros(members, bool)
                    for k in range(members):                   # the node sums of all columns, old members in increasing order
                        nz = dn[k] != 0                        # a zero of either sign takes no part
                        if not nz.any():
                            continue
                        p = xc[k][None, :] * dn[k, nz].astype(np.float64)[:, None]      # exact: 24 + 24 bits
                        t[nz] = np.where(exists[nz, None], t[nz] + p, p)
                        exists |= nz
                    for m in np.nonzero(exists)[0]:
                        sm, hm = s[m][cells], has[m][cells]
                        first = phi[cells] * t[m]
                        if hm.any():
                            sm[hm] = blend(sm[hm], phi[cells][hm], t[m][hm])
                        sm[~hm] = first[~hm]
                        s[m][cells] = sm
                        has[m][cells] = True
        y = (xd + s).astype(F32)                               # rounded once, then to float
    return np.where(has, y, x)


def define_local(x, d):
    """the definition of fluid_transform_members_local with null taper and box (tests/test_gpu_local.py)"""
    x, d = np.asarray(x, F32), np.asarray(d, F32)
    members = x.shape[0]
    xd = x.astype(np.float64)
    out = x.copy()
    with np.errstate(all="ignore"):
        for m in range(members):
            s = None
            for k in range(members):
                if d[k, m] != 0:
                    p = xd[k] * np.float64(d[k, m])
                    s = p if s is None else s + p
            if s is not None:
                out[m] = (xd[m] + 1.0 * s).astype(F32)
    return out


def stored_mask(d, w, origin, step):
    """(M, W, W) bool: where the definition stores"""
    probe = np.ones((d.shape[2], w, w), F32)
    marked = np.where(np.asarray(d, F32) != 0, F32(1), F32(0))
    return define_lattice(probe, marked, origin, step) != probe


def narrow(y, storage):
    with np.errstate(all="ignore"):
        return y.astype(np.float16).astype(F32) if storage else y


def same(got, want, what):
    """bit for bit, except that a NaN is any NaN"""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, what
    ok = np.where(np.isnan(want), np.isnan(got), got.view(np.uint32) == want.view(np.uint32))
    if not ok.all():
        at = tuple(np.argwhere(~ok)[0])
        raise AssertionError("%s: %d of %d values differ; first at %s: got %r (%08x) want %r (%08x)" % (
            what, int((~ok).sum()), ok.size, at, got[at], got.view(np.uint32)[at], want[at], want.view(np.uint32)[at]))


def same_bits(got, want, what):
    """every bit, NaN payloads included: for memory the call must not have stored"""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d of %d words changed; first at %s" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


# ---- data ------------------------------------------------------------------------------------------------------------------
def mixed_values(rng, shape, storage):
    """magnitudes over many binades, float (fp16 storage: half) denormals, +-0"""
    lo, hi = (-26, 10) if storage else (-149, 60)
    x = np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(lo, hi, shape)) * rng.choice([-1.0, 1.0], shape)
    x = x.astype(F32)
    kind = rng.integers(0, 12, shape)
    x[kind == 0] = 0.0
    x[kind == 1] = -0.0
    x[kind == 2] = F32(2.0 ** -24 if storage else 1e-45) * rng.choice([-1, 1, 3, -5], shape)[kind == 2]       # denormals
    return x


def mixed_increments(rng, nodes, m, zeros=True):
    shape = tuple(nodes) + (m, m)
    d = (np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(-10, 10, shape)) * rng.choice([-1.0, 1.0], shape)).astype(F32)
    if zeros:
        kind = rng.integers(0, 6, shape)
        d[kind == 0] = 0.0
        d[kind == 1] = -0.0
    return d


def small_increments(rng, nodes, m):
    return (rng.uniform(-1.0, 1.0, tuple(nodes) + (m, m)) / np.sqrt(m)).astype(F32)


def shown(s, field):
    """what the pack shows: every member of a field, the lazy state settled"""
    return s.download_members(field)


def apply_and_check(s, field, d, origin, step, storage, what):
    """one call on one field against the definition applied to what the pack showed before; returns (before, after)"""
    before = shown(s, field)
    s.transform_lattice(d, origin, step, fields=(field,))
    after = shown(s, field)
    same(after, narrow(define_lattice(before, d, origin, step), storage), what)
    return before, after


# ---- 0. the definition itself, on the CPU ---------------------------------------------------------------------------------------
def test_the_cases_reach_every_branch_of_rule_2():
    for m in MEMBERS:
        assert len({c[1] for c in cases_of(m)}) >= 2
    for n in (1, 6, 13, 30, 61):
        assert len({c[1] for c in CASES if c[0] == n}) >= 2
    assert {c[2] for c in CASES} == {8, 16, 24} and {c[1] for c in CASES} == {(1, 1), (1, 3), (3, 1), (2, 2), (3, 4)}
    for n, nodes, step, origin in CASES:
        if nodes == (3, 4) and n >= 30:
            for axis in (0, 1):
                a, t0, t1 = axis_weights(n + 2, nodes[axis], origin[axis], step)
                assert (t1[a == 0] == 0).any() and (t1 == 1).any() and ((t1 > 0) & (t1 < 1)).any() and a.max() == nodes[axis] - 2


def cases_of(members):
    """every member count meets every N and every lattice; the three largest counts skip every other case of the middle sizes"""
    if members < 32:
        return CASES
    return [c for k, c in enumerate(CASES) if c[0] in (1, 61) or k % 2 == (members == 64)]


# ---- 1. random increments and values over the shapes -----------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", MEMBERS)
def test_random_increments_and_values(members, storage):
    rng = np.random.default_rng(1000 * storage + members)
    for k, (n, nodes, step, origin) in enumerate(cases_of(members)):
        w = n + 2
        zeros = bool((k + members) % 2)          # with zeros: the tables with masks; without: every term taken
        what = "n=%d M=%d storage=%d nodes %s step %d origin %s zeros=%s" % (n, members, storage, nodes, step, origin, zeros)
        with solver(n, members, storage) as s:
            x = mixed_values(rng, (members, w, w), storage)
            s.upload_members(u=x)
            same(shown(s, "u"), narrow(x, storage), what + ": the upload")
            d = mixed_increments(rng, nodes, members, zeros)
            before, after = apply_and_check(s, "u", d, origin, step, storage, what)
            if nodes == (1, 1):                  # the anchor: fluid_transform_members_local with that D, null taper and box
                with solver(n, members, storage) as twin:
                    twin.upload_members(u=x)
                    twin.transform_local(d[0, 0], fields=("u",))
                    local = shown(twin, "u")
                    ok = ~np.isnan(local)
                    same_bits(after[ok], local[ok], what + ": against transform_local")
                    assert np.isnan(after[~ok]).all()
            # cells on a node: that node's D alone, as the local call defines it
            for ia in range(nodes[0]):
                for ib in range(nodes[1]):
                    i, j = origin[0] + ia * step, origin[1] + ib * step
                    if 0 <= i < w and 0 <= j < w:
                        same(after[:, i, j], narrow(define_local(before[:, i:i + 1, j:j + 1], d[ia, ib]), storage)[:, 0, 0],
                             what + ": the cell on node (%d, %d)" % (ia, ib))


# ---- 2. every patch shape, more than one block ------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("step", [8, 16, 32, 64, 192])
def test_patch_shapes_across_blocks(step, storage):
    """step decides the patch a wave takes (8 x 8, 4 x 16, 2 x 32, 1 x 64 cells); W = 302 is more than one block of four
    patches for each of them, and no multiple of any side; the origin's phase moves the first patch off the array"""
    rng = np.random.default_rng(2000 * storage + step)
    n, members = 300, 5
    w = n + 2
    with solver(n, members, storage) as s:
        for nodes, origin in (((3, 4), (5, -21)), ((2, 2), (-64, 130)), ((1, 1), (w + 9, 3))):
            x = narrow(rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32), storage)
            s.upload_members(dens=x)
            d = small_increments(rng, nodes, members)
            d[rng.integers(0, 3, d.shape) == 0] = 0
            apply_and_check(s, "dens", d, origin, step, storage, "n=%d M=%d storage=%d step %d nodes %s" % (n, members, storage, step, nodes))


# ---- 3. the corner order and the unfused blend are pinned ------------------------------------------------------------------------
def test_the_corner_order_and_the_unfused_blend():
    """Float rounding hides most double-level differences.  D00 = base * 2^30 and D11 = -D00 make the first and last
    corners' products large and nearly cancelling, D01 and D10 stay small: blended in another order, or with the product
    fused into the sum, some cells round differently -- shown on the CPU first, for this very data."""
    rng = np.random.default_rng(3)
    n, members, step, origin = 52, 3, 24, (3, 3)
    w = n + 2
    x = rng.standard_normal((members, w, w)).astype(F32)
    base = rng.uniform(-1.0, 1.0, (members, members)).astype(F32)
    d = np.zeros((2, 2, members, members), F32)
    d[0, 0] = base * F32(2.0 ** 30)
    d[1, 1] = -d[0, 0]
    d[0, 1] = base
    d[1, 0] = F32(0.75) * base
    want = define_lattice(x, d, origin, step)
    four = np.zeros((w, w), bool)
    four[origin[0] + 1:origin[0] + step, origin[1] + 1:origin[1] + step] = True        # strictly inside the lattice cell
    assert four.sum() * members == 1587
    other_order = define_lattice(x, d, origin, step, corners=(0, 3, 1, 2))
    fused = define_lattice(x, d, origin, step, blend=fused_blend)
    n_order = int((other_order.view(np.uint32) != want.view(np.uint32))[:, four].sum())
    n_fused = int((fused.view(np.uint32) != want.view(np.uint32))[:, four].sum())
    print("corner order (00, 11, 01, 10) differs in %d, a fused blend in %d of %d values" % (n_order, n_fused, four.sum() * members))
    assert n_order >= 1 and n_fused >= 1
    with solver(n, members) as s:
        s.upload_members(u=x)
        s.transform_lattice(d, origin, step, fields=("u",))
        same(shown(s, "u"), want, "the contract's order, unfused")


# ---- 4. zero weights and poison ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", [3, 9, 64])
def test_a_zero_weight_keeps_poison_out(members, storage):
    rng = np.random.default_rng(4000 * storage + members)
    n, nodes, step, origin = 30, (2, 2), 16, (8, 8)
    w = n + 2
    bad = members - 2
    hit = [m for m in range(members) if m % 2 == 0 and m != bad]       # the new members whose column names the bad one
    a, t0, _ = axis_weights(w, 2, origin[0], step)
    phi00 = t0[:, None] * t0[None, :]
    assert (phi00 == 0).any() and (phi00 != 0).any()
    for poison in (np.nan, np.inf):
        x = narrow(rng.uniform(0.5, 2.0, (members, w, w)).astype(F32), storage)
        x[bad] = poison
        d = rng.uniform(0.25, 1.0, nodes + (members, members)).astype(F32)
        d[:, :, :, bad] = 0                                            # the bad member itself is stored nowhere
        d[:, :, bad, :] = rng.choice([0.0, -0.0], nodes + (members,))
        d[0, 0, bad, hit] = 1.5                                        # ... and named at node (0, 0) only
        with solver(n, members, storage) as s:
            s.upload_members(u=x)
            before, after = apply_and_check(s, "u", d, origin, step, storage, "M=%d storage=%d poison %s" % (members, storage, poison))
            same_bits(after[bad], before[bad], "the bad member")
            good = [m for m in range(members) if m != bad]
            assert np.isfinite(after[good][:, phi00 == 0]).all(), "poison under a zero weight"
            assert not np.isfinite(after[hit][:, phi00 != 0]).any()
            clean = [m for m in good if m not in hit]
            assert np.isfinite(after[clean]).all()
            # zero increments everywhere for the bad member: it poisons nobody
            d[0, 0, bad, :] = 0
            s.upload_members(u=x)
            before, after = apply_and_check(s, "u", d, origin, step, storage, "M=%d storage=%d poison %s unnamed" % (members, storage, poison))
            assert np.isfinite(after[good]).all()
            same_bits(after[bad], before[bad], "the bad member")


# ---- 5. not stored means not stored ---------------------------------------------------------------------------------------------
def arena_ensemble(n, members, storage):
    import torch
    from fluidsimulationcuda_amd import capi
    nbytes = capi.lib().fluid_arena_bytes_ensemble(n, storage, members)
    arena = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return solver(n, members, storage, arena_ptr=arena.data_ptr(), arena_bytes=nbytes), arena


def arena_rows(s, arena):
    """the arena as (12 x members, N+2, pitch) stored elements, and the offset of column 0"""
    import torch
    from fluidsimulationcuda_amd import capi
    pitch, xoff, ff = C.c_int(), C.c_int(), C.c_size_t()
    assert capi.lib().fluid_layout(s.n, C.byref(pitch), C.byref(xoff), C.byref(ff)) == 0
    s.synchronize()
    torch.cuda.synchronize()
    dtype = np.uint16 if s.storage else np.uint32
    raw = arena.cpu().numpy()[:12 * s.members * ff.value * dtype().itemsize].view(dtype)
    return raw.reshape(12 * s.members, s.n + 2, pitch.value), xoff.value


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", [3, 9, 33])
def test_members_without_a_term_pads_and_other_fields(members, storage):
    from fluidsimulationcuda_amd import capi
    rng = np.random.default_rng(5000 * storage + members)
    for n, nodes, step, origin in ((13, (2, 2), 8, (3, 4)), (61, (3, 4), 16, (7, -5)), (6, (1, 3), 8, (9, 1))):
        w = n + 2
        idle = [1, members - 1]                                        # no term in any node
        d = mixed_increments(rng, nodes, members)
        d[:, :, :, idle] = rng.choice([0.0, -0.0], nodes + (members, 2))
        d[:, :, idle, :] = rng.choice([0.0, -0.0], nodes + (2, members))          # ... and named by nobody: their NaNs stay theirs
        s, arena = arena_ensemble(n, members, storage)
        with s:
            fields = {}
            for name in capi.FIELD_NAMES:
                x = narrow(mixed_values(rng, (members, w, w), storage), storage)
                x[x == 0] = 1.5                                        # no zero word anywhere: a pad written would show
                if not storage:
                    x[idle[0]].view(np.uint32)[::2, ::3] = 0x7fc12345  # NaNs with a payload, and a negative one
                    x[idle[1]].view(np.uint32)[1::2, ::2] = 0xffc00abc
                fields[name] = x
                s.upload_members(**{name: x})
            stored, xoff = arena_rows(s, arena)
            stored = stored.copy()
            before = shown(s, "v")
            s.transform_lattice(d, origin, step, fields=("v",))
            after = shown(s, "v")
            what = "n=%d M=%d storage=%d" % (n, members, storage)
            same(after, narrow(define_lattice(before, d, origin, step), storage), what)
            same_bits(after[idle], before[idle], what + ": members without a term")
            raw, _ = arena_rows(s, arena)
            assert not raw[:, :, :xoff].any() and not raw[:, :, xoff + w:].any(), what + ": pad columns were written"
            v = capi.FIELD_NAMES.index("v")
            others = np.ones(12 * members, bool)
            others[v * members:(v + 1) * members] = False
            assert np.array_equal(raw[others], stored[others]), what + ": another field changed"
            assert np.array_equal(raw[v * members:(v + 1) * members][idle], stored[v * members:(v + 1) * members][idle]), what + ": an idle member's words"


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_zero_increments_launch_nothing_and_settle_the_field(storage):
    rng = np.random.default_rng(5500 + storage)
    n, members = 13, 5
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    fields["u"][2] = np.nan
    with solver(n, members, storage) as a, solver(n, members, storage) as b:
        for s in (a, b):
            s.upload_members(**fields)
            s.step(use_sources=True)
            s.add_source("dens", "dens_prev", DT)                      # dens owes itself an increment
        a.transform_lattice(rng.choice([0.0, -0.0], (3, 4, members, members)), (2, 1), 8, fields=("dens", "u", "u_prev"))
        for name in MAIN:
            same(shown(a, name), shown(b, name), "storage=%d: %s after increments of zeros" % (storage, name))
        for s in (a, b):
            s.step(use_sources=not storage)
        for name in ("v", "dens"):
            same(shown(a, name), shown(b, name), "storage=%d: %s a step later" % (storage, name))


# ---- 6. lazy state, scaled fp16 fields ----------------------------------------------------------------------------------------
def prepared(n, members, storage, fields, case):
    """a context in one of the lazy states, and the fields the call is made on"""
    s = solver(n, members, storage)
    if case == "fill":
        s.upload_members(**fields)
        s.fill("dens", 0.375)
        s.fill("u_prev", 0.0)
        return s, ("dens", "u_prev")
    s.upload_members(**fields)
    s.step(use_sources=True)                  # fp16 storage: u_prev and v_prev now hold the pressure and the divergence scaled
    if case == "step":
        return s, MAIN
    s.computeDivergenceAndPressure("u", "v", "dens_prev", "tmp0")       # its pressure is zero by definition: marked, not written
    s.add_source("dens", "dens_prev", DT)     # ... and adding such a source is deferred: dens owes itself an increment
    return s, ("dens", "dens_prev")


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("case", ["fill", "step", "pending"])
@pytest.mark.parametrize("members", [2, 5, 33])
def test_lazy_state_is_settled_first(members, storage, case):
    """The call against the definition applied to what a twin context shows (the pack settles what the field owes itself
    and divides a scale back): stored cells hold narrow(y), every other cell shows exactly what it showed -- in an fp16
    field held at a scale too (u_prev and v_prev after a step), where that need not be a half."""
    rng = np.random.default_rng(6000 * storage + members)
    for n, nodes, step, origin in ((13, (2, 2), 8, (3, 4)), (30, (3, 4), 8, (4, 2))):
        w = n + 2
        fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
        d = small_increments(rng, nodes, members)
        d[:, :, :, members - 1] = 0                                    # one member is stored nowhere
        d[0, 0, 0, 0] = 0
        what = "n=%d M=%d storage=%d %s" % (n, members, storage, case)
        a, names = prepared(n, members, storage, fields, case)
        b, _ = prepared(n, members, storage, fields, case)
        with a, b:
            a.transform_lattice(d, origin, step, fields=names)
            state = {name: shown(a, name) for name in MAIN}
            for name in MAIN:
                before = shown(b, name)                                # the twin: the call never ran there
                want = before
                if name in names:
                    want = np.where(stored_mask(d, w, origin, step), narrow(define_lattice(before, d, origin, step), storage), before)
                    if storage and case == "step" and name == "u_prev":
                        print("%s: %d of %d values of the scaled u_prev shown before the call are no halves" % (
                            what, int((narrow(before, 1) != before).sum()), before.size))
                same(state[name], want, "%s: %s against the definition on what the twin shows" % (what, name))
                if name not in names:
                    same_bits(state[name], before, "%s: %s was not listed" % (what, name))
            # one more step: the record of every field is right again.  fp16 storage: without sources, so that the step reads
            # no *_prev field -- a fresh context cannot be given the scaled ones bit for bit (an upload rounds to halves)
            with solver(n, members, storage) as fresh:
                fresh.upload_members(**state)
                for s in (a, fresh):
                    s.step(use_sources=not storage)
                for name in ("u", "v", "dens"):
                    same(shown(a, name), shown(fresh, name), "%s: %s a step later, against a fresh context" % (what, name))


# ---- 7. repeated calls -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_successive_calls_need_no_wait_and_repeat(storage):
    rng = np.random.default_rng(7000 + storage)
    n, members = 61, 9
    w = n + 2
    x = narrow(rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32), storage)
    first = ((3, 4), 16, (7, 5), small_increments(rng, (3, 4), members))
    second = ((2, 2), 24, (-4, 30), small_increments(rng, (2, 2), members))          # a smaller table in the same buffer
    third = ((4, 4), 8, (1, 1), small_increments(rng, (4, 4), members))              # ... and a larger one: the buffer grows
    with solver(n, members, storage) as s, solver(n, members, storage) as twin:
        for c in (s, twin):
            c.upload_members(u=x, v=x)
        want = x
        for nodes, step, origin, d in (first, second, third):
            s.transform_lattice(d, origin, step, fields=("u", "v"))                   # no wait, no download in between
            want = narrow(define_lattice(want, d, origin, step), storage)
        got = shown(s, "u")
        same(got, want, "storage=%d: three calls back to back" % storage)
        same_bits(shown(s, "v"), got, "storage=%d: two fields of equal data" % storage)
        for nodes, step, origin, d in (first, second, third):
            twin.transform_lattice(d, origin, step, fields=("u",))
        same_bits(shown(twin, "u"), got, "storage=%d: identical calls on equal data" % storage)


# ---- 8. refusals on a live context ----------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(8)
    n, members = 6, 5
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    name = b"fluid_transform_members_lattice"

    def ints(*v):
        return (C.c_int * len(v))(*v)

    def lattice(hnd, ids, d, count=None, nodes=None, origin=(1, 2), step=8):
        d = np.ascontiguousarray(d, F32)
        nr, nc = d.shape[:2] if nodes is None else nodes
        return lambda: L.fluid_transform_members_lattice(hnd, ids, len(ids) if count is None else count, d.ctypes.data_as(capi._MF), nr, nc,
                                                         origin[0], origin[1], step)

    good, ids = small_increments(rng, (2, 3), members), ints(0, 1, 2)
    with solver(n, members) as s, solver(n, members) as twin:
        for c in (s, twin):
            c.timing_enable(True)
            c.upload_members(**fields)
            c.step(use_sources=True)
            c.add_source("dens", "dens_prev", DT)                      # a lazy state that must survive the refusals
        hnd = s._h
        nan_d, inf_d = good.copy(), good.copy()
        nan_d[1, 2, 3, 1] = np.nan
        inf_d[0, 1, 0, 4] = -np.inf
        one = np.zeros(1, F32)
        refused = [
            (lambda: L.fluid_transform_members_lattice(hnd, None, 1, good.ctypes.data_as(capi._MF), 2, 3, 0, 0, 8), (b"fields",)),
            (lambda: L.fluid_transform_members_lattice(hnd, ids, 3, None, 2, 3, 0, 0, 8), (b"increments",)),
            (lattice(None, ids, good), (b"null context",)),
            (lattice(hnd, ids, good, 0), (b"nfields 0",)),
            (lattice(hnd, ids, good, 13), (b"nfields 13",)),
            (lattice(hnd, ids, good, -1), (b"nfields -1",)),
            (lattice(hnd, ints(0, 12), good), (b"bad field id 12", b"fields[1]")),
            (lattice(hnd, ints(-1, 2), good), (b"bad field id -1", b"fields[0]")),
            (lattice(hnd, ints(2, 1, 2), good), (b"field 2", b"twice", b"fields[0]", b"fields[2]")),
            (lattice(hnd, ids, good, nodes=(0, 3)), (b"nodes_row = 0",)),
            (lattice(hnd, ids, good, nodes=(2, -1)), (b"nodes_col = -1",)),
            (lattice(hnd, ids, one, nodes=(64, 65)), (b"4160", b"FLUID_LATTICE_MAX_NODES", b"4096")),
            (lattice(hnd, ids, one, nodes=(1 << 20, 1 << 20)), (b"FLUID_LATTICE_MAX_NODES", b"4096")),
            (lattice(hnd, ids, good, step=0), (b"step = 0", b"multiple of 8")),
            (lattice(hnd, ids, good, step=-8), (b"step = -8", b"multiple of 8")),
            (lattice(hnd, ids, good, step=4), (b"step = 4", b"multiple of 8")),
            (lattice(hnd, ids, good, step=12), (b"step = 12", b"multiple of 8")),
            (lattice(hnd, ids, nan_d), (b"not finite", b"a = 1", b"b = 2", b"k = 3", b"m = 1")),
            (lattice(hnd, ids, inf_d), (b"not finite", b"a = 0", b"b = 1", b"k = 0", b"m = 4")),
        ]
        for call, words in refused:
            L.fluid_synchronize(None)                   # (an unrelated message in between)
            assert call() == capi.E_INVALID, words
            msg = L.fluid_last_error()
            assert name in msg and all(word in msg for word in words), (words, msg)
        s.synchronize()
        ta, tb = s.timing_read(reset=False), twin.timing_read(reset=False)
        assert ta == {**tb, **{k: ta[k] for k in ta if k.endswith("_ms")}}             # every count; the times are times
        for f in capi.FIELD_NAMES:                      # every field of every member, and what they still owe themselves
            same_bits(shown(s, f), shown(twin, f), "%s after the refusals" % f)
        # what is not refused: the extremes of the origin, and the call belongs to no timing category
        assert lattice(hnd, ids, good, origin=(-2 ** 31, 2 ** 31 - 1), step=2 ** 31 - 8)() == capi.OK
        twin.transform_lattice(good, (-2 ** 31, 2 ** 31 - 1), 2 ** 31 - 8)
        ta, tb = s.timing_read(reset=False), twin.timing_read(reset=False)
        assert ta == {**tb, **{k: ta[k] for k in ta if k.endswith("_ms")}}
        for c in (s, twin):
            c.step(use_sources=True)
        for f in ("u", "v", "dens"):
            same(shown(s, f), shown(twin, f), "%s a step after the refusals" % f)
    # the cap: one member too many
    big = capi.TRANSFORM_MAX_MEMBERS + 1
    with solver(1, big) as s:
        x = rng.uniform(-1.0, 1.0, (big, 3, 3)).astype(F32)
        s.upload_members(u=x)
        assert lattice(s._h, ints(0), np.ones((1, 1, big, big), F32))() == capi.E_INVALID
        msg = L.fluid_last_error()
        assert name in msg and b"65" in msg and b"64" in msg, msg
        same_bits(shown(s, "u"), x, "u after the refused call of 65 members")
    # row slabs
    with F().FluidSolver(n, rank=0, nranks=2) as s:
        assert lattice(s._h, ints(0), np.ones((1, 1, 1, 1), F32))() == capi.E_INVALID
        msg = L.fluid_last_error()
        assert name in msg and b"slab" in msg, msg


def test_the_extreme_origin_against_the_definition():
    """row0 = -2^31 with the largest step: q and (n - 1) * step need 64 bits"""
    rng = np.random.default_rng(81)
    n, members = 13, 3
    w = n + 2
    step = 2 ** 31 - 8
    with solver(n, members) as s:
        for origin in ((-2 ** 31, 2 ** 31 - 1), (-step + 5, -step - 2), (3, -step)):
            s.upload_members(u=rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32))
            apply_and_check(s, "u", small_increments(rng, (3, 3), members), origin, step, 0, "origin %s" % (origin,))
