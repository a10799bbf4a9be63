"""GPU: the ensemble Gram matrix -- fluid_member_gram (include/fluid_amd.h, "ensemble diagnostics"): the M x M matrix of
inner products between the members of a field over the interior cells, or between their anomalies about the per-cell mean.

Every expected value comes from `define` below, the header's definition in numpy -- the member-order mean chain, the
subtraction, float64 products -- applied to what download_members (the pack) showed before the call.  On dyadic data every
partial sum is representable and the result is compared with `==` (bit for bit where two results of the library are
compared); on general data against the textbook bound of a recursive double sum in any order, gamma = (n + 2) u /
(1 - (n + 2) u) times the sum of the |products|, n = N^2, u = 2^-53 (the + 2: the reference's own rounded products and final
rounding) -- derived, not measured."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZES = [1, 6, 13, 30, 61, 254]             # rows shorter and longer than a wave, W % 4 != 0; 254: more than one block and
                                            # more than one partial per fold lane
MEMBERS = [1, 2, 3, 5, 8, 9, 17, 32, 33, 64]   # every padded count and the counts just past one
COARSE = np.array([-1, -0.5, -0.25, 0.0, -0.0, 0.25, 0.5, 1], F32)       # as in tests/test_gpu_lazy_state.py
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
def operands(xd, centre):
    """xd: (M, ...) float64, the widened values of some cells.  a_k of the header."""
    with np.errstate(all="ignore"):
        if centre:
            s = xd[0].copy()
            for m in range(1, xd.shape[0]):               # member order
                s = s + xd[m]
            xd = xd - s / np.float64(xd.shape[0])         # one rounding
    return xd


def define(x, centre):
    """x: (M, W, W) float32, what the pack shows before the call.  The operands a_k over the interior cells, (M, N*N) float64."""
    xd = np.asarray(x, F32).astype(np.float64)[:, 1:-1, 1:-1]
    return operands(xd, centre).reshape(xd.shape[0], -1)


def fsum_gram(a, absolute=False):
    """G[k, m] = fsum of the float64 products a_k * a_m (of their magnitudes with `absolute`): correctly rounded sums"""
    m = a.shape[0]
    g = np.empty((m, m), np.float64)
    for k in range(m):
        for j in range(k, m):
            p = a[k] * a[j]
            g[k, j] = g[j, k] = math.fsum(np.abs(p) if absolute else p)
    return g


def exact_gram(a, bits):
    """the exact sum for operands that are multiples of 2^-bits: integer arithmetic; a sample of entries is held against
    math.fsum of the exact products, which is what every entry is at the smaller sizes"""
    m, cells = a.shape
    if cells <= 61 * 61:
        return fsum_gram(a)
    i = np.ldexp(a, bits)
    assert (i == np.rint(i)).all() and np.abs(i).max() < 2 ** 20
    i = i.astype(np.int64)
    g = np.ldexp((i @ i.T).astype(np.float64), -2 * bits)       # |sums| < 2^53: exact
    for k, j in {(0, 0), (0, m - 1), (m - 1, m - 1), (m // 2, m // 3)}:
        assert g[k, j] == math.fsum(a[k] * a[j])
    return g


def gamma(n):
    return (n * n + 2) * U / (1 - (n * n + 2) * U)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, what
    ok = np.where(np.isnan(want), np.isnan(got), got.view(np.uint64) == want.view(np.uint64))
    if not ok.all():
        at = tuple(np.argwhere(~ok)[0])
        raise AssertionError("%s: %d of %d entries differ; first at %s: got %r want %r" % (what, int((~ok).sum()), ok.size, at, got[at], want[at]))


def equal(got, want, what):
    """`==`, entry by entry: the exact sum.  (The sign of a sum that is zero is IEEE addition's in the kernel's order and is
    not compared: math.fsum gives +0 for a single product of -0.)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(want).all(), what
    ok = got == want
    if not ok.all():
        at = tuple(np.argwhere(~ok)[0])
        raise AssertionError("%s: %d of %d entries differ; first at %s: got %r want %r" % (what, int((~ok).sum()), ok.size, at, got[at], want[at]))


def symmetric(g, what):
    assert np.array_equal(g.view(np.uint64), g.T.view(np.uint64)), "%s: not bit-symmetric" % what


def within_bound(got, a, n, what):
    want, mag = fsum_gram(a), fsum_gram(a, absolute=True)
    bound = gamma(n) * mag
    err = np.abs(got - want)
    ratio = float((err / bound).max())
    print("%s: largest error / bound = %.4f" % (what, ratio))
    assert (err <= bound).all(), "%s: %d entries outside the summation bound (largest ratio %.3g)" % (what, int((err > bound).sum()), ratio)


# ---- 1. exact on dyadic data ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", MEMBERS)
def test_exact_on_dyadic_data(members, storage):
    rng = np.random.default_rng(1000 * storage + members)
    for n in SIZES:
        w = n + 2
        with solver(n, members, storage) as s:
            x = rng.choice(COARSE, size=(members, w, w)).astype(F32)
            s.upload_members(dens=x)
            before = s.download_members("dens")
            assert np.array_equal(before.view(np.uint32), x.view(np.uint32))
            for centre in (False, True):
                if centre and members not in (1, 2, 8, 64):       # a power of two: mean, anomalies and products are exact
                    continue
                what = "n=%d M=%d storage=%d centre=%s" % (n, members, storage, centre)
                got = s.member_gram("dens", centre=centre)
                equal(got, exact_gram(define(before, centre), 8 if centre else 2), what)
                symmetric(got, what)
            assert np.array_equal(s.download_members("dens").view(np.uint32), x.view(np.uint32)), "the call changed the field"


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_zero_fields_give_plus_zero(storage):
    for members in (1, 5, 64):
        for n in (1, 30):
            with solver(n, members, storage) as s:
                for centre in (False, True):
                    g = s.member_gram("tmp3", centre=centre)        # untouched: lazily zero
                    assert not g.view(np.uint64).any(), "an untouched field: M=%d n=%d centre=%s" % (members, n, centre)
                s.upload_members(v=np.full((members, n + 2, n + 2), -0.0, F32))
                for centre in (False, True):
                    g = s.member_gram("v", centre=centre)
                    assert not g.view(np.uint64).any(), "a field of -0: M=%d n=%d centre=%s" % (members, n, centre)


# ---- 2. a small spread on a large mean -----------------------------------------------------------------------------------------
def test_small_spread_on_a_large_mean():
    members = 8
    rng = np.random.default_rng(2)
    for n in (30, 61):
        w = n + 2
        d = rng.integers(-7, 8, (members, w, w))
        x = (4096.0 + d * 2.0 ** -10).astype(F32)
        assert np.array_equal(x.astype(np.float64), 4096.0 + d * 2.0 ** -10)
        with solver(n, members) as s:
            s.upload_members(u=x)
            a = define(s.download_members("u"), True)               # multiples of 2^-13, |a| < 2^-6: the products are exact
            want = fsum_gram(a)
            assert want.any() and np.abs(want).max() < 1.0
            # what the raw identity would need: the sum of x_k x_m itself takes more than 53 bits
            assert 2 * 23 + math.log2(n * n) > 53
            got = s.member_gram("u", centre=True)
            equal(got, want, "n=%d: the centred Gram of 4096 + d 2^-10" % n)
            symmetric(got, "n=%d" % n)


# ---- 3. general data within the summation bound ------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n,members", [(61, 5), (30, 9), (254, 3), (13, 33), (30, 64), (30, 32), (61, 17)])
def test_general_data_within_the_summation_bound(n, members, storage):
    rng = np.random.default_rng(3000 * storage + 10 * n + members)
    w = n + 2
    with solver(n, members, storage) as s:
        for scale in (1e-3, 1.0, 1e3):
            for centre in (False, True):
                x = rng.uniform(0.25, 1.0, (members, w, w)) * rng.choice([-1.0, 1.0], (members, w, w)) * scale
                if centre:
                    x = x + 50 * scale
                s.upload_members(v=x.astype(F32))
                before = s.download_members("v")
                assert np.isfinite(before).all()
                what = "n=%d M=%d storage=%d scale=%g centre=%s" % (n, members, storage, scale, centre)
                got = s.member_gram("v", centre=centre)
                within_bound(got, define(before, centre), n, what)
                symmetric(got, what)


# ---- 4. determinism --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n,members", [(61, 33), (254, 64), (254, 5), (30, 32), (61, 17)])
def test_the_same_bits_every_time(n, members, storage):
    rng = np.random.default_rng(4000 * storage + n + members)
    w = n + 2
    x = rng.normal(size=(members, w, w)).astype(F32)
    with solver(n, members, storage) as a, solver(n, members, storage) as b:
        a.upload_members(u=x)
        b.upload_members(u=x)
        for centre in (False, True):
            what = "n=%d M=%d storage=%d centre=%s" % (n, members, storage, centre)
            first = a.member_gram("u", centre=centre)
            same_bits(a.member_gram("u", centre=centre), first, what + ": two calls in a row")
            same_bits(b.member_gram("u", centre=centre), first, what + ": a second context")
            symmetric(first, what)


# ---- 5. lazy state and fp16 ------------------------------------------------------------------------------------------------------
def prepared(n, members, storage, fields, case):
    """a context in one of the lazy states, and the field the state is about"""
    s = solver(n, members, storage)
    s.timing_enable(True)
    s.upload_members(**fields)
    s.step(use_sources=True)
    if case == "scaled":                   # fp16 storage: the pressure of a step (u_prev) is held scaled
        return s, "u_prev"
    s.computeDivergenceAndPressure("u", "v", "dens_prev", "tmp0")       # dens_prev: zero by definition, marked, not written
    s.add_source("dens", "dens_prev", DT)  # ... and adding such a source is deferred: dens owes itself an increment
    return s, "dens"


@pytest.mark.parametrize("storage,case", [(0, "scaled"), (0, "pending"), (1, "scaled"), (1, "pending")])
@pytest.mark.parametrize("members", [3, 33])
def test_lazy_state_is_settled_and_nothing_is_altered(members, storage, case):
    rng = np.random.default_rng(5000 * storage + members)
    n = 30
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    a, f = prepared(n, members, storage, fields, case)
    b, _ = prepared(n, members, storage, fields, case)
    with a, b:
        grams = {centre: a.member_gram(f, centre=centre) for centre in (False, True)}
        shown = a.download_members(f)
        assert np.abs(shown[:, 1:-1, 1:-1]).max() > 0
        for centre, got in grams.items():
            what = "M=%d storage=%d %s centre=%s" % (members, storage, case, centre)
            within_bound(got, define(shown, centre), n, what)
            symmetric(got, what)
        from fluidsimulationcuda_amd import capi
        for name in capi.FIELD_NAMES:          # every field of every member, against the twin that never made the call
            assert np.array_equal(a.download_members(name).view(np.uint32), b.download_members(name).view(np.uint32)), name
        ta, tb = a.timing_read(reset=False), b.timing_read(reset=False)
        assert {k: ta[k] for k in COUNTS} == {k: tb[k] for k in COUNTS}
        for s in (a, b):
            s.step(use_sources=True)
        for name in ("u", "v", "dens"):
            assert np.array_equal(a.download_members(name).view(np.uint32), b.download_members(name).view(np.uint32)), name + " a step later"
        ta, tb = a.timing_read(reset=False), b.timing_read(reset=False)
        assert {k: ta[k] for k in COUNTS} == {k: tb[k] for k in COUNTS}


# ---- 6. NaN containment ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_nan_containment(storage):
    members, n, bad = 5, 61, 2
    rng = np.random.default_rng(6 + storage)
    w = n + 2
    x = rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32)
    with solver(n, members, storage) as s:
        s.upload_members(u=x)
        clean = s.member_gram("u")
        assert np.isfinite(clean).all() and np.isfinite(s.member_gram("u", centre=True)).all()
        x[bad, 17, 40] = np.nan
        s.upload_members(u=x)
        got = s.member_gram("u")
        assert np.isnan(got[bad]).all() and np.isnan(got[:, bad]).all()
        keep = np.ones((members, members), bool)
        keep[bad] = keep[:, bad] = False
        assert np.array_equal(got.view(np.uint64)[keep], clean.view(np.uint64)[keep]), "a NaN in member 2 changed another entry"
        assert np.isnan(s.member_gram("u", centre=True)).all()
        # a NaN in the ghost ring takes no part
        x[bad, 17, 40] = 0.25
        s.upload_members(u=x)
        inner = s.member_gram("u")
        x[bad, 0, 5] = x[bad, 9, w - 1] = np.nan
        s.upload_members(u=x)
        same_bits(s.member_gram("u"), inner, "a NaN in the ghost ring")


# ---- 7. refusals with a live context ----------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(7)
    n, members = 6, 5
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    out = np.full((members, members), 7.0)
    dp = C.POINTER(C.c_double)
    with solver(n, members) as s, solver(n, members) as twin:
        for c in (s, twin):
            c.timing_enable(True)
            c.upload_members(**fields)
            c.step(use_sources=True)
            c.add_source("dens", "dens_prev", DT)                      # a lazy state that must survive the refusals
        for field, words in ((12, (b"bad field id 12",)), (-1, (b"bad field id -1",))):
            L.fluid_synchronize(None)                                  # (an unrelated message in between)
            assert L.fluid_member_gram(s._h, field, 1, out.ctypes.data_as(dp)) == capi.E_INVALID
            msg = L.fluid_last_error()
            assert b"fluid_member_gram" in msg and all(word in msg for word in words), msg
        assert L.fluid_member_gram(s._h, 0, 0, None) == capi.E_INVALID
        assert b"fluid_member_gram" in L.fluid_last_error() and b"gram" in L.fluid_last_error()
        assert (out == 7.0).all()
        ta, tb = s.timing_read(reset=False), twin.timing_read(reset=False)
        assert ta == {**tb, **{k: ta[k] for k in ta if k.endswith("_ms")}}             # every count; the times are times
        for f in capi.FIELD_NAMES:
            assert np.array_equal(s.download_members(f).view(np.uint32), twin.download_members(f).view(np.uint32)), f
        for c in (s, twin):
            c.step(use_sources=True)
        for f in ("u", "v", "dens"):
            assert np.array_equal(s.download_members(f).view(np.uint32), twin.download_members(f).view(np.uint32)), f
    # the cap: one member too many
    big = capi.TRANSFORM_MAX_MEMBERS + 1
    with solver(2, big) as s:
        x = rng.uniform(-1.0, 1.0, (big, 4, 4)).astype(F32)
        s.upload_members(u=x)
        g = np.full((big, big), 7.0)
        for centre in (0, 1):
            assert L.fluid_member_gram(s._h, 0, centre, g.ctypes.data_as(dp)) == capi.E_INVALID
            msg = L.fluid_last_error()
            assert b"fluid_member_gram" in msg and b"65" in msg and b"64" in msg, msg
        assert (g == 7.0).all()
        assert np.array_equal(s.download_members("u"), x)
    # row slabs
    with F().FluidSolver(n, rank=0, nranks=2) as s:
        one = np.full((1, 1), 7.0)
        assert L.fluid_member_gram(s._h, 0, 0, one.ctypes.data_as(dp)) == capi.E_INVALID
        msg = L.fluid_last_error()
        assert b"fluid_member_gram" in msg and b"slab" in msg, msg
        assert one[0, 0] == 7.0


# ---- 8. closes the loop ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_inflation_through_the_transform_scales_the_gram(storage):
    members, n, lam = 8, 30, 2.0
    rng = np.random.default_rng(8 + storage)
    w = n + 2
    x = rng.choice(COARSE, size=(members, w, w)).astype(F32)
    with solver(n, members, storage) as s:
        s.upload_members(dens=x)
        g = s.member_gram("dens", centre=True)
        assert g.any()
        equal(g, fsum_gram(define(x, True)), "the centred Gram before")
        eye = np.eye(members)
        t = eye + (lam - 1.0) * (eye - np.ones((members, members)) / members)      # inflates the spread by lam; dyadic weights
        s.transform(t, fields=("dens",))
        y = s.download_members("dens")
        mean = x.astype(np.float64).mean(axis=0)
        assert np.array_equal(y.astype(np.float64), mean + lam * (x - mean))        # the mean kept, the anomalies doubled
        equal(s.member_gram("dens", centre=True), lam * lam * g, "the centred Gram after inflation by %g" % lam)


# ---- 9. member 63 at least 2^32 bytes behind member 0 ------------------------------------------------------------------------------
def test_members_past_4_gib():
    """Member and row bases are 64-bit arithmetic in the kernel and it takes no index-width template: this is the one place
    where they can go wrong -- the smallest N whose 64th fp32 member starts 2^32 bytes or more behind the first.  Every
    member holds one constant but for a few cells of members 31 and 63, all dyadic: the expected matrix is exact and needs
    no pass over the field on the host."""
    import torch
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    members = 64

    def field_floats(n):
        pitch, xoff, ff = C.c_int(), C.c_int(), C.c_size_t()
        assert L.fluid_layout(n, C.byref(pitch), C.byref(xoff), C.byref(ff)) == 0
        return ff.value

    n = next(n for n in range(3900, 4200) if (members - 1) * field_floats(n) * 4 >= 1 << 32)
    w = n + 2
    arena = L.fluid_arena_bytes_ensemble(n, 0, members)
    free, total = torch.cuda.mem_get_info()
    if free < arena + (1 << 30):
        pytest.skip("n=%d, M=64 needs an arena of %.1f GB, %.1f GB of %.1f GB are free" % (n, arena / 1e9, free / 1e9, total / 1e9))
    rng = np.random.default_rng(9)
    cells = [(1, 1), (1, n), (n, 1), (n, n), (n // 2, 257), (7, n - 64), (n - 3, 64), (2049, 2048)]       # (row, column), interior
    table = np.full((members, 1 + len(cells)), 0.5)                  # column 0: every other cell; then the marked cells
    table[31, 0], table[63, 0] = -1.0, 0.25
    for m in (31, 63):
        table[m, 1:] = rng.choice(COARSE, len(cells))
    with solver(n, members) as s:
        s.fill("u", 0.5)
        for m in (31, 63):
            a = np.full((w, w), table[m, 0], F32)
            for c, (i, j) in enumerate(cells):
                a[i, j] = table[m, 1 + c]
            a[0, :] = a[:, 0] = a[w - 1, :] = a[:, w - 1] = 3.0      # the ghost ring takes no part
            s.upload(member=m, u=a)
        weight = np.array([n * n - len(cells)] + [1] * len(cells), np.float64)
        for centre in (False, True):
            a = operands(table, centre)                              # multiples of 2^-8; every sum below is exact
            want = (a * weight) @ a.T
            got = s.member_gram("u", centre=centre)
            equal(got, want, "n=%d M=64 centre=%s" % (n, centre))
            symmetric(got, "n=%d" % n)
