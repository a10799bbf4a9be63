"""GPU: ensemble products -- fluid_member_quantiles and fluid_member_exceedance (include/fluid_amd.h, "ensemble products"): per
cell of the W x W array the order statistics across the members, interpolated at up to 16 levels, and the fraction of members
above or below up to 16 thresholds.

Every expected value comes from tests/quantile_model.py, the header's rules in numpy float64, applied to what download_members
(the pack) showed before the call, and is compared exactly (a NaN is any NaN).  tests/test_quantile_abi.py shows on the CPU
what the model itself has to have.

The kernels' own indexing (fluid_quantile.hip): one lane per cell, no cap on the grid -- lane t of block t / 256 takes cell
t = row * W + col and no other, so there is no wrap of the grid to test.  The seams: the end of a row (t = k * W - 1 | k * W),
the end of a wave (t = 63 | 64) and the end of a block (t = 255 | 256).  The member count picks one of six quantile kernels,
padded to MP = 2, 4, 8, 16, 32, 64 members; the exceedance kernel walks the members four at a time, then one at a time.

Shapes: N = 14 is one partial block, N = 30 four blocks exactly (W = 32: a row seam at every wave seam), N = 61 has W = 63, odd
and no multiple of 4, N = 66 is where fp16 storage holds the pressure at a scale."""
import ctypes as C

import numpy as np
import pytest

from quantile_model import ABOVE, BELOW, F32, LEVELS, exceedance, inputs, quantiles
from verify_model import narrow

pytestmark = pytest.mark.gpu
MAIN = ("u", "v", "dens", "u_prev", "v_prev", "dens_prev")
DT = 0.016
NAN32 = 0x7FC5A5A5                 # a NaN: memory the call must not write
UNORDERED = (0.9, 0.1, 0.5, 0.5, 1.0, 0.0)                 # a repeated level, no order
LEVELS16 = LEVELS + UNORDERED
DENS = 2                            # the field id of "dens"
assert len(LEVELS16) == 16


def F():
    import fluidsimulationcuda_amd as f
    return f


def torch_():
    import torch
    return torch


def solver(n, members, storage=0, **kw):
    return F().FluidSolver(n, members=members, storage=storage, **kw)


def floats(*v):
    return (C.c_float * len(v))(*v)


def shown(s, field):
    """what the pack shows: every member of a field, the lazy state settled"""
    return s.download_members(field)


def same(got, want, what):
    """bit for bit, except that a NaN is any NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F32, what
    ok = np.where(np.isnan(want), np.isnan(got), got.view(np.uint32) == want.view(np.uint32))
    if not ok.all():
        at = tuple(np.argwhere(~ok)[0])
        raise AssertionError("%s: %d of %d values differ; first at %s: got %r want %r" % (what, int((~ok).sum()), ok.size, at, got[at], want[at]))


def same_bits(got, want, what):
    """every bit, NaN payloads included: for memory the call must not have changed"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = got.view(np.uint8) != want.view(np.uint8)
    assert not bad.any(), "%s: %d of %d bytes changed; first at %s" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


def poisoned(count, w):
    torch = torch_()
    return torch.full((count, w, w), NAN32, dtype=torch.int32, device="cuda").view(torch.float32)


def run_q(s, levels, field="dens"):
    out = poisoned(len(levels), s.n + 2)
    assert s.quantiles(field, levels, out=out).data_ptr() == out.data_ptr()
    return out.cpu().numpy()


def run_e(s, thresholds, below=False, field="dens"):
    out = poisoned(len(thresholds), s.n + 2)
    assert s.exceedance(field, thresholds, below=below, out=out).data_ptr() == out.data_ptr()
    return out.cpu().numpy()


def check_q(s, x, levels, what, field="dens"):
    got = run_q(s, levels, field)
    same(got, quantiles(x, levels), what + ": the quantile maps")
    return got


def check_e(s, x, thresholds, what, field="dens"):
    for mode in (ABOVE, BELOW):
        same_bits(run_e(s, thresholds, mode == BELOW, field), exceedance(x, thresholds, mode), "%s: the exceedance maps, mode %d" % (what, mode))


# ---- 1. quantiles: every kernel at both ends of its range, other sizes, fp16 -----------------------------------------------------
@pytest.mark.parametrize("members", [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64])
def test_quantiles_at_both_ends_of_every_kernels_range(members):
    """M = MP / 2 + 1 and M = MP of every padded class, and M = 1; 16 levels (the ten, a repeated one, no order) and 1 level"""
    n = 14
    x = inputs(n, members, 0, seed=100 * n + members)
    with solver(n, members) as s:
        s.upload_members(dens=x)
        same_bits(shown(s, "dens"), x, "the upload")
        got = check_q(s, x, LEVELS16, "n=14 M=%d, 16 levels" % members)
        same_bits(got[12], got[13], "the repeated level")
        same_bits(got[5], got[12], "the median, wherever it is listed")
        check_q(s, x, (0.5,), "n=14 M=%d, 1 level" % members)
        r = s.quantiles()                                       # the defaults: the median of dens, a fresh tensor
        assert tuple(r.shape) == (1, n + 2, n + 2) and r.dtype == torch_().float32
        same_bits(r.cpu().numpy()[0], got[5], "quantiles() is the median of dens")


@pytest.mark.parametrize("members", [3, 8, 64])
def test_quantiles_at_other_sizes(members):
    for n in (30, 61):
        x = inputs(n, members, 0, seed=100 * n + members)
        with solver(n, members) as s:
            s.upload_members(dens=x)
            check_q(s, x, LEVELS16, "n=%d M=%d" % (n, members))
            check_q(s, x, (1.0 / 3.0,), "n=%d M=%d, 1 level" % (n, members))


@pytest.mark.parametrize("members", [2, 5, 33])
def test_quantiles_of_fp16_fields(members):
    for n in (14, 66):
        x = inputs(n, members, 1, seed=100 * n + members + 7)
        with solver(n, members, 1) as s:
            s.upload_members(dens=x)
            same_bits(shown(s, "dens"), x, "the upload")
            check_q(s, x, LEVELS16, "fp16 n=%d M=%d" % (n, members))
            check_q(s, x, (0.95,), "fp16 n=%d M=%d, 1 level" % (n, members))


# ---- 2. exceedance: the member loop's batches and its tail, ties, zeros, thresholds beyond everything -----------------------------
def exceed_inputs(n, members, storage, seed):
    """the shared inputs, and in a third of the cells member 0 equal to 0.25, in an eighth a member -0, in an eighth +0"""
    rng = np.random.default_rng(seed)
    x = inputs(n, members, storage, seed)
    w = n + 2
    x[0][rng.uniform(size=(w, w)) < 1.0 / 3.0] = F32(0.25)
    x[members // 2][rng.uniform(size=(w, w)) < 0.125] = F32(-0.0)
    x[members - 1][rng.uniform(size=(w, w)) < 0.125] = F32(0.0)
    return x


THRESHOLDS16 = (0.25, 0.0, -0.0, 1e30, -1e30, 100.0, -100.0, 0.5, -0.5, 3.0, -3.0, 0.25, 1e-45, -1e-45, 50.0, 0.001)
assert len(THRESHOLDS16) == 16


@pytest.mark.parametrize("members", [1, 2, 3, 64, 65, 200])
def test_exceedance_counts(members):
    n = 14
    x = exceed_inputs(n, members, 0, seed=7000 + members)
    assert (x == F32(0.25)).any(axis=0).mean() > 0.15 and (x == 0).any(axis=0).mean() > 0.1 and np.signbit(x[x == 0]).any()
    with solver(n, members) as s:
        s.upload_members(dens=x)
        check_e(s, x, THRESHOLDS16, "n=14 M=%d, 16 thresholds" % members)
        check_e(s, x, (0.25,), "n=14 M=%d, 1 threshold" % members)
        top, bottom = run_e(s, (1e30, -1e30)), run_e(s, (1e30, -1e30), below=True)
        assert not top[0].any() and (top[1] == 1).all() and (bottom[0] == 1).all() and not bottom[1].any()


def test_exceedance_of_fp16_fields():
    n, members = 66, 5
    x = exceed_inputs(n, members, 1, seed=7066)
    with solver(n, members, 1) as s:
        s.upload_members(dens=x)
        same_bits(shown(s, "dens"), x, "the upload")
        check_e(s, x, THRESHOLDS16, "fp16 n=66 M=5")
        check_e(s, x, (0.0,), "fp16 n=66 M=5, 1 threshold")


# ---- 3. planted cells ------------------------------------------------------------------------------------------------------------
def test_planted_cells():
    """one constant everywhere, one outlier member in one cell: every map is the model's everywhere -- the cell is seen and
    nothing else moves"""
    n, members = 30, 3
    w = n + 2
    cells = [(0, 0), (0, w - 1), (w - 1, 0), (w - 1, w - 1),          # the corners
             (3, w - 1), (4, 0),                                       # the last column of a row and the first of the next
             (63 // w, 63 % w), (64 // w, 64 % w),                     # the wave seam
             (255 // w, 255 % w), (256 // w, 256 % w)]                 # the block seam
    assert cells[6:] == [(1, 31), (2, 0), (7, 31), (8, 0)]
    const = F32(0.75)
    levels, thresholds = (0.0, 0.25, 0.5, 0.75, 1.0), (0.75, 1.0)
    with solver(n, members) as s:
        for k, (i, j) in enumerate(cells):
            x = np.full((members, w, w), const, F32)
            x[k % members, i, j] = F32(2.5) if k & 1 else F32(-1.5)
            s.upload_members(dens=x)
            q = check_q(s, x, levels, "cell (%d, %d) planted" % (i, j))
            assert (q[:, i, j] != const).sum() >= 2 and (np.delete(q.reshape(5, -1), i * w + j, axis=1) == const).all()
            check_e(s, x, thresholds, "cell (%d, %d) planted" % (i, j))
            e = run_e(s, thresholds, below=not (k & 1))
            assert e[0, i, j] == F32(1.0 / 3.0) and not np.delete(e[0].ravel(), i * w + j).any()


# ---- 4. memory not to be written -------------------------------------------------------------------------------------------------
def layout(n):
    from fluidsimulationcuda_amd import capi
    pitch, xoff, ff = C.c_int(), C.c_int(), C.c_size_t()
    assert capi.lib().fluid_layout(n, C.byref(pitch), C.byref(xoff), C.byref(ff)) == 0
    return pitch.value, xoff.value, ff.value


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_nothing_else_is_written_and_no_pad_is_read(storage):
    """level_stride = W * W + 5: the floats between the arrays, before the first and behind the last keep their bytes.  The
    context lives in an arena the test owns: with every pad column of the field a NaN pattern the maps are still the model's
    -- no pad is read as data -- and the arena holds the same bytes after the calls -- no pad, and nothing else, is written."""
    torch = torch_()
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    n, members = 30, 5
    w = n + 2
    cells, stride, lead = w * w, w * w + 5, 3
    x = inputs(n, members, storage, seed=4000 + storage)
    nbytes = L.fluid_arena_bytes_ensemble(n, storage, members)
    arena = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pitch, xoff, ff = layout(n)
    esz = 2 if storage else 4
    with solver(n, members, storage, arena_ptr=arena.data_ptr(), arena_bytes=nbytes) as s:
        s.upload_members(dens=x)
        s.synchronize()
        off = s.field_ptr("dens") - arena.data_ptr()
        assert off >= 0 and off % esz == 0
        v = arena[off:off + members * ff * esz].view(torch.int16 if storage else torch.int32).view(members, w, pitch)
        v[:, :, :xoff] = 0x7E5A if storage else NAN32
        v[:, :, xoff + w:] = 0x7E5A if storage else NAN32
        torch.cuda.synchronize()
        same_bits(shown(s, "dens"), x, "the field beside its poisoned pads")
        before = arena.cpu().numpy().copy()
        for count in (1, 3, 16):
            words = lead + (count - 1) * stride + cells + 5
            for kind in ("quantiles", "above", "below"):
                out = torch.full((words,), NAN32, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                if kind == "quantiles":
                    lv = LEVELS16[:count]
                    rc = L.fluid_member_quantiles(s._h, DENS, floats(*lv), count, out.data_ptr() + 4 * lead, stride)
                    want = quantiles(x, lv)
                else:
                    lv = THRESHOLDS16[:count]
                    mode = BELOW if kind == "below" else ABOVE
                    rc = L.fluid_member_exceedance(s._h, DENS, floats(*lv), count, mode, out.data_ptr() + 4 * lead, stride)
                    want = exceedance(x, lv, mode)
                assert rc == capi.OK, L.fluid_last_error()
                s.synchronize()
                got = out.cpu().numpy().view(np.uint32)
                untouched = np.ones(words, bool)
                for l in range(count):
                    at = lead + l * stride
                    same(got[at:at + cells].view(F32).reshape(w, w), want[l], "%s, storage %d, array %d of %d" % (kind, storage, l, count))
                    untouched[at:at + cells] = False
                assert untouched.sum() == lead + (count - 1) * 5 + 5 and (got[untouched] == NAN32).all(), "the floats between and around the arrays"
        same_bits(arena.cpu().numpy(), before, "the arena after the calls (storage %d)" % storage)


# ---- 5. non-finite members -------------------------------------------------------------------------------------------------------
def test_non_finite_members():
    n, members = 14, 5
    w = n + 2
    x = inputs(n, members, 0, seed=51)
    clean = x.copy()
    bad = [(4, 4), (0, 0), (w - 1, 9), (9, 1), (w - 1, w - 1)]
    x[1, 4, 4] = np.nan
    x[4, 0, 0] = np.inf
    x[0, w - 1, 9] = -np.inf
    x[0, 9, 1], x[2, 9, 1], x[4, 9, 1] = np.nan, np.inf, -np.inf       # all three, in different members
    x[:, w - 1, w - 1] = np.nan
    keep = np.ones((w, w), bool)
    for (i, j) in bad:
        keep[i, j] = False
    with solver(n, members) as s:
        s.upload_members(dens=clean)
        base = run_q(s, LEVELS16)
        s.upload_members(dens=x)
        got = check_q(s, x, LEVELS16, "non-finite members")
        assert all(np.isnan(got[:, i, j]).all() for (i, j) in bad)
        same_bits(got[:, keep], base[:, keep], "the quantiles of the other cells")
        thresholds = (0.0, 1e30, -1e30, float(clean[2, 4, 4]))
        check_e(s, x, thresholds, "non-finite members")
        above, below = run_e(s, thresholds), run_e(s, thresholds, below=True)
        # inf is counted, NaN is not: against +-1e30 the cell with all three has one member above, one below, three between
        assert above[1, 9, 1] == F32(0.2) and below[2, 9, 1] == F32(0.2) and above[2, 9, 1] == F32(0.6) and below[1, 9, 1] == F32(0.6)
        assert above[1, 0, 0] == F32(0.2) and below[2, w - 1, 9] == F32(0.2)
        assert not above[:, w - 1, w - 1].any() and not below[:, w - 1, w - 1].any()
        assert above[2, 4, 4] == F32(0.8) and below[1, 4, 4] == F32(0.8)


# ---- 6. lazy state ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_fields_a_step_has_left(storage):
    """after a step with sources dens owes itself a deferred source and, with fp16 storage from N = 16 on, u_prev holds the
    pressure at a scale.  What the pack shows comes from a twin context the calls never ran on."""
    n, members = 66, 5
    w = n + 2
    rng = np.random.default_rng(60 + storage)
    fields = {f: narrow(rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32), storage) for f in MAIN}

    def prepared():
        s = solver(n, members, storage)
        s.upload_members(**fields)
        s.step(use_sources=True)
        s.add_source("dens", "dens_prev", DT)
        return s

    with prepared() as s, prepared() as twin:
        for f in ("dens", "u_prev"):
            before = shown(twin, f)
            what = "storage %d, %s" % (storage, f)
            check_q(s, before, LEVELS, what, field=f)
            thresholds = (0.0, float(np.median(before)), float(before[0, w // 2, w // 2]))
            check_e(s, before, thresholds, what, field=f)
            same_bits(shown(s, f), before, what + " after the calls")
        for c in (s, twin):
            c.step(use_sources=True)
        for f in ("u", "v", "dens"):
            same_bits(shown(s, f), shown(twin, f), "%s a step after the calls" % f)


# ---- 7. wait=False ---------------------------------------------------------------------------------------------------------------
def test_unwaited_calls_on_a_shared_stream():
    """calls back to back without a wait in between, each with its own levels and its own tensor"""
    torch = torch_()
    n, members = 30, 8
    w = n + 2
    x = inputs(n, members, 0, seed=71)
    ts = torch.cuda.Stream()
    with solver(n, members, stream=ts.cuda_stream) as s:
        s.upload_members(dens=x)
        with torch.cuda.stream(ts):
            a, b, c, d = poisoned(3, w), poisoned(2, w), poisoned(2, w), poisoned(1, w)
            assert s.quantiles("dens", (0.05, 0.5, 0.95), out=a, wait=False).data_ptr() == a.data_ptr()
            s.quantiles("dens", (1.0, 0.25), out=b, wait=False)
            s.exceedance("dens", (0.5, -0.5), out=c, wait=False)
            s.exceedance("dens", (0.5,), below=True, out=d, wait=False)
            s.synchronize()
        same(a.cpu().numpy(), quantiles(x, (0.05, 0.5, 0.95)), "the first call")
        same(b.cpu().numpy(), quantiles(x, (1.0, 0.25)), "the second call")
        same_bits(c.cpu().numpy(), exceedance(x, (0.5, -0.5), ABOVE), "the third call")
        same_bits(d.cpu().numpy(), exceedance(x, (0.5,), BELOW), "the fourth call")


# ---- 8. refusals on a live context -----------------------------------------------------------------------------------------------
def hip_runtime():
    """the HIP runtime this process already holds (the one libfluid_amd.so runs on)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            lib = C.CDLL(line.split()[-1])
            lib.hipMalloc.argtypes, lib.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
            lib.hipFree.argtypes, lib.hipFree.restype = [C.c_void_p], C.c_int
            return lib
    raise RuntimeError("no HIP runtime is loaded")


def test_refusals_change_nothing():
    torch = torch_()
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(8)
    n, members = 6, 5
    w = n + 2
    cells = w * w
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    hip = hip_runtime()
    exact = C.c_void_p()
    size = 1 << 20
    assert hip.hipMalloc(C.byref(exact), size) == 0
    try:
        end = exact.value + size
        fits, short = end - 2 * cells * 4, end - 2 * cells * 4 + 4                 # two dense arrays that end with the allocation
        out = torch.full((3, w, w), NAN32, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        nan, inf = float("nan"), float("inf")

        def q(hnd, field=DENS, levels=(0.25, 0.5), count=None, o=None, stride=0):
            return lambda: L.fluid_member_quantiles(hnd, field, floats(*levels), len(levels) if count is None else count,
                                                    out.data_ptr() if o is None else o, stride)

        def e(hnd, field=DENS, th=(0.25, 0.5), count=None, mode=0, o=None, stride=0):
            return lambda: L.fluid_member_exceedance(hnd, field, floats(*th), len(th) if count is None else count, mode,
                                                     out.data_ptr() if o is None else o, stride)

        Q, E = b"fluid_member_quantiles", b"fluid_member_exceedance"
        with solver(n, members) as s, solver(n, members) as twin:
            for c in (s, twin):
                c.timing_enable(True)
                c.upload_members(**fields)
                c.step(use_sources=True)
                c.add_source("dens", "dens_prev", DT)                      # a lazy state that must survive the refusals
            hnd = s._h
            refused = [
                (lambda: L.fluid_member_quantiles(hnd, DENS, None, 2, out.data_ptr(), 0), (Q, b"levels")),
                (lambda: L.fluid_member_quantiles(hnd, DENS, floats(0.5), 1, None, 0), (Q, b"out_dev")),
                (lambda: L.fluid_member_exceedance(hnd, DENS, None, 2, 0, out.data_ptr(), 0), (E, b"thresholds")),
                (lambda: L.fluid_member_exceedance(hnd, DENS, floats(0.5), 1, 0, None, 0), (E, b"out_dev")),
                (q(None), (Q, b"null context")),
                (e(None), (E, b"null context")),
                (q(hnd, count=0), (Q, b"nlevels 0", b"[1, 16]")),
                (q(hnd, levels=(0.5,) * 17), (Q, b"nlevels 17")),
                (q(hnd, count=-1), (Q, b"nlevels -1")),
                (e(hnd, count=0), (E, b"nthresholds 0", b"[1, 16]")),
                (e(hnd, th=(0.5,) * 17), (E, b"nthresholds 17")),
                (q(hnd, field=12), (Q, b"bad field id 12")),
                (q(hnd, field=-1), (Q, b"bad field id -1")),
                (e(hnd, field=12), (E, b"bad field id 12")),
                (q(hnd, levels=(0.5, nan)), (Q, b"levels[1]", b"nan")),
                (q(hnd, levels=(inf, 0.5)), (Q, b"levels[0]", b"inf")),
                (q(hnd, levels=(0.5, 0.25, -0.1)), (Q, b"levels[2]", b"-0.1", b"[0, 1]")),
                (q(hnd, levels=(1.5,)), (Q, b"levels[0]", b"1.5", b"[0, 1]")),
                (e(hnd, th=(0.5, nan)), (E, b"thresholds[1]", b"not finite")),
                (e(hnd, th=(-inf, 0.5)), (E, b"thresholds[0]", b"not finite")),
                (e(hnd, mode=2), (E, b"mode 2")),
                (e(hnd, mode=-1), (E, b"mode -1")),
                (q(hnd, stride=cells - 1), (Q, b"level_stride %d" % (cells - 1),)),
                (e(hnd, stride=1), (E, b"level_stride 1",)),
                (q(hnd, stride=2 ** 62), (Q, b"level_stride", b"too large")),
                (q(hnd, o=short), (Q, b"out_dev", b"allocation ends")),
                (e(hnd, o=short), (E, b"out_dev", b"allocation ends")),
                (q(hnd, o=fits, stride=cells + 1), (Q, b"out_dev", b"allocation ends")),
                (q(hnd, o=fields["dens"].ctypes.data), (Q, b"not device memory")),
                (e(hnd, o=fields["dens"].ctypes.data), (E, b"not device memory")),
                (q(hnd, o=out.data_ptr() + 2), (Q, b"4 bytes")),
            ]
            for fn, words in refused:
                L.fluid_synchronize(None)                   # (an unrelated message in between)
                assert fn() == capi.E_INVALID, words
                msg = L.fluid_last_error()
                assert all(word in msg for word in words), (words, msg)
            s.synchronize()
            assert (out.cpu().numpy() == NAN32).all()
            ta, tb = s.timing_read(reset=False), twin.timing_read(reset=False)
            assert ta == {**tb, **{k: ta[k] for k in ta if k.endswith("_ms")}}             # every count; the times are times
            for f in capi.FIELD_NAMES:
                same_bits(shown(s, f), shown(twin, f), "%s after the refusals" % f)
            # what is not refused: arrays that end with their allocation
            assert q(hnd, o=fits)() == capi.OK, L.fluid_last_error()
            assert e(hnd, o=fits)() == capi.OK, L.fluid_last_error()
            s.synchronize()
            ta, tb = s.timing_read(reset=False), twin.timing_read(reset=False)
            assert ta == {**tb, **{k: ta[k] for k in ta if k.endswith("_ms")}}, "the launches belong to no timing category"
        with solver(n, 65) as s:
            x = rng.uniform(-1.0, 1.0, (65, w, w)).astype(F32)
            s.upload_members(dens=x)
            assert q(s._h)() == capi.E_INVALID
            msg = L.fluid_last_error()
            assert Q in msg and b"65 members" in msg and b"64" in msg, msg
            same_bits(shown(s, "dens"), x, "dens after the refusal")
            elsewhere = torch.zeros((2, w, w), dtype=torch.float32, device="cuda")
            assert e(s._h, o=elsewhere.data_ptr())() == capi.OK, "the exceedance has no cap"
            s.synchronize()
            same_bits(elsewhere.cpu().numpy(), exceedance(x, (0.25, 0.5)), "65 members above two thresholds")
        with F().FluidSolver(n, rank=0, nranks=2) as s:
            for fn, name in ((q(s._h), Q), (e(s._h), E)):
                assert fn() == capi.E_INVALID
                assert name in L.fluid_last_error() and b"slab" in L.fluid_last_error()
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == NAN32).all()
    finally:
        hip.hipFree(exact)


def test_the_solver_refuses_tensors_and_lists_of_the_wrong_kind():
    torch = torch_()
    n, members = 6, 3
    w = n + 2
    with solver(n, members) as s:
        s.upload_members(dens=np.random.default_rng(2).uniform(-1, 1, (members, w, w)).astype(F32))
        for bad in (torch.ones((2, w, w), dtype=torch.float32, device="cuda"), torch.ones((1, w, w), dtype=torch.float64, device="cuda"),
                    torch.ones((1, w, 2 * w), dtype=torch.float32, device="cuda")[:, :, ::2], torch.ones((1, w, w), dtype=torch.float32)):
            with pytest.raises(ValueError):
                s.quantiles("dens", (0.5,), out=bad)
            with pytest.raises(ValueError):
                s.exceedance("dens", (0.5,), out=bad)
        with pytest.raises(TypeError):
            s.quantiles("dens", (0.5,), out=np.ones((1, w, w), F32))
        for bad in ((), (0.5,) * 17, ((0.5, 0.25),)):
            with pytest.raises(ValueError):
                s.quantiles("dens", bad)
            with pytest.raises(ValueError):
                s.exceedance("dens", bad)
        with pytest.raises(RuntimeError):
            s.quantiles("dens", (1.5,))
        big = torch.zeros((4, 2, w, w), dtype=torch.float32, device="cuda")
        assert s.quantiles("u", (0.0, 1.0), out=big[2]).data_ptr() == big[2].data_ptr()
        assert s.exceedance("dens", 0.0).shape == (1, w, w)                       # a scalar is a list of one
