"""GPU: block-averaged ensemble snapshots -- fluid_pack_members_coarse, fluid_download_members_coarse, fluid_run_coarse /
fluid_run_members_coarse (include/fluid_amd.h, "coarse snapshots").

The expected values come from `model` below, the header's definition in numpy: float64 arrays, the columns of a block
summed level by level as d[:, 0::2] + d[:, 1::2], then the rows added one after the other starting from row 0, one exact
scaling, one rounding to float.  It is applied to what download(field, member=m) returns.  Every comparison is bit for bit;
there is no tolerance anywhere.  Device buffers are torch tensors."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_ensemble import member_fields, solver, upload_all
from test_gpu_ensemble_reduce import hip_runtime, stages
from test_gpu_lazy_state import NAMES

pytestmark = pytest.mark.gpu
F32 = np.float32
DT, VISC, DIFF = 0.016, 0.0025, 0.1
SENTINEL = 0x7FA5C3C3        # the bit pattern of a NaN that no computation here produces
FACTORS = (1, 2, 4, 8, 16, 32, 64)


def torch_():
    import torch
    return torch


def factors_of(n):
    return [r for r in FACTORS if (n + 2) % r == 0]


def model(x, r):
    """(..., H, W) float32 -> (..., H / r, W / r) float32: the definition, step by step"""
    d = np.asarray(x, F32).astype(np.float64)
    k = r
    while k > 1:                                        # 1. the pairwise tree over adjacent columns, level by level
        d = d[..., 0::2] + d[..., 1::2]
        k //= 2
    lead, rows, cols = d.shape[:-2], d.shape[-2], d.shape[-1]
    d = d.reshape(lead + (rows // r, r, cols))
    s = d[..., 0, :].copy()                             # 2. s = p_0, then the rows in order
    for i in range(1, r):
        s = s + d[..., i, :]
    return (s * (1.0 / (r * r))).astype(F32)            # 3. exact scaling, one rounding (numpy keeps float denormals)


def sequential_model(x, r):
    """what the test must NOT be blind to: the same block summed cell after cell in row-major order"""
    d = np.asarray(x, F32).astype(np.float64)
    lead, rows, cols = d.shape[:-2], d.shape[-2], d.shape[-1]
    d = d.reshape(lead + (rows // r, r, cols // r, r))
    s = d[..., 0, :, 0].copy()
    for i in range(r):
        for j in range(r):
            if i or j:
                s = s + d[..., i, :, j]
    return (s * (1.0 / (r * r))).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_same_bits(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), "%s: %d of %d coarse cells differ; first at %s: got %08x want %08x" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def on_host(t):
    return t.cpu().numpy()


# ---- the data ----------------------------------------------------------------------------------------------------------------
def cancellation(rng, members, w, r, shift=0):
    """every r x r block holds +2^k and -2^k (k from 30 .. 49, less `shift`) in two random cells, uniform(-1, 1) elsewhere"""
    x = rng.uniform(-1, 1, size=(members, w, w)).astype(F32)
    if r < 2:
        return x
    c = w // r
    a = rng.integers(0, r * r, size=(members, c, c))
    b = (a + rng.integers(1, r * r, size=(members, c, c))) % (r * r)
    big = np.exp2(rng.integers(30, 50, size=(members, c, c)) - shift).astype(F32)
    m, bi, bj = np.meshgrid(np.arange(members), np.arange(c), np.arange(c), indexing="ij")
    x[m, bi * r + a // r, bj * r + a % r] = big
    x[m, bi * r + b // r, bj * r + b % r] = -big
    return x


def zero_blocks(members, c):
    """(members, c, c): the blocks that are -0 everywhere -- a checkerboard, shifted from member to member"""
    m, bi, bj = np.indices((members, c, c))
    return (m + bi + bj) % 2 == 0


def special(rng, members, w, r):
    """fp32 only: denormals around 1e-40, every other block all -0, one NaN and one inf per member in different blocks;
    returns the data and the (member, I, J) of the poisoned coarse cells"""
    x = (rng.uniform(-4, 4, size=(members, w, w)) * 1e-40).astype(F32)
    c = w // r
    x[np.repeat(np.repeat(zero_blocks(members, c), r, axis=1), r, axis=2)] = F32(-0.0)
    poisoned = []
    for m in range(members):
        if c * c >= 2:
            p, q = rng.choice(c * c, size=2, replace=False)
            for at, v in ((p, np.nan), (q, np.inf)):
                x[m, (at // c) * r + rng.integers(r), (at % c) * r + rng.integers(r)] = v
                poisoned.append((m, at // c, at % c))
    return x, poisoned


def draw(kind, rng, members, w, r, storage):
    if kind == "uniform":
        return rng.uniform(-1, 1, size=(members, w, w)).astype(F32), None
    if kind == "cancellation":
        # fp16 storage holds nothing above 65504: there the exponents are 35 lower (2^-5 .. 2^14), the largest range a half
        # takes.  (A double then holds every partial sum exactly: it is the fp32 cases that tell the orders apart.)
        return cancellation(rng, members, w, r, shift=35 if storage else 0), None
    if kind == "special":
        return special(rng, members, w, r)
    return rng.integers(-8, 9, size=(members, w, w)).astype(F32), None


# ---- 1. sizes, factors, members, data: the coarse pack against the model ------------------------------------------------------
SIZES = [1, 2, 6, 14, 30, 61, 62, 126, 254, 1022, 2046]
KINDS = ["uniform", "cancellation", "special", "integers"]


def members_for(n):
    return (1, 2) if n == 2046 else (1, 2, 3, 5, 16)


# (fp16 storage has no float denormals to keep, and the -0 / NaN / inf cases are about the double sum: fp32 storage only)
CASES = [(storage, kind) for storage in (0, 1) for kind in KINDS if not (storage and kind == "special")]


@pytest.mark.parametrize("storage, kind", CASES, ids=["%s-%s" % (("f32", "f16")[st], k) for st, k in CASES])
@pytest.mark.parametrize("n", SIZES)
def test_coarse_pack_equals_the_model(n, storage, kind):
    torch = torch_()
    w = n + 2
    most = max(members_for(n))
    rng = np.random.default_rng([n, storage, KINDS.index(kind)])
    # data that depends on the factor (cancellation, special) is drawn per factor; the model is computed once per data set,
    # in the largest ensemble, from what the library shows of it, and shared by the smaller ones
    per_factor = kind in ("cancellation", "special")
    data, want = {}, {}
    x = shown = None
    for members in sorted(members_for(n), reverse=True):
        with solver(n, members, storage=storage) as s:
            for r in factors_of(n):
                if members == most:
                    if per_factor or x is None:
                        x, poisoned = draw(kind, rng, most, w, r, storage)
                        s.upload_members(dens=x)
                        shown = np.stack([s.download("dens", member=m) for m in range(most)])
                        if not storage:
                            assert np.array_equal(bits(shown), bits(x))
                    data[r], want[r] = x, model(shown, r)
                    check_the_model(kind, storage, n, r, shown, want[r], poisoned)
                elif per_factor or r == 1:
                    s.upload_members(dens=data[r][:members])
                got = s.pack("dens", coarse=r)
                what = "n=%d M=%d storage=%d %s r=%d" % (n, members, storage, kind, r)
                assert tuple(got.shape) == (members, w // r, w // r), what
                assert_same_bits(on_host(got), want[r][:members], what)
                if r == 1:
                    assert torch.equal(got.view(torch.int32), s.pack("dens").view(torch.int32)), what + ": r = 1 is the dense pack"


def check_the_model(kind, storage, n, r, shown, want, poisoned):
    """what each kind of data is there for, asserted of the model itself before anything is compared with it"""
    most, c = shown.shape[0], shown.shape[1] // r
    if kind == "cancellation" and not storage and r >= 4:
        few = slice(0, 2)               # (two members are enough to see it)
        blind = bits(want[few]) == bits(sequential_model(shown[few], r))
        print("n=%d r=%d: the model and a row-major sequential sum agree on %d of %d cells" % (n, r, int(blind.sum()), blind.size))
        assert (~blind).sum() * 4 >= blind.size, "the data does not tell the specified order from a sequential sum"
    if kind == "integers":
        mean = shown.astype(np.float64).reshape(most, c, r, c, r).mean(axis=(2, 4))
        assert np.array_equal(bits(want), bits(mean.astype(F32)))
    if kind == "special":
        finite = np.isfinite(want)
        assert sorted(set(poisoned)) == sorted(map(tuple, np.argwhere(~finite))), "only the blocks that hold the NaN / the inf"
        assert (bits(want)[zero_blocks(most, c) & finite] == 0x80000000).all(), "a block of -0 has the mean -0"
        rest = ~zero_blocks(most, c) & finite
        assert not rest.any() or (want[rest] != 0).any(), "the denormal means were flushed"


# ---- 2. the shape of the call ---------------------------------------------------------------------------------------------------
def sentinel_buffer(words):
    torch = torch_()
    return torch.full((words,), SENTINEL, dtype=torch.int32, device="cuda")


def check_coarse_pack(s, field, r, variant, what):
    """one coarse pack of `field` -- the shape of the call by `variant` -- into a sentinel-filled buffer, then the model of
    every member's download: the same bits in the members' cells, the sentinel everywhere else"""
    members, side = s.members, (s.n + 2) // r
    cells = side * side
    stride = cells + 3 if variant in (1, 2) else 0
    lead = 1 if variant in (1, 2, 3) else 0              # the base pointer offset by one float
    first, count = {0: (0, 0), 1: (0, 0), 2: (members // 2, 0), 3: (0, max(1, members - 1))}[variant]
    moved = count or members - first
    step = stride or cells
    words = lead + (moved - 1) * step + cells + 5
    buf = sentinel_buffer(words)
    s.pack(field, out=buf.view(torch_().float32)[lead:], first=first, count=count, member_stride=stride, coarse=r)
    got = on_host(buf).view(np.uint32)
    mask = np.ones(words, bool)
    for k in range(moved):
        at = lead + k * step
        want = model(s.download(field, member=first + k), r)
        assert_same_bits(got[at:at + cells].view(F32).reshape(side, side), want, "%s: %s member %d r=%d (variant %d)" % (what, field, first + k, r, variant))
        mask[at:at + cells] = False
    assert (got[mask] == SENTINEL).all(), "%s: %s r=%d variant %d: words outside the members' cells were written" % (what, field, r, variant)


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n, members", [(14, 5), (62, 3), (126, 2)])
def test_shape_of_the_call(n, members, storage):
    rng = np.random.default_rng(n)
    with solver(n, members, storage=storage) as s:
        s.upload_members(u=rng.uniform(-1, 1, size=(members, n + 2, n + 2)).astype(F32))
        for r in factors_of(n):
            for variant in range(4):
                check_coarse_pack(s, "u", r, variant, "n=%d M=%d storage=%d" % (n, members, storage))


# ---- 3. lazy state ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n, members", [(62, 3), (14, 2)])
def test_coarse_pack_meets_every_lazy_state_and_disturbs_nothing(oracle, n, members, storage):
    """the stage sequence of the ensemble diagnostics' tests: each look names two fields -- zero by definition, owing an
    increment, (fp16) kept scaled -- and the coarse pack comes first, so that it is the pack that meets the state; a twin
    context goes through the same calls without a look, and all twelve fields of all members must agree at the end"""
    fields = member_fields(oracle, n, members, seed=n)
    rs = factors_of(n)
    with solver(n, members, storage=storage) as s, solver(n, members, storage=storage) as twin:
        upload_all(s, fields)
        upload_all(twin, fields)
        calls = [0]

        def look(a, b, *_):
            for f in (a, b):
                check_coarse_pack(s, f, rs[calls[0] % len(rs)], (calls[0] + members) % 4, "n=%d M=%d storage=%d look %d" % (n, members, storage, calls[0]))
                calls[0] += 1
            return F32(0)

        stages(s, oracle, look, look)
        stages(twin, oracle, lambda *_: F32(0), lambda *_: F32(0))
        assert calls[0] >= 2 * len(rs)
        for m in range(members):
            for k in NAMES:
                assert_same_bits(s.download(k, member=m), twin.download(k, member=m), "%s of member %d after the looks" % (k, m))


# ---- 4. the host path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n, members", [(1, 1), (14, 5), (62, 16), (1022, 17)])
def test_download_members_coarse_equals_the_pack(n, members, storage):
    """(1022, 17): sixteen dense members fill the 64 MiB staging buffer, so r = 1 moves two groups through it"""
    rng = np.random.default_rng(n + members)
    with solver(n, members, storage=storage) as s:
        s.upload_members(dens=rng.uniform(-1, 1, size=(members, n + 2, n + 2)).astype(F32))
        for r in factors_of(n):
            assert_same_bits(s.download_members("dens", coarse=r), on_host(s.pack("dens", coarse=r)), "n=%d M=%d r=%d" % (n, members, r))
        s.step(2, iters=4)              # lazy fields through the bulk download: zero by definition, fp16: kept scaled
        for k in ("u_prev", "dens_prev"):
            r = factors_of(n)[-1]
            got = s.download_members(k, coarse=r)
            want = np.stack([model(s.download(k, member=m), r) for m in range(members)])
            assert_same_bits(got, want, "n=%d M=%d %s r=%d after two steps" % (n, members, k, r))
        with pytest.raises(ValueError):
            s.download_members("dens", out=np.empty((members, n + 2, n + 3), F32), coarse=1)


# ---- 5. recorded runs -----------------------------------------------------------------------------------------------------------------
RUN_FIELDS = ("u", "dens", "u_prev")


@pytest.mark.parametrize("per_member", [False, True], ids=["scalar", "members"])
@pytest.mark.parametrize("r", [None, 2, 8])
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n", [62, 254])
def test_run_coarse_equals_the_loop_of_calls(oracle, n, storage, r, per_member):
    from fluidsimulationcuda_amd import capi
    torch = torch_()
    members, iters, nsteps, every = 3, 4, 4, 2
    side = n + 2 if r is None else (n + 2) // r
    par = dict(dt=[0.016, 0.008, 0.03], diff=[0.1, 0.0, 0.02], visc=[0.0025, 0.01, 0.0]) if per_member else dict(dt=DT, diff=DIFF, visc=VISC)
    fields = member_fields(oracle, n, members, seed=n, kinds=("parameters", "uniform", "coarse"))
    rng = np.random.default_rng(n)
    sources = torch.from_numpy(rng.uniform(-1, 1, size=(3, members, n + 2, n + 2)).astype(F32)).cuda()
    what = "n=%d storage=%d r=%r per_member=%d" % (n, storage, r, per_member)
    with solver(n, members, storage=storage) as loop:
        upload_all(loop, fields)
        want = []
        for z in range(nsteps):
            for k, name in enumerate(("u_prev", "v_prev", "dens_prev")):
                loop.unpack(name, sources[k])
            loop.step(1, use_sources=True, iters=iters, **par)
            if (z + 1) % every == 0:
                want.append([on_host(loop.pack(f, coarse=r)) for f in RUN_FIELDS])
        want_final = [[loop.download(f, member=m) for f in NAMES] for m in range(members)]
    exact = (nsteps // every) * len(RUN_FIELDS) * members * side * side
    with solver(n, members, storage=storage) as s:
        upload_all(s, fields)
        before = [s.download(f, member=1) for f in NAMES]
        short = torch.zeros(exact - 1, dtype=torch.float32, device="cuda")
        with pytest.raises(capi.FluidError, match="capacity"):
            s.run(nsteps, every=every, fields=RUN_FIELDS, sources=sources, out=short, iters=iters, coarse=r, **par)
        assert not short.any().item()
        for f, x in zip(NAMES, before):
            assert_same_bits(s.download(f, member=1), x, what + ": %s after the refused run" % f)
        out = sentinel_buffer(exact)
        got, written = s.run(nsteps, every=every, fields=RUN_FIELDS, sources=sources, out=out.view(torch.float32), iters=iters, coarse=r, **par)
        assert written == nsteps // every == len(want)
        got = on_host(got).reshape(written, len(RUN_FIELDS), members, side, side)
        for k in range(written):
            for f, name in enumerate(RUN_FIELDS):
                assert_same_bits(got[k, f], want[k][f], "%s: snapshot %d %s" % (what, k, name))
        for m in range(members):
            for k, name in enumerate(NAMES):
                assert_same_bits(s.download(name, member=m), want_final[m][k], "%s: final %s member %d" % (what, name, m))
        # out=None allocates the coarse shape
        alloc, written = s.run(2, every=1, fields=("dens",), iters=iters, coarse=r)
        assert written == 2 and tuple(alloc.shape) == (2, 1, members, side, side)
        assert_same_bits(on_host(alloc[1, 0]), on_host(s.pack("dens", coarse=r)), what + ": the last snapshot of an allocated run")


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from fluidsimulationcuda_amd import capi
    import fluidsimulationcuda_amd as F
    torch = torch_()
    hip = hip_runtime()
    n, members, r = 30, 5, 4
    side = (n + 2) // r
    cells = side * side
    L = capi.lib()
    rng = np.random.default_rng(30)
    x = rng.uniform(-1, 1, size=(members, n + 2, n + 2)).astype(F32)
    good = np.linspace(0.5, 1.5, members).astype(F32)
    host = np.zeros((members, n + 2, n + 2), F32)
    dev = torch.zeros(4 * members * cells, dtype=torch.float32, device="cuda")     # two coarse snapshots of two fields
    ids = (C.c_int * 2)(0, 2)
    bad_ids = (C.c_int * 2)(0, 12)
    written = C.c_int(-7)
    exact = C.c_void_p()
    size = 1 << 20
    assert hip.hipMalloc(C.byref(exact), C.c_size_t(size)) == 0
    span = members * cells * 4
    fits = exact.value + size - span                # a coarse array of all members that ends with the allocation
    short = fits + 4                                # ... and one that is one float too short

    def mf(a):
        return a.ctypes.data_as(capi._MF)

    def plan(**kw):
        p = dict(iters=4, nsteps=4, use_sources=0, sources=None, every=2, fields=ids, nfields=2, snapshots=dev.data_ptr(), capacity=dev.numel())
        p.update(kw)
        return C.byref(capi.RunPlan(**p))

    def run(factor=r, **kw):
        return lambda: L.fluid_run_coarse(hnd, DT, DIFF, VISC, plan(**kw), factor, C.byref(written))

    def run_m(factor=r, dt=None, **kw):
        dt = good if dt is None else dt
        return lambda: L.fluid_run_members_coarse(hnd, mf(dt), mf(good), mf(good), plan(**kw), factor, C.byref(written))

    def pack(field=0, first=0, count=0, factor=r, dst=None, stride=0):
        return lambda: L.fluid_pack_members_coarse(hnd, field, first, count, factor, d if dst is None else dst, stride)

    try:
        with solver(n, members) as s:
            s.upload_members(u=x, v=x[::-1].copy(), dens=x)
            s.computeDivergenceAndPressure("u", "v", "u_prev", "v_prev")        # a lazy state that must survive the refusals
            s.add_source("dens", "u_prev", DT)
            hnd, d = s._h, dev.data_ptr()
            refused = [
                ("fluid_pack_members_coarse", lambda: L.fluid_pack_members_coarse(hnd, 0, 0, 0, r, None, 0), b"dst_dev"),
                ("fluid_pack_members_coarse", pack(field=12), b"12"),
                ("fluid_pack_members_coarse", pack(field=-1), b"-1"),
                ("fluid_pack_members_coarse", pack(first=-1), b"first -1"),
                ("fluid_pack_members_coarse", pack(first=6), b"first 6"),
                ("fluid_pack_members_coarse", pack(first=2, count=4), b"count 4"),
                ("fluid_pack_members_coarse", pack(count=-2), b"count -2"),
                ("fluid_pack_members_coarse", pack(stride=cells - 1), b"member_stride"),
                ("fluid_pack_members_coarse", pack(dst=host.ctypes.data), b"not device memory"),
                ("fluid_pack_members_coarse", pack(dst=short), b"allocation ends"),
                ("fluid_pack_members_coarse", pack(dst=d, stride=1 << 40), b"allocation ends"),
                ("fluid_pack_members_coarse", pack(dst=fits, factor=2), b"allocation ends"),      # the span is the factor's
                ("fluid_download_members_coarse", lambda: L.fluid_download_members_coarse(hnd, 0, r, None), b"null host pointer"),
                ("fluid_download_members_coarse", lambda: L.fluid_download_members_coarse(hnd, 12, r, mf(host)), b"12"),
                ("fluid_run_coarse", lambda: L.fluid_run_coarse(hnd, DT, DIFF, VISC, None, r, None), b"null plan"),
                ("fluid_run_coarse", run(iters=3), b"sweep count"),
                ("fluid_run_coarse", run(nsteps=-1), b"nsteps"),
                ("fluid_run_coarse", run(every=-1), b"every"),
                ("fluid_run_coarse", run(nfields=0), b"nfields"),
                ("fluid_run_coarse", run(fields=None), b"fields"),
                ("fluid_run_coarse", run(fields=bad_ids), b"12"),
                ("fluid_run_coarse", run(snapshots=None), b"snapshots"),
                ("fluid_run_coarse", run(capacity=2 * 2 * members * cells - 1), b"capacity"),
                ("fluid_run_coarse", run(factor=2), b"capacity"),                 # the same buffer is too small for factor 2
                ("fluid_run_coarse", run(snapshots=host.ctypes.data), b"not device memory"),
                ("fluid_run_coarse", run(snapshots=short, nsteps=2, nfields=1, capacity=members * cells), b"allocation ends"),
                ("fluid_run_coarse", run(sources=host.ctypes.data), b"not device memory"),
                ("fluid_run_members_coarse", lambda: L.fluid_run_members_coarse(hnd, mf(good), mf(good), mf(good), None, r, None), b"null plan"),
                ("fluid_run_members_coarse", lambda: L.fluid_run_members_coarse(hnd, mf(good), None, mf(good), plan(), r, None), b"diff"),
                ("fluid_run_members_coarse", run_m(iters=5), b"sweep count"),
                ("fluid_run_members_coarse", run_m(capacity=7), b"capacity"),
            ]
            for factor in (0, 3, 128, -2):          # not one of the seven values
                word = b"factor %d" % factor
                refused += [("fluid_pack_members_coarse", pack(factor=factor), word),
                            ("fluid_download_members_coarse", lambda factor=factor: L.fluid_download_members_coarse(hnd, 0, factor, mf(host)), word),
                            ("fluid_run_coarse", run(factor=factor), word), ("fluid_run_members_coarse", run_m(factor=factor), word)]
            word = b"divide N + 2 = 32"             # one of the seven, and no divisor of 32
            refused += [("fluid_pack_members_coarse", pack(factor=64), word),
                        ("fluid_download_members_coarse", lambda: L.fluid_download_members_coarse(hnd, 0, 64, mf(host)), word),
                        ("fluid_run_coarse", run(factor=64), word), ("fluid_run_members_coarse", run_m(factor=64), word)]
            u0 = s.download("u", member=3)
            want = np.stack([model(s.download("dens", member=m), r) for m in range(members)])
            for name, call, word in refused:
                L.fluid_synchronize(None)               # (an unrelated message in between)
                assert call() == capi.E_INVALID, (name, word)
                msg = L.fluid_last_error()
                assert name.encode() in msg and word in msg, (name, word, msg)
                assert written.value == -7 and not dev.any().item(), (name, word)
                assert_same_bits(s.download("u", member=3), u0, "u after the refusal %r" % ((name, word),))
                assert L.fluid_pack_members_coarse(hnd, 2, 0, 0, r, fits, 0) == capi.OK, (name, word)      # ends with its allocation
                s.synchronize()
                got = np.empty((members, side, side), F32)
                assert hip.hipMemcpy(got.ctypes.data, fits, span, 2) == 0
                assert_same_bits(got, want, "a valid call after the refusal %r" % ((name, word),))
            got = on_host(s.pack("u_prev", first=2, count=1, coarse=r))[0]          # zero by definition, never looked at so far
            assert_same_bits(got, model(s.download("u_prev", member=2), r), "the lazy field after the refusals")
        # row slabs: every call that takes a context is refused
        with F.FluidSolver(n, rank=0, nranks=2) as s:
            hnd, d = s._h, dev.data_ptr()
            one = (C.c_float * 1)(0.5)
            for name, call in (("fluid_pack_members_coarse", pack()),
                               ("fluid_download_members_coarse", lambda: L.fluid_download_members_coarse(hnd, 0, r, mf(host))),
                               ("fluid_run_coarse", run()),
                               ("fluid_run_members_coarse", lambda: L.fluid_run_members_coarse(hnd, one, one, one, plan(), r, None))):
                assert call() == capi.E_INVALID, name
                msg = L.fluid_last_error()
                assert name.encode() in msg and b"slab" in msg, (name, msg)
    finally:
        assert hip.hipFree(exact) == 0


# ---- 7. limits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_the_maximum_member_count(storage):
    from fluidsimulationcuda_amd import capi
    n, members = 6, capi.MAX_MEMBERS
    rng = np.random.default_rng(members)
    x = rng.uniform(-1, 1, size=(members, n + 2, n + 2)).astype(F32)
    with solver(n, members, storage=storage) as s:
        s.upload_members(v=x)
        for r in (1, 8):
            got = on_host(s.pack("v", coarse=r))
            host = s.download_members("v", coarse=r)
            assert got.shape == (members, 8 // r, 8 // r)
            for m in (0, members // 2, members - 1):
                want = model(s.download("v", member=m), r)
                assert_same_bits(got[m], want, "member %d r=%d" % (m, r))
                assert_same_bits(host[m], want, "member %d r=%d through the host path" % (m, r))
            assert np.array_equal(bits(got), bits(host))


def test_a_field_past_4_gib():
    """N = 32800, the size at which tests/test_gpu_huge.py takes a field past 4 GiB (4.3 GB in fp32): the 64-bit field offsets
    of the coarse pack.  N + 2 = 32802 = 2 * 16401 leaves the factors 1 and 2.  Compared with the model on bands of rows at
    both ends and in the middle -- the last rows are the highest addresses -- and, over the whole array, with the same sum
    in torch on the device: the values are small integers, every order gives the same double."""
    torch = torch_()
    n = 32800
    w = n + 2
    with solver(n, 1) as s:
        src = torch.arange(w * w, dtype=torch.float32, device="cuda").remainder_(2039.0).sub_(1019.0)
        s.unpack("u", src)
        got = s.pack("u", coarse=2)
        assert tuple(got.shape) == (1, w // 2, w // 2)
        rows = src.view(w, w)
        for lo in (0, (w // 4) * 2, w - 8):
            want = model(on_host(rows[lo:lo + 8]), 2)
            assert_same_bits(on_host(got[0, lo // 2:lo // 2 + 4]), want, "rows %d .. %d" % (lo, lo + 7))
        whole = rows[0::2, 0::2].double()
        whole += rows[0::2, 1::2]
        whole += rows[1::2, 0::2]
        whole += rows[1::2, 1::2]
        whole *= 0.25
        assert torch.equal(got[0].view(torch.int32), whole.float().view(torch.int32))
        del whole
        assert torch.equal(s.pack("u", coarse=1).view(-1).view(torch.int32), src.view(torch.int32)), "r = 1"
