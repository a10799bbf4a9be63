"""GPU: moving whole ensembles -- fluid_pack_members / fluid_unpack_members (one launch between the library's layout and a
dense float array on the device), fluid_download_members / fluid_upload_members (bulk host copies built on them) and
fluid_run / fluid_run_members (forced, recorded runs without the host in the loop).

What each is held to (include/fluid_amd.h, "moving ensembles"), bit for bit throughout, no tolerance anywhere:
- pack: every cell of every member equals fluid_download_member right after the call, in every lazy state; whatever the
  destination held outside the members' cells (stride gaps, the words before and behind) is untouched;
- unpack: fluid_download_member gives the input back (fp16 storage: numpy's float16 rounding of it), the pad columns of the
  whole arena stay zero, the lazy marks are dropped (all members) or settled for the others (a sub-range);
- the bulk host calls: the per-member loops they replace;
- run: the loop of unpack / step / pack calls it is defined as, and the oracle per member where the oracle applies (fp32).
Device buffers are torch tensors."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import rnd
from test_gpu_ensemble import compare_all, ensemble_ops, member_fields, play_ensemble, solver, upload_all
from test_gpu_ensemble_reduce import COUNTERS, hip_runtime, stages
from test_gpu_f16 import h
from test_gpu_lazy_state import COARSE, NAMES, Model, draw_fields, draw_sequence, play, same_bits

pytestmark = pytest.mark.gpu
F32 = np.float32
DT, VISC, DIFF = 0.016, 0.0025, 0.1
SENTINEL = 0x7FA5C3C3        # the bit pattern of a NaN that no computation here produces
PACK_SIZES = [1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 61, 62, 63, 64, 65, 254, 258, 1022]
MEMBERS = [1, 2, 3, 5, 16]


def torch_():
    import torch
    return torch


def sentinel_buffer(words):
    torch = torch_()
    return torch.full((words,), SENTINEL, dtype=torch.int32, device="cuda")


def layout(n):
    from fluidsimulationcuda_amd import capi
    pitch, xoff, ff = C.c_int(), C.c_int(), C.c_size_t()
    assert capi.lib().fluid_layout(n, C.byref(pitch), C.byref(xoff), C.byref(ff)) == 0
    return pitch.value, xoff.value, ff.value


# ---- 1. pack against fluid_download_member ---------------------------------------------------------------------------------
def check_pack(s, field, variant, what):
    """one pack of `field` -- the shape of the call by `variant` -- into a sentinel-filled buffer, then every member's
    download: the same bits in the members' cells, the sentinel everywhere else"""
    n, members, cells = s.n, s.members, (s.n + 2) ** 2
    stride = cells + 3 if variant in (1, 2) else 0
    lead = 1 if variant in (1, 2, 3) else 0              # the base pointer offset by one float
    first, count = {0: (0, 0), 1: (0, 0), 2: (members // 2, 0), 3: (0, max(1, members - 1))}[variant]
    moved = count or members - first
    step = stride or cells
    words = lead + (moved - 1) * step + cells + 5
    buf = sentinel_buffer(words)
    s.pack(field, out=buf.view(torch_().float32)[lead:], first=first, count=count, member_stride=stride)
    got = buf.cpu().numpy().view(np.uint32)
    mask = np.ones(words, bool)
    for k in range(moved):
        at = lead + k * step
        want = s.download(field, member=first + k)
        assert np.array_equal(got[at:at + cells], want.view(np.uint32).ravel()), \
            "%s: %s member %d (variant %d): %d cells differ from fluid_download_member" % (
                what, field, first + k, variant, int((got[at:at + cells] != want.view(np.uint32).ravel()).sum()))
        mask[at:at + cells] = False
    assert (got[mask] == SENTINEL).all(), "%s: %s variant %d: words outside the members' cells were written" % (what, field, variant)


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n", PACK_SIZES)
def test_pack_equals_download_member(oracle, n, storage):
    fields = member_fields(oracle, n, max(MEMBERS), seed=n)
    for members in MEMBERS:
        with solver(n, members, storage=storage) as s:
            upload_all(s, fields[:members])
            calls = [0]

            def look(a, b, *_):
                # the stages of the ensemble diagnostics' tests name two fields per look; the pack comes first, so that it
                # is the pack that meets the lazy state (zero by definition, an increment owed, fp16: a scale kept)
                for f in (a, b):
                    check_pack(s, f, (calls[0] + members) % 4, "n=%d M=%d storage=%d look %d" % (n, members, storage, calls[0]))
                    calls[0] += 1
                return F32(0)

            stages(s, oracle, look, look)


# ---- 2. unpack --------------------------------------------------------------------------------------------------------------
def arena_ensemble(n, members, storage=0, params=None):
    """an ensemble on a torch arena: the whole arena can be looked at"""
    import fluidsimulationcuda_amd as F
    from fluidsimulationcuda_amd import capi
    torch = torch_()
    nbytes = capi.lib().fluid_arena_bytes_ensemble(n, storage, members)
    arena = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = F.FluidSolver(n, members=members, storage=storage, arena_ptr=arena.data_ptr(), arena_bytes=nbytes, params=params)
    return s, arena


def arena_fields(s, arena):
    """the arena as (12 x members, N+2, pitch) stored elements (uint16 / uint32 bit patterns), and where each field starts"""
    pitch, xoff, ff = layout(s.n)
    s.synchronize()
    torch_().cuda.synchronize()
    dtype = np.uint16 if s.storage else np.uint32
    raw = arena.cpu().numpy()[:12 * s.members * ff * dtype().itemsize].view(dtype)
    return raw.reshape(12 * s.members, s.n + 2, pitch), xoff


def stored_bits(s, arena, field):
    """(members, N+2, N+2) bit patterns of a field as the device holds it"""
    pitch, xoff, ff = layout(s.n)
    esz = 2 if s.storage else 4
    at = (s.field_ptr(field) - arena.data_ptr()) // (ff * esz)
    all_fields, xoff = arena_fields(s, arena)
    return all_fields[at:at + s.members, :, xoff:xoff + s.n + 2]


def pads_are_zero(s, arena, what):
    all_fields, xoff = arena_fields(s, arena)
    w = s.n + 2
    assert not all_fields[:, :, :xoff].any() and not all_fields[:, :, xoff + w:].any(), "%s: pad columns were written" % what


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_unpack_then_download_and_the_pads(storage):
    torch = torch_()
    rng = np.random.default_rng(storage)
    for n in PACK_SIZES[:-1]:
        for members in (1, 3, 16) if n < 200 else (2,):
            w = n + 2
            x = rng.uniform(0.5, 2.0, size=(members, w, w)).astype(F32)       # no zero anywhere: a pad written would show
            x[rng.random(x.shape) < 0.5] *= F32(-1)
            stride = w * w + 3
            src = torch.full((1 + members * stride,), 7.0, dtype=torch.float32, device="cuda")
            src[1:].view(members, stride)[:, :w * w] = torch.from_numpy(x.reshape(members, -1)).cuda()
            s, arena = arena_ensemble(n, members, storage)
            with s:
                what = "n=%d M=%d storage=%d" % (n, members, storage)
                s.unpack("dens", src[1:], member_stride=stride)              # base offset by one float, gaps between members
                want = h(x) if storage else x
                for m in range(members):
                    same_bits(s.download("dens", member=m), want[m], what + " member %d" % m)
                pads_are_zero(s, arena, what)
                # a sub-range, dense: the others keep what they had
                if members > 1:
                    y = (x[1:] * F32(0.5)).astype(F32)
                    s.unpack("dens", torch.from_numpy(y).cuda(), first=1)
                    same_bits(s.download("dens", member=0), want[0], what + " member 0 after a sub-range")
                    for m in range(1, members):
                        same_bits(s.download("dens", member=m), (h(y) if storage else y)[m - 1], what + " member %d of the sub-range" % m)
                    pads_are_zero(s, arena, what + " sub-range")


@pytest.mark.parametrize("whole", [True, False], ids=["all", "subrange"])
def test_unpack_against_operator_marks(oracle, whole):
    """test_gpu_ensemble.test_member_upload_against_operator_marks with an unpack: dens_prev zero by definition over stale
    memory, dens owing dt * (+0).  All members: the marks are gone with the old contents.  Member 1 alone: the other
    members hold the zeros / the increment."""
    torch = torch_()
    n, members = 30, 3
    a, b = oracle.coefficients(n, DT, DIFF)
    for target in ("dens_prev", "dens"):
        fields = [{k: np.full((n + 2, n + 2), -0.0, F32) for k in NAMES} for _ in range(members)]
        for f in fields:
            f["dens_prev"][...] = 0.75
        models = [Model(oracle, f) for f in fields]
        new = np.stack([rnd(np.random.default_rng(8 + m), n) for m in range(members)])
        with solver(n, members) as s:
            upload_all(s, fields)
            for op in (("divergence", "u", "v", "dens_prev", "v_prev"), ("add_source", "dens", "dens_prev", DT)):
                play_ensemble(s, models, op, target)
            if whole:
                s.unpack(target, torch.from_numpy(new).cuda())
                for m in range(members):
                    models[m].f[target][...] = new[m]
            else:
                s.unpack(target, torch.from_numpy(new[1:2].copy()).cuda(), first=1, count=1)
                models[1].f[target][...] = new[1]
            for op in (("diffuse", 0, "u_prev", "dens", a, b, 8), ("add_source", "u", "dens_prev", 0.5)):
                play_ensemble(s, models, op, target)
            compare_all(s, models, "unpack of %s, %s" % (target, "all members" if whole else "member 1"))


@pytest.mark.parametrize("whole", [True, False], ids=["all", "subrange"])
def test_unpack_against_scaled_fields_fp16(whole):
    """fp16 storage: a step leaves u_prev / v_prev multiplied by a power of two.  u_prev is unpacked -- all members, or
    member 1 alone -- and a sourced step reads it: each member equals a one-member fp16 context given the same calls with
    fluid_upload in the unpack's place."""
    from fluidsimulationcuda_amd import capi
    from oracle.oracle import Oracle
    torch = torch_()
    n, members, iters = 113, 3, 20
    fields = member_fields(Oracle(), n, members, seed=1, kinds=("parameters", "uniform", "parameters"))
    new = np.stack([rnd(np.random.default_rng(4 + m), n) for m in range(members)])

    def calls(s, put):
        s.step(1, use_sources=True, iters=iters)
        s.step(1, iters=iters)
        put(s)
        s.step(1, use_sources=True, iters=iters)

    def put_ensemble(s):
        if whole:
            s.unpack("u_prev", torch.from_numpy(new).cuda())
        else:
            s.unpack("u_prev", torch.from_numpy(new[1:2].copy()).cuda(), first=1, count=1)

    with solver(n, members, storage=capi.STORAGE_F16) as s:
        upload_all(s, fields)
        calls(s, put_ensemble)
        got = [{k: s.download(k, member=m) for k in NAMES} for m in range(members)]
    for m in range(members):
        with solver(n, 1, storage=capi.STORAGE_F16) as one:
            one.upload(**fields[m])
            calls(one, (lambda s: s.upload(u_prev=new[m])) if whole or m == 1 else (lambda s: None))
            for k in NAMES:
                same_bits(got[m][k], one.download(k), "member %d, %s" % (m, k))


def conversion_values():
    """every half widened, its float neighbours one ulp either side, every tie between adjacent halves, +-0, values that
    overflow to inf, 2^22 random bit patterns"""
    halves = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(F32)
    bits = halves.view(np.uint32)
    finite = np.arange(0x7C00, dtype=np.uint32).astype(np.uint16)            # +0 .. the largest finite half
    lo = finite.view(np.float16).astype(np.float64)
    hi = np.append(lo[1:], 65536.0)                                          # (the tie above 65504 rounds to inf)
    ties = ((lo + hi) / 2).astype(F32)
    assert ((lo + hi) / 2 == ties.astype(np.float64)).all()
    special = np.array([0.0, -0.0, 65504.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e5, 3.0e38, np.inf, 2.0 ** -24, 2.0 ** -25,
                        np.nextafter(F32(2.0 ** -25), F32(1)), 2.0 ** -26], F32)
    special = np.concatenate([special, -special, np.array([0x7FC00000, 0xFFC00000], np.uint32).view(F32)])
    rng = np.random.default_rng(2 ** 22)
    random = rng.integers(0, 1 << 32, size=1 << 22, dtype=np.uint64).astype(np.uint32).view(F32)
    return np.concatenate([np.array([0x7FC00000], np.uint32).view(F32), halves, (bits + 1).view(F32), (bits - 1).view(F32), ties, -ties,
                           special, random])


def test_unpack_narrows_like_numpy_and_like_upload_member():
    torch = torch_()
    vals = conversion_values()
    n = 1022
    cells = (n + 2) ** 2
    members = -(-vals.size // cells)
    dense = np.zeros(members * cells, F32)
    dense[:vals.size] = vals
    dense = dense.reshape(members, n + 2, n + 2)
    with np.errstate(all="ignore"):
        want = dense.astype(np.float16).view(np.uint16)
    s, arena = arena_ensemble(n, members, storage=1)
    with s:
        s.unpack("u", torch.from_numpy(dense).cuda())
        got = stored_bits(s, arena, "u").copy()
        nan = np.isnan(dense)
        assert nan.any() and (got[~nan] == want[~nan]).all(), "%d values are not numpy's float16 rounding" % int((got[~nan] != want[~nan]).sum())
        assert np.isnan(got[nan].view(np.float16)).all(), "a NaN did not stay a NaN"
        assert dense.view(np.uint32).ravel()[0] == 0x7FC00000 and got.ravel()[0] == 0x7E00
        pads_are_zero(s, arena, "conversion values")
        for m in range(members):
            s.upload(member=m, v=dense[m])
        host = stored_bits(s, arena, "v")
        assert np.array_equal(got, host), "%d stored values differ between the device's narrowing and fluid_upload_member's" % int((got != host).sum())


# ---- 3. beyond 4 GiB on the dense side ----------------------------------------------------------------------------------------
def test_dense_side_beyond_4_gib():
    torch = torch_()
    n, members, stride = 14, 1100, 2 ** 20 + 1
    cells = (n + 2) ** 2
    words = (members - 1) * stride + cells
    assert words * 4 > 1 << 32
    rng = np.random.default_rng(1100)
    x = rng.uniform(-1, 1, size=(members, n + 2, n + 2)).astype(F32)
    probes = (0, members // 2, members - 1)
    with solver(n, members) as s:
        s.upload_members(u=x)
        buf = sentinel_buffer(words)
        s.pack("u", out=buf.view(torch.float32), member_stride=stride)
        for m in probes:
            got = buf[m * stride:m * stride + cells + 1].cpu().numpy().view(np.uint32)
            assert np.array_equal(got[:cells], x[m].view(np.uint32).ravel()), "pack: member %d" % m
            assert m == members - 1 or got[cells] == SENTINEL
        y = (x * F32(0.5)).astype(F32)
        src = buf.view(torch.float32)
        for m in probes:
            src[m * stride:m * stride + cells] = torch.from_numpy(y[m].ravel()).cuda()
        s.unpack("v", src, member_stride=stride)
        for m in probes:
            same_bits(s.download("v", member=m), y[m], "unpack: member %d" % m)
        same_bits(s.download("v", member=1), x[1], "unpack: member 1 (what the pack left in the buffer)")


@pytest.mark.skipif(not os.environ.get("FLUID_HUGE_N"), reason="the 64-bit field index: N = 32800, 4.3 GB per field; set FLUID_HUGE_N")
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_field_side_beyond_32_bit_offsets(storage):
    torch = torch_()
    n = 32800
    w = n + 2
    with solver(n, 1, storage=storage) as s:
        src = torch.arange(w * w, dtype=torch.float32, device="cuda").remainder_(2039.0)
        s.unpack("u", src)
        out = s.pack("u")
        assert torch.equal(out.view(-1), src)
        row = s.download("u", member=0)[w - 1]
        assert np.array_equal(row, src[(w - 1) * w:].cpu().numpy())


# ---- 4. nothing is disturbed ----------------------------------------------------------------------------------------------------
def insert_packs(rng, ops):
    ops = list(ops)
    for _ in range(int(rng.integers(3, 9))):
        ops.insert(int(rng.integers(0, len(ops) + 1)), ("x_pack", NAMES[rng.integers(6)], int(rng.integers(4))))
    return ops


def run_sequence(oracle, n, members, params, fields, ops, what, models):
    with solver(n, members, params=params) as s:
        s.timing_enable(True)
        upload_all(s, fields)
        s.timing_read(reset=True)
        for op in ops:
            if op[0] == "x_pack":
                first = op[2] % members
                s.pack(op[1], first=first, count=0 if op[2] & 1 else 1)
            elif op[0] == "upload_member":
                s.upload(member=op[1], **{op[2]: op[3]})
                if models:
                    models[op[1]].f[op[2]][...] = op[3]
            elif op[0] == "download_member":
                got = s.download(op[2], member=op[1])
                if models:
                    same_bits(got, models[op[1]].f[op[2]], "%r -- %s" % (op[:3], what))
            elif models:
                play_ensemble(s, models, op, what)
            else:
                play(s, None, op, what)
        if models:
            compare_all(s, models, what)
        t = s.timing_read(reset=True)
        return [[s.download(k, member=m) for k in NAMES] for m in range(members)], {k: t[k] for k in COUNTERS}


@pytest.mark.parametrize("seed", range(16))
def test_packs_disturb_nothing(oracle, seed):
    from fluidsimulationcuda_amd import capi
    rng = np.random.default_rng(17000 + seed)
    n = int(rng.choice([1, 2, 3, 5, 8, 13, 31, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 200, 255, 256, 257]))
    members = int(rng.choice([1, 2, 3, 5]))
    params = {capi.PARAM_TB_T16_MIN_CELLS: int(rng.choice([0, -1]))}
    fields = [draw_fields(rng, n) for _ in range(members)]
    plain = []
    for op in ensemble_ops(rng, draw_sequence(rng, oracle, n), n, members):
        if op[0] == "upload_member":        # the array goes into the op, so that both runs upload the same one
            host = rng.choice(COARSE, size=(n + 2, n + 2)).astype(F32) if op[3] else np.full((n + 2, n + 2), op[3], F32)
            op = op[:3] + (host,)
        plain.append(op)
    ops = insert_packs(rng, plain)
    what = "seed %d n=%d M=%d %r: %r" % (seed, n, members, params, [op[:3] for op in ops])
    got, counts = run_sequence(oracle, n, members, params, fields, ops, what, [Model(oracle, f) for f in fields])
    ref, ref_counts = run_sequence(oracle, n, members, params, fields, plain, what, None)
    for m in range(members):
        for k, name in enumerate(NAMES):
            same_bits(got[m][k], ref[m][k], "member %d %s against the sequence without the packs -- %s" % (m, name, what))
    assert counts == ref_counts, what


# ---- 5. bulk host calls -------------------------------------------------------------------------------------------------------
def mem_free():
    hip = hip_runtime()
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def bulk_against_the_loop(n, members, storage, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, size=(members, n + 2, n + 2)).astype(F32)
    with solver(n, members, storage=storage) as s, solver(n, members, storage=storage) as loop:
        s.upload_members(dens=x)
        for m in range(members):
            loop.upload(member=m, dens=x[m])
        got = s.download_members("dens")
        for m in range(members):
            want = loop.download("dens", member=m)
            same_bits(s.download("dens", member=m), want, "upload_members, member %d" % m)
            same_bits(got[m], want, "download_members, member %d" % m)
        # a lazy field through the bulk download: zero by definition, and what an fp16 step keeps scaled
        s.step(2, iters=4)
        loop.step(2, iters=4)
        for k in ("u_prev", "dens_prev"):
            got = s.download_members(k)
            for m in range(members):
                same_bits(got[m], loop.download(k, member=m), "download_members(%s), member %d" % (k, m))


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n, members", [(1, 1), (14, 5), (61, 16), (129, 3), (4094, 2)])
def test_bulk_host_calls_equal_the_member_loop(n, members, storage):
    """(4094, 2): one member fills the 64 MiB staging buffer (4096^2 floats), so the call moves two groups through it"""
    bulk_against_the_loop(n, members, storage, seed=n + members)


def test_destroy_frees_the_staging_buffer():
    """N = 4094: the staging buffer is one member, 64 MiB.  hipMemGetInfo before the context, after the first bulk call and
    after fluid_destroy.  Slack: 16 MiB, a quarter of the buffer; the idle variation -- five readings in a row with nothing
    in between -- is printed beside it (0 on an otherwise idle device; the runtime hands memory out in 2 MiB granules)."""
    n, members, slack = 4094, 1, 16 << 20
    stage = (n + 2) ** 2 * 4
    with solver(14, 2) as warm:              # whatever the runtime sets up at the first such calls is set up now
        warm.upload_members(u=np.ones((2, 16, 16), F32))
    torch_().cuda.synchronize()
    idle = [mem_free() for _ in range(5)]
    print("idle variation of hipMemGetInfo: %d bytes; slack %d bytes; staging buffer %d bytes" % (max(idle) - min(idle), slack, stage))
    before = mem_free()
    s = solver(n, members)
    created = mem_free()
    s.upload_members(u=np.ones((members, n + 2, n + 2), F32))
    staged = mem_free()
    s.close()
    after = mem_free()
    print("free: before %d, context %d, staged %d, destroyed %d" % (before, created, staged, after))
    assert created - staged >= stage - slack, "no staging buffer was allocated?"
    assert abs(after - before) <= slack, "fluid_destroy left %d bytes behind" % (before - after)


# ---- 6. run -----------------------------------------------------------------------------------------------------------------
RUN_FIELDS = ("u", "v", "dens", "u_prev")
RUN_CASES = [(14, 4), (61, 4), (129, 4), (97, 40), (510, 40)]
NSTEPS, EVERY = 5, 2


def run_params(iters):
    from fluidsimulationcuda_amd import capi
    # 40 sweeps: the parameters with which test_gpu_step sees the sources added inside the first diffusion launch
    return {capi.PARAM_TB_MIN_CELLS: 0, capi.PARAM_TB_T16_MIN_CELLS: 0} if iters == 40 else None


def sources_for(n, members, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([rnd(rng, n) for _ in range(members)]) for _ in range(3)])       # (3, M, W, W)


def step_by_step(s, iters, sources, models=None, use_sources=False, dt=DT, diff=DIFF, visc=VISC):
    """the loop fluid_run is defined as, call by call; snapshots through fluid_download_member.  With models: the oracle
    per member beside it, the sources supplied afresh before every step."""
    torch = torch_()
    snaps = []
    dev = torch.from_numpy(sources).cuda() if sources is not None else None
    for z in range(NSTEPS):
        if dev is not None:
            for k, name in enumerate(("u_prev", "v_prev", "dens_prev")):
                s.unpack(name, dev[k])
        s.step(1, use_sources=dev is not None or (use_sources and z == 0), dt=dt, diff=diff, visc=visc, iters=iters)
        for m, mod in enumerate(models or ()):
            if sources is not None:
                for k, name in enumerate(("u_prev", "v_prev", "dens_prev")):
                    mod.f[name][...] = sources[k][m]
            mod.step(sources is not None or (use_sources and z == 0), DT, DIFF, VISC, iters)
        if (z + 1) % EVERY == 0:
            snaps.append([[s.download(f, member=m) for m in range(s.members)] for f in RUN_FIELDS])
            for m, mod in enumerate(models or ()):
                for k, f in enumerate(RUN_FIELDS):
                    same_bits(snaps[-1][k][m], mod.f[f], "call by call against the oracle: step %d %s member %d" % (z + 1, f, m))
    return snaps, [[s.download(f, member=m) for f in NAMES] for m in range(s.members)]


def check_run(got, written, final, want_snaps, want_final, what):
    assert written == len(want_snaps) == NSTEPS // EVERY and tuple(got.shape[:2]) == (written, len(RUN_FIELDS))
    got = got.cpu().numpy()
    for k, snap in enumerate(want_snaps):
        for f, name in enumerate(RUN_FIELDS):
            for m, want in enumerate(snap[f]):
                same_bits(got[k, f, m], want, "%s: snapshot %d %s member %d" % (what, k, name, m))
    for m, fields in enumerate(want_final):
        for k, name in enumerate(NAMES):
            same_bits(final[m][k], fields[k], "%s: final %s member %d" % (what, name, m))


@pytest.mark.parametrize("forced", [False, True], ids=["plain", "forced"])
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n, iters", RUN_CASES)
def test_run_equals_the_loop_of_calls(oracle, n, iters, storage, forced):
    """(a), (b), (d): snapshots and final fields of run() against the call-by-call twin context, and (fp32) the oracle"""
    torch = torch_()
    members = 3
    fields = member_fields(oracle, n, members, seed=n, kinds=("parameters", "uniform", "coarse"))
    sources = sources_for(n, members, n) if forced else None
    what = "n=%d iters=%d storage=%d forced=%d" % (n, iters, storage, forced)
    with solver(n, members, storage=storage, params=run_params(iters)) as twin:
        upload_all(twin, fields)
        models = [Model(oracle, f) for f in fields] if storage == 0 else None
        want_snaps, want_final = step_by_step(twin, iters, sources, models, use_sources=True)
    with solver(n, members, storage=storage, params=run_params(iters)) as s:
        upload_all(s, fields)
        s.timing_enable(True)
        s.timing_read(reset=True)
        got, written = s.run(NSTEPS, every=EVERY, fields=RUN_FIELDS, sources=None if sources is None else torch.from_numpy(sources).cuda(),
                             iters=iters, use_sources=True)
        t = s.timing_read(reset=True)
        if forced and iters == 40:
            assert t["source_calls"] == 0, "the sourced steps of a run left the source-adding first launch: %r" % (t,)
        final = [[s.download(f, member=m) for f in NAMES] for m in range(members)]
    check_run(got, written, final, want_snaps, want_final, what)


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_run_members_against_one_member_contexts(oracle, storage):
    """(c): distinct dt / diff / visc per member"""
    torch = torch_()
    n, iters, members = 61, 4, 3
    dt, diff, visc = [0.016, 0.008, 0.03], [0.1, 0.0, 0.02], [0.0025, 0.01, 0.0]
    fields = member_fields(oracle, n, members, seed=5, kinds=("parameters", "uniform", "coarse"))
    sources = sources_for(n, members, 61)
    with solver(n, members, storage=storage) as s:
        upload_all(s, fields)
        got, written = s.run(NSTEPS, every=EVERY, fields=RUN_FIELDS, sources=torch.from_numpy(sources).cuda(), iters=iters, dt=dt, diff=diff, visc=visc)
        final = [[s.download(f, member=m) for f in NAMES] for m in range(members)]
    for m in range(members):
        with solver(n, 1, storage=storage) as one:
            one.upload(**fields[m])
            snaps, last = step_by_step(one, iters, sources[:, m:m + 1].copy(), dt=dt[m], diff=diff[m], visc=visc[m])
        check_run(got[:, :, m:m + 1], written, final[m:m + 1], snaps, last, "member %d alone" % m)


def test_run_that_records_nothing(oracle):
    """(e): every = 0, nsteps = 0, every > nsteps"""
    torch = torch_()
    n, members, iters = 14, 3, 4
    fields = member_fields(oracle, n, members, seed=2, kinds=("uniform", "coarse"))
    for nsteps, every in ((3, 0), (0, 2), (3, 4)):
        models = [Model(oracle, f) for f in fields]
        with solver(n, members) as s:
            upload_all(s, fields)
            out = sentinel_buffer(4 * members * (n + 2) ** 2)
            got, written = s.run(nsteps, every=every, fields=("u", "dens") if every else (), out=out.view(torch.float32) if every else None,
                                 iters=iters, use_sources=True)
            assert written == 0 and (got is None) == (every == 0)
            assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all(), "nsteps=%d every=%d wrote a snapshot" % (nsteps, every)
            for z in range(nsteps):
                for mod in models:
                    mod.step(z == 0, DT, DIFF, VISC, iters)
            compare_all(s, models, "nsteps=%d every=%d" % (nsteps, every))


def test_run_nan_member_stays_alone(oracle):
    """(f)"""
    torch = torch_()
    n, members, iters = 61, 3, 4
    fields = member_fields(oracle, n, members, seed=7, kinds=("parameters", "uniform", "coarse"))
    sources = sources_for(n, members, 7)
    bad_fields = [dict(f) for f in fields]
    bad_fields[1] = {k: np.full((n + 2, n + 2), np.nan, F32) for k in NAMES}
    bad_sources = sources.copy()
    bad_sources[:, 1] = np.nan
    shots = []
    for f, src in ((fields, sources), (bad_fields, bad_sources)):
        with solver(n, members) as s:
            upload_all(s, f)
            got, written = s.run(NSTEPS, every=1, fields=NAMES, sources=torch.from_numpy(src).cuda(), iters=iters)
            assert written == NSTEPS
            shots.append(got.cpu().numpy())
    assert np.isnan(shots[1][:, :, 1]).all()
    for m in (0, 2):
        same_bits(shots[1][:, :, m], shots[0][:, :, m], "member %d beside a member full of NaN" % m)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(oracle):
    from fluidsimulationcuda_amd import capi
    import fluidsimulationcuda_amd as F
    torch = torch_()
    hip = hip_runtime()
    n, members = 30, 5
    cells = (n + 2) ** 2
    L = capi.lib()
    fields = member_fields(oracle, n, members, seed=2, kinds=("uniform", "coarse"))
    good = np.linspace(0.5, 1.5, members).astype(F32)
    host = np.zeros((members, n + 2, n + 2), F32)
    dev = torch.zeros(4 * members * cells, dtype=torch.float32, device="cuda")     # two snapshots of two fields
    ids = (C.c_int * 2)(0, 2)
    bad_ids = (C.c_int * 2)(0, 12)
    written = C.c_int(-7)
    exact = C.c_void_p()
    assert hip.hipMalloc(C.byref(exact), C.c_size_t(1 << 20)) == 0
    edge = exact.value + (1 << 20) - 1024           # device memory whose allocation ends 1024 bytes further on

    def mf(a):
        return a.ctypes.data_as(capi._MF)

    def plan(**kw):
        p = dict(iters=4, nsteps=4, use_sources=0, sources=None, every=2, fields=ids, nfields=2, snapshots=dev.data_ptr(), capacity=dev.numel())
        p.update(kw)
        return C.byref(capi.RunPlan(**p))

    def run(**kw):
        return lambda: L.fluid_run(hnd, DT, DIFF, VISC, plan(**kw), C.byref(written))

    def run_m(dt=None, **kw):
        dt = good if dt is None else dt
        return lambda: L.fluid_run_members(hnd, mf(dt), mf(good), mf(good), plan(**kw), C.byref(written))

    nan_dt = good.copy()
    nan_dt[3] = np.nan
    try:
        with solver(n, members) as s:
            upload_all(s, fields)
            s.computeDivergenceAndPressure("u", "v", "u_prev", "v_prev")        # a lazy state that must survive the refusals
            s.add_source("dens", "u_prev", DT)
            hnd, d = s._h, dev.data_ptr()
            refused = [
                ("fluid_pack_members", lambda: L.fluid_pack_members(hnd, 0, 0, 0, None, 0), b"dst_dev"),
                ("fluid_pack_members", lambda: L.fluid_pack_members(hnd, 12, 0, 0, d, 0), b"12"),
                ("fluid_pack_members", lambda: L.fluid_pack_members(hnd, -1, 0, 0, d, 0), b"-1"),
                ("fluid_pack_members", lambda: L.fluid_pack_members(hnd, 0, -1, 0, d, 0), b"first -1"),
                ("fluid_pack_members", lambda: L.fluid_pack_members(hnd, 0, 6, 0, d, 0), b"first 6"),
                ("fluid_pack_members", lambda: L.fluid_pack_members(hnd, 0, 2, 4, d, 0), b"count 4"),
                ("fluid_pack_members", lambda: L.fluid_pack_members(hnd, 0, 0, -2, d, 0), b"count -2"),
                ("fluid_pack_members", lambda: L.fluid_pack_members(hnd, 0, 0, 0, d, cells - 1), b"member_stride"),
                ("fluid_pack_members", lambda: L.fluid_pack_members(hnd, 0, 0, 0, host.ctypes.data, 0), b"not device memory"),
                ("fluid_pack_members", lambda: L.fluid_pack_members(hnd, 0, 0, 0, edge, 0), b"allocation ends"),
                ("fluid_pack_members", lambda: L.fluid_pack_members(hnd, 0, 0, 0, d, 1 << 40), b"allocation ends"),
                ("fluid_unpack_members", lambda: L.fluid_unpack_members(hnd, 0, 0, 0, None, 0), b"src_dev"),
                ("fluid_unpack_members", lambda: L.fluid_unpack_members(hnd, 99, 0, 0, d, 0), b"99"),
                ("fluid_unpack_members", lambda: L.fluid_unpack_members(hnd, 0, 5, 1, d, 0), b"count 1"),
                ("fluid_unpack_members", lambda: L.fluid_unpack_members(hnd, 0, 0, 0, d, 17), b"member_stride"),
                ("fluid_unpack_members", lambda: L.fluid_unpack_members(hnd, 0, 0, 0, host.ctypes.data, 0), b"not device memory"),
                ("fluid_unpack_members", lambda: L.fluid_unpack_members(hnd, 0, 0, 0, edge, 0), b"allocation ends"),
                ("fluid_download_members", lambda: L.fluid_download_members(hnd, 0, None), b"null host pointer"),
                ("fluid_download_members", lambda: L.fluid_download_members(hnd, 12, mf(host)), b"12"),
                ("fluid_upload_members", lambda: L.fluid_upload_members(hnd, 0, None), b"null host pointer"),
                ("fluid_upload_members", lambda: L.fluid_upload_members(hnd, -3, mf(host)), b"-3"),
                ("fluid_run", lambda: L.fluid_run(hnd, DT, DIFF, VISC, None, None), b"null plan"),
                ("fluid_run", run(iters=3), b"sweep count"),
                ("fluid_run", run(iters=-2), b"sweep count"),
                ("fluid_run", run(nsteps=-1), b"nsteps"),
                ("fluid_run", run(every=-1), b"every"),
                ("fluid_run", run(nfields=0), b"nfields"),
                ("fluid_run", run(nfields=13), b"nfields"),
                ("fluid_run", run(fields=None), b"fields"),
                ("fluid_run", run(fields=bad_ids), b"12"),
                ("fluid_run", run(snapshots=None), b"snapshots"),
                ("fluid_run", run(capacity=2 * 2 * members * cells - 1), b"capacity"),
                ("fluid_run", run(snapshots=host.ctypes.data), b"not device memory"),
                ("fluid_run", run(snapshots=edge), b"allocation ends"),
                ("fluid_run", run(sources=host.ctypes.data), b"not device memory"),
                ("fluid_run", run(sources=edge), b"allocation ends"),
                ("fluid_run_members", lambda: L.fluid_run_members(hnd, mf(good), mf(good), mf(good), None, None), b"null plan"),
                ("fluid_run_members", lambda: L.fluid_run_members(hnd, mf(good), None, mf(good), plan(), None), b"diff"),
                ("fluid_run_members", run_m(dt=nan_dt), b"member 3"),
                ("fluid_run_members", run_m(iters=5), b"sweep count"),
                ("fluid_run_members", run_m(sources=edge), b"allocation ends"),
            ]
            for name, call, word in refused:
                L.fluid_synchronize(None)               # (an unrelated message in between)
                assert call() == capi.E_INVALID, (name, word)
                msg = L.fluid_last_error()
                assert name.encode() in msg and word in msg, (name, word, msg)
            assert written.value == -7 and not dev.any().item()
            models = [Model(oracle, f) for f in fields]
            for mod in models:
                mod.o.divergence(mod.f["u"], mod.f["v"], mod.f["u_prev"], mod.f["v_prev"])
                mod.o.add_source(mod.f["dens"], mod.f["u_prev"], DT)
            compare_all(s, models, "after the refusals")
        # row slabs: all six calls refused
        with F.FluidSolver(n, rank=0, nranks=2) as s:
            hnd, d = s._h, dev.data_ptr()
            one = (C.c_float * 1)(0.5)
            for name, call in (("fluid_pack_members", lambda: L.fluid_pack_members(hnd, 0, 0, 0, d, 0)),
                               ("fluid_unpack_members", lambda: L.fluid_unpack_members(hnd, 0, 0, 0, d, 0)),
                               ("fluid_download_members", lambda: L.fluid_download_members(hnd, 0, mf(host))),
                               ("fluid_upload_members", lambda: L.fluid_upload_members(hnd, 0, mf(host))),
                               ("fluid_run", run()),
                               ("fluid_run_members", lambda: L.fluid_run_members(hnd, one, one, one, plan(), None))):
                assert call() == capi.E_INVALID, name
                msg = L.fluid_last_error()
                assert name.encode() in msg and b"slab" in msg, (name, msg)
    finally:
        assert hip.hipFree(exact) == 0


def test_one_member_context_and_plain_addresses(oracle):
    """M = 1 on an ordinary context; a buffer given as a plain integer address and as a __cuda_array_interface__"""
    torch = torch_()
    import fluidsimulationcuda_amd as F
    n = 14
    fields = member_fields(oracle, n, 1, seed=9, kinds=("uniform",))[0]

    class Cai:
        def __init__(self, t):
            self.t = t
            self.__cuda_array_interface__ = {"data": (t.data_ptr(), False), "shape": tuple(t.shape), "typestr": "<f4", "version": 2}

    with F.FluidSolver(n) as s:
        s.upload(**fields)
        out = torch.zeros((1, n + 2, n + 2), dtype=torch.float32, device="cuda")
        s.pack("u", out=out.data_ptr())
        same_bits(out[0].cpu().numpy(), fields["u"], "pack into an integer address")
        s.unpack("v", Cai(out))
        same_bits(s.download("v"), fields["u"], "unpack from a __cuda_array_interface__")
        snaps = torch.zeros((2, 1, 1, n + 2, n + 2), dtype=torch.float32, device="cuda")
        got, written = s.run(2, every=1, fields=("dens",), out=Cai(snaps), iters=4)
        assert written == 2 and got.t is snaps
        same_bits(snaps[1, 0, 0].cpu().numpy(), s.download("dens"), "the last snapshot of a one-member run")
        same_bits(s.download_members("u")[0], s.download("u"), "download_members on one member")
