"""GPU: the ensemble noise -- fluid_noise_members / fluid_noise_dense (include/fluid_amd.h, "ensemble noise"): approximately
normal noise of a counter-based generator set into or added to the members of a field in place, and written to a dense
device array.

Every expected value comes from tests/noise_model.py, the header's definition in numpy, applied -- for FLUID_NOISE_ADD -- to
what download_members (the pack) showed before the call.  Everything is compared bit for bit, in every cell of every
member of every listed field; a NaN is a NaN, its sign and payload are not compared.  There is no tolerance anywhere.

Shapes (W = N + 2; a lane takes 4 columns, vector 0 is ghost column 0 alone): N = 1 is the ghost ring and one cell; N = 6 a
single masked vector behind vector 0; N = 30 an even W, N = 61 an odd one with both edge vectors masked; N = 254 has more
than one wave per row; M = 70 is past the 64 members the transforms stop at."""
import ctypes as C

import numpy as np
import pytest

from noise_model import ADD, SET, noise_add, noise_dense, noise_set
from relax_model import F32, narrow
from test_gpu_relax import (DT, MAIN, F, arena_ensemble, hip_runtime, ints, pads_of, plant_pads, random_values, same, same_bits,
                            scaled_slot, shown, slot_values, solver, stored_bits, torch_)

pytestmark = pytest.mark.gpu
SHAPES = [(1, 2), (6, 3), (30, 3), (61, 5), (254, 2), (14, 70)]          # (N, M)
SEED = 0x0123456789ABCDEF
ID = {name: k for k, name in enumerate(("u", "v", "dens", "u_prev", "v_prev", "dens_prev"))}


def floats(*v):
    return (C.c_float * len(v))(*v)


def amplitudes(rng, members, storage):
    a = rng.uniform(0.25, 2.0, members) * rng.choice([-1.0, 1.0], members)
    return a.astype(F32)


# ---- 1. both modes against the model, every cell of every member of every listed field; pads and other fields keep their bits -----
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n,members", SHAPES, ids=["n%d-m%d" % nm for nm in SHAPES])
def test_set_and_add_are_the_model_in_every_cell(n, members, storage):
    rng = np.random.default_rng(1000 * storage + 10 * n + members)
    w = n + 2
    what = "n=%d M=%d storage=%d" % (n, members, storage)
    s, arena = arena_ensemble(n, members, storage)
    with s:
        s.upload_members(**{f: random_values(rng, (members, w, w), storage) for f in MAIN})
        for f in MAIN:
            plant_pads(s, arena, f)
        amp = amplitudes(rng, members, storage)
        for mode, listed, sequence in ((SET, ("u", "dens_prev"), 7), (ADD, ("v", "u"), 8), (SET, ("u", "dens_prev"), 7)):
            before = {f: shown(s, f) for f in listed}
            raw = {f: stored_bits(s, arena, f) for f in MAIN}
            s.noise(listed, amp, SEED, sequence, mode)
            for f in listed:
                if mode == SET:
                    want = noise_set(w, members, amp, SEED, sequence, ID[f], storage)
                else:
                    want = noise_add(before[f], amp, SEED, sequence, ID[f], storage)
                same(shown(s, f), want, "%s: mode %d of %s" % (what, mode, f))
            for f in MAIN:
                got = stored_bits(s, arena, f)
                same_bits(pads_of(got, n), pads_of(raw[f], n), "%s: mode %d, the pads of %s" % (what, mode, f))
                if f not in listed:
                    same_bits(got, raw[f], "%s: mode %d, %s was not listed" % (what, mode, f))
        # (the third round repeated the first: the same arguments gave the same bits, over a field that held other values)
        # a scalar amplitude is that amplitude for every member
        s.noise("dens", 0.5, SEED, 9, "set")
        same(shown(s, "dens"), noise_set(w, members, 0.5, SEED, 9, ID["dens"], storage), what + ": scalar amplitude")


# ---- 2. the lazy state: SET drops what the field owed itself, ADD settles it first ---------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("case", ["source", "zero source"])
def test_set_drops_the_debt_and_add_settles_it(case, storage):
    rng = np.random.default_rng(2000 + storage)
    n, members = 30, 3
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    amp = amplitudes(rng, members, storage)

    def prepared():
        s = solver(n, members, storage)
        s.upload_members(**fields)
        if case == "zero source":
            s.step(use_sources=True)
            s.computeDivergenceAndPressure("u", "v", "dens_prev", "tmp0")       # its pressure is zero by definition: marked, not written
        s.add_source("dens", "dens_prev", DT)                                   # deferred: dens owes itself the increment
        return s

    what = "%s storage=%d" % (case, storage)
    with prepared() as a, prepared() as b, prepared() as c:
        before = shown(b, "dens")                                               # the twin: the calls never ran there
        if case == "source":
            assert not np.array_equal(before, narrow(fields["dens"], storage)), "the source does something"
        a.noise(("dens",), amp, SEED, 1, SET)
        same(shown(a, "dens"), noise_set(w, members, amp, SEED, 1, ID["dens"], storage), what + ": SET replaces the field, debt included")
        c.noise(("dens",), amp, SEED, 1, ADD)
        same(shown(c, "dens"), noise_add(before, amp, SEED, 1, ID["dens"], storage), what + ": ADD on the settled field")
        for f in MAIN:
            if f != "dens":
                same_bits(shown(a, f), shown(b, f), "%s: %s was not listed (SET)" % (what, f))
                same_bits(shown(c, f), shown(b, f), "%s: %s was not listed (ADD)" % (what, f))
        if case == "zero source":
            # dens_prev is all +0 by a mark alone: SET writes the field, the mark is gone
            a.noise(("dens_prev",), amp, SEED, 2, SET)
            same(shown(a, "dens_prev"), noise_set(w, members, amp, SEED, 2, ID["dens_prev"], storage), what + ": SET over a marked field")
            c.noise(("dens_prev",), amp, SEED, 2, ADD)
            same(shown(c, "dens_prev"), noise_add(np.zeros((members, w, w), F32), amp, SEED, 2, ID["dens_prev"], storage),
                 what + ": ADD to a marked field")
        for s in (a, c):                                                          # and the fields go on stepping
            s.step()
            for f in ("u", "v", "dens"):
                assert np.isfinite(shown(s, f)).all(), "%s: %s a step later" % (what, f)


# ---- 3. an fp16 field held at a pressure scale: ADD keeps the scale --------------------------------------------------------------
@pytest.mark.parametrize("members", [2, 5])
def test_add_keeps_the_pressure_scale_of_an_fp16_field(members):
    rng = np.random.default_rng(3000 + members)
    n = 30                                         # (the library scales the pressure from N = 16 on)
    w = n + 2
    what = "n=%d M=%d" % (n, members)
    s, arena = arena_ensemble(n, members, 1)
    with s:
        s.upload_members(**{f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN})
        s.step(use_sources=True)                   # fp16 storage: u_prev now holds the pressure, scaled
        before = shown(s, "u_prev")
        slot, scale = scaled_slot(s, arena, before)
        assert scale not in (None, 1.0), "%s: u_prev is not held at a scale other than 1 (%s)" % (what, scale)
        raw = slot_values(s, arena, slot)
        amp = (np.abs(before).max() * amplitudes(rng, members, 1)).astype(F32)
        amp[1] = 0.0
        s.noise(("u_prev",), amp, SEED, 4, ADD)
        want = noise_add(before, amp, SEED, 4, ID["u_prev"], 1)
        after = shown(s, "u_prev")
        same(after, want, what + ": the pack shows narrow(y)")
        stored = np.arange(members) != 1                       # (member 1 keeps what it showed, which need not be a half)
        assert np.array_equal(narrow(after[stored], 1), after[stored]), what
        held = slot_values(s, arena, slot)
        same(held, after * F32(scale), what + ": the field is still held at its scale")
        same_bits(held[1], raw[1], what + ": the member with amplitude 0 keeps its stored bits")
        assert (after[0] != before[0]).mean() > 0.9, what
        s.step(use_sources=True)
        for f in ("u", "v", "dens"):
            assert np.isfinite(shown(s, f)).all(), "%s: %s a step later" % (what, f)


# ---- 4. ADD: amplitude 0 of either sign keeps -0 and NaN bits; a non-finite x stays non-finite in its own cell -------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_add_with_amplitude_zero_keeps_every_bit(storage):
    rng = np.random.default_rng(4000 + storage)
    n, members = 14, 4
    w = n + 2
    what = "storage=%d" % storage
    s, arena = arena_ensemble(n, members, storage)
    with s:
        x = random_values(rng, (members, w, w), storage)
        x[:, 2, 3] = -0.0
        x[:, 0, 0] = -0.0
        x[:, 5, 5].view(np.uint32)[:] = 0x7FC12345 if not storage else 0x7FC12000       # a NaN with a payload (a half keeps 10 bits of it)
        x[:, 6, 1] = np.inf
        x[:, 1, w - 1] = -np.inf
        s.upload_members(dens=x)
        plant_pads(s, arena, "dens")
        raw = stored_bits(s, arena, "dens")
        before = shown(s, "dens")
        amp = np.array([0.0, -0.0, 1.5, -0.75], F32)
        s.noise(("dens",), amp, SEED, 11, ADD)
        got = stored_bits(s, arena, "dens")
        same_bits(got[:2], raw[:2], what + ": members with amplitude +0 and -0")
        same_bits(pads_of(got, n), pads_of(raw, n), what + ": the pads")
        after = shown(s, "dens")
        same(after, noise_add(before, amp, SEED, 11, ID["dens"], storage), what)
        assert np.signbit(after[:2, 2, 3]).all() and np.isnan(after[:, 5, 5]).all(), what
        assert (after[2:, 6, 1] == np.inf).all() and (after[2:, 1, w - 1] == -np.inf).all(), what
        special = np.zeros((w, w), bool)
        special[5, 5] = special[6, 1] = special[1, w - 1] = True
        assert np.isfinite(after[:, ~special]).all(), what + ": a non-finite value stays in its own cell"
        # all members at amplitude 0: nothing is stored at all
        raw = stored_bits(s, arena, "dens")
        s.noise(("dens",), 0.0, SEED, 12, ADD)
        same_bits(stored_bits(s, arena, "dens"), raw, what + ": every amplitude 0")


# ---- 5. splitting an ensemble over contexts is exact; sequence, seed halves and field id all matter ------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_splitting_is_exact(storage):
    rng = np.random.default_rng(5000 + storage)
    n = 14
    w = n + 2
    x = random_values(rng, (5, w, w), storage)
    amp = amplitudes(rng, 5, storage)
    got = {}
    with solver(n, 5, storage) as s:
        s.upload_members(v=x)
        s.noise(("u",), amp, SEED, 3, SET)
        s.noise(("v",), amp, SEED, 3, ADD)
        got = {f: shown(s, f) for f in ("u", "v")}
    same(got["u"], noise_set(w, 5, amp, SEED, 3, ID["u"], storage), "the whole ensemble, SET")
    same(got["v"], noise_add(x, amp, SEED, 3, ID["v"], storage), "the whole ensemble, ADD")
    for first, count in ((0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (2, 3)):
        with solver(n, count, storage) as s:
            s.upload_members(v=x[first:first + count])
            s.noise(("u",), amp[first:first + count], SEED, 3, SET, member_offset=first)
            s.noise(("v",), amp[first:first + count], SEED, 3, ADD, member_offset=first)
            same_bits(shown(s, "u"), got["u"][first:first + count], "SET: %d member(s) at offset %d" % (count, first))
            same_bits(shown(s, "v"), got["v"][first:first + count], "ADD: %d member(s) at offset %d" % (count, first))
    # the last legal offset
    with solver(n, 3, storage) as s:
        s.noise(("u",), 1.0, SEED, 3, SET, member_offset=65533)
        same(shown(s, "u"), noise_set(w, 3, 1.0, SEED, 3, ID["u"], storage, member_offset=65533), "member ids 65533 .. 65535")


def test_sequence_seed_halves_and_field_id_all_matter():
    n, members = 14, 3
    w = n + 2
    cases = {"base": (SEED, 3, "u"), "sequence": (SEED, 4, "u"), "seed, low half": (SEED ^ 1, 3, "u"),
             "seed, high half": (SEED ^ (1 << 32), 3, "u"), "field": (SEED, 3, "v"), "seed halves swapped": (((SEED & 0xFFFFFFFF) << 32) | (SEED >> 32), 3, "u")}
    got = {}
    with solver(n, members) as s:
        for name, (seed, sequence, field) in cases.items():
            s.noise((field,), 1.0, seed, sequence, SET)
            got[name] = shown(s, field)
            same(got[name], noise_set(w, members, 1.0, seed, sequence, ID[field]), name)
        s.noise(("u",), 1.0, SEED, 3, SET)
        same_bits(shown(s, "u"), got["base"], "the same arguments, the same bits")
    names = list(cases)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert (got[a] != got[b]).mean() > 0.99, (a, b)
    assert (got["base"][0] != got["base"][1]).mean() > 0.99                       # ... and so does the member


# ---- 6. fluid_noise_dense ------------------------------------------------------------------------------------------------------
def test_noise_dense():
    torch = torch_()
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    hip = hip_runtime()
    exact = C.c_void_p()
    size = 1 << 16
    assert hip.hipMalloc(C.byref(exact), C.c_size_t(size)) == 0
    try:
        with solver(6, 2) as s:
            for count in (0, 1, 63, 64, 65, 4097):
                for stream_id, amplitude, sequence in ((0, 1.0, 0), (9, -2.5, 6)):
                    buf = torch.full((count + 16,), 123.25, dtype=torch.float32, device="cuda")
                    out = s.noise_dense(buf, amplitude, SEED, sequence, stream_id, count=count)
                    assert out is buf
                    got = buf.cpu().numpy()
                    same_bits(got[:count], noise_dense(count, amplitude, SEED, sequence, stream_id), "count %d, stream %d" % (count, stream_id))
                    assert (got[count:] == 123.25).all(), "count %d: the floats behind it" % count
            buf = torch.zeros(65, dtype=torch.float32, device="cuda")
            s.noise_dense(buf, 1.0, SEED, 1, 65535)                                  # the whole buffer, the last stream
            same_bits(buf.cpu().numpy(), noise_dense(65, 1.0, SEED, 1, 65535), "count None")
            a, b = noise_dense(4097, 1.0, SEED, 0, 0), noise_dense(4097, 1.0, SEED, 0, 9)
            assert (a != b).mean() > 0.99
            # a field cell never shares a counter with a dense float: tag 15 is no field id
            assert capi.NOISE_DENSE_TAG >= capi.NFIELDS
            # refusals: nothing is written
            hnd = s._h
            fits = exact.value + size - 4 * 64                                       # 64 floats that end with their allocation
            host = np.ones(64, F32)
            refused = [
                (lambda: L.fluid_noise_dense(hnd, None, 4, 1.0, 1, 0, 0), (b"out_dev",)),
                (lambda: L.fluid_noise_dense(None, buf.data_ptr(), 4, 1.0, 1, 0, 0), (b"null context",)),
                (lambda: L.fluid_noise_dense(hnd, buf.data_ptr(), 4, float("nan"), 1, 0, 0), (b"amplitude",)),
                (lambda: L.fluid_noise_dense(hnd, buf.data_ptr(), 4, float("inf"), 1, 0, 0), (b"amplitude",)),
                (lambda: L.fluid_noise_dense(hnd, buf.data_ptr(), 4, 1.0, 1, 0, -1), (b"stream_id -1",)),
                (lambda: L.fluid_noise_dense(hnd, buf.data_ptr(), 4, 1.0, 1, 0, 65536), (b"stream_id 65536",)),
                (lambda: L.fluid_noise_dense(hnd, host.ctypes.data, 4, 1.0, 1, 0, 0), (b"not device memory",)),
                (lambda: L.fluid_noise_dense(hnd, fits, 65, 1.0, 1, 0, 0), (b"allocation ends",)),
                (lambda: L.fluid_noise_dense(hnd, fits + 4, 64, 1.0, 1, 0, 0), (b"allocation ends",)),
                (lambda: L.fluid_noise_dense(hnd, fits + 2, 8, 1.0, 1, 0, 0), (b"aligned",)),
                (lambda: L.fluid_noise_dense(hnd, fits, 1 << 62, 1.0, 1, 0, 0), (b"count",)),
            ]
            keep = buf.cpu().numpy()
            for call, words in refused:
                L.fluid_synchronize(None)                   # (an unrelated message in between)
                assert call() == capi.E_INVALID, words
                msg = L.fluid_last_error()
                assert b"fluid_noise_dense" in msg and all(word in msg for word in words), (words, msg)
            s.synchronize()
            same_bits(buf.cpu().numpy(), keep, "the buffer after the refusals")
            assert L.fluid_noise_dense(hnd, fits, 64, 1.0, 1, 0, 0) == capi.OK, L.fluid_last_error()      # ends with its allocation
            s.synchronize()
            with pytest.raises(ValueError, match="count"):
                s.noise_dense(buf, 1.0, SEED, count=66)
        with F().FluidSolver(6, rank=0, nranks=2) as s:
            assert L.fluid_noise_dense(s._h, exact.value, 4, 1.0, 1, 0, 0) == capi.E_INVALID
            assert b"fluid_noise_dense" in L.fluid_last_error() and b"slab" in L.fluid_last_error()
    finally:
        assert hip.hipFree(exact) == 0


# ---- 7. refusals on a live context change nothing -------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(7)
    n, members = 6, 5
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    name = b"fluid_noise_members"
    good = floats(*([1.0] * members))

    def call(hnd, ids, count=None, mode=SET, amp=good, offset=0):
        return lambda: L.fluid_noise_members(hnd, ids, len(ids) if count is None else count, mode, amp, 1, 0, offset)

    ids3 = ints(0, 1, 2)
    with solver(n, members) as s, solver(n, members) as twin:
        for c in (s, twin):
            c.timing_enable(True)
            c.upload_members(**fields)
            c.step(use_sources=True)
            c.add_source("dens", "dens_prev", DT)                      # a lazy state that must survive the refusals
        hnd = s._h
        refused = []
        for mode in (SET, ADD):
            refused += [
                (lambda mode=mode: L.fluid_noise_members(hnd, None, 3, mode, good, 1, 0, 0), (b"fields",)),
                (lambda mode=mode: L.fluid_noise_members(hnd, ids3, 3, mode, None, 1, 0, 0), (b"amplitude",)),
                (call(None, ids3, mode=mode), (b"null context",)),
                (call(hnd, ids3, 0, mode=mode), (b"nfields 0",)),
                (call(hnd, ids3, 13, mode=mode), (b"nfields 13",)),
                (call(hnd, ids3, -1, mode=mode), (b"nfields -1",)),
                (call(hnd, ints(0, 12), mode=mode), (b"bad field id 12", b"fields[1]")),
                (call(hnd, ints(-1, 2), mode=mode), (b"bad field id -1", b"fields[0]")),
                (call(hnd, ints(2, 1, 2), mode=mode), (b"field 2", b"twice", b"fields[0]", b"fields[2]")),
                (call(hnd, ids3, mode=mode, amp=floats(1.0, 1.0, float("nan"), 1.0, 1.0)), (b"member 2", b"amplitude", b"not finite")),
                (call(hnd, ids3, mode=mode, amp=floats(float("inf"), 1.0, 1.0, 1.0, 1.0)), (b"member 0", b"amplitude", b"not finite")),
                (call(hnd, ids3, mode=mode, amp=floats(1.0, 1.0, 1.0, 1.0, -float("inf"))), (b"member 4", b"amplitude", b"not finite")),
                (call(hnd, ids3, mode=mode, offset=-1), (b"member_offset -1",)),
                (call(hnd, ids3, mode=mode, offset=65536 - members + 1), (b"member_offset %d" % (65536 - members + 1),)),
                (call(hnd, ids3, mode=mode, offset=2 ** 31 - 1), (b"member_offset",)),
            ]
        refused += [(call(hnd, ids3, mode=m), (b"mode %d" % m,)) for m in (-1, 2, 7)]
        for c, words in refused:
            L.fluid_synchronize(None)                   # (an unrelated message in between)
            assert c() == capi.E_INVALID, words
            msg = L.fluid_last_error()
            assert name in msg and all(word in msg for word in words), (words, msg)
        s.synchronize()
        ta, tb = s.timing_read(reset=False), twin.timing_read(reset=False)
        assert ta == {**tb, **{k: ta[k] for k in ta if k.endswith("_ms")}}             # every count; the times are times
        for f in capi.FIELD_NAMES:                      # every field of every member, and what they still owe themselves
            same_bits(shown(s, f), shown(twin, f), "%s after the refusals" % f)
        for c in (s, twin):
            c.step(use_sources=True)
        for f in ("u", "v", "dens"):
            same_bits(shown(s, f), shown(twin, f), "%s a step after the refusals" % f)
        # the launches belong to none of the timing categories
        ta = s.timing_read(reset=False)
        s.noise(("u", "v"), 1.0, 1, 0, SET)
        s.noise(("u", "v"), 1.0, 1, 0, ADD)
        s.synchronize()
        tb = s.timing_read(reset=False)
        assert all(ta[k] == tb[k] for k in ta if k.endswith("_calls")), (ta, tb)
        # the last legal offset is legal
        assert call(hnd, ids3, offset=65536 - members)() == capi.OK, L.fluid_last_error()
        with pytest.raises(ValueError, match="amplitude"):
            s.noise(("u",), [1.0, 2.0], 1)
    # row slabs
    with F().FluidSolver(n, rank=0, nranks=2) as s:
        assert call(s._h, ints(0), amp=floats(1.0))() == capi.E_INVALID
        msg = L.fluid_last_error()
        assert name in msg and b"slab" in msg, msg


# ---- 8. perturb is its three calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_perturb_equals_the_three_calls_made_by_hand(storage):
    rng = np.random.default_rng(8000 + storage)
    n, members = 30, 3
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    amp = amplitudes(rng, members, storage)
    alpha = np.array([0.5, 1.0, 2.0], F32)
    beta = (1.0 + 4.0 * alpha).astype(F32)
    with solver(n, members, storage) as a, solver(n, members, storage) as b:
        for s in (a, b):
            s.upload_members(**fields)
        a.perturb("dens", ("u_prev", "v_prev"), amp, SEED, 5, alpha, beta, 8)
        b.noise(("u_prev",), 1.0, SEED, 5, SET)
        b.diffuse(0, "v_prev", "u_prev", alpha, beta, 8)
        b.add_source("dens", "v_prev", amp)
        for f in MAIN:
            same_bits(shown(a, f), shown(b, f), "storage=%d: %s" % (storage, f))
        white = noise_set(w, members, 1.0, SEED, 5, ID["u_prev"], storage)
        same(shown(a, "u_prev"), white, "storage=%d: the white noise" % storage)
        smooth = shown(a, "v_prev")
        assert smooth[:, 1:-1, 1:-1].var() < 0.9 * white[:, 1:-1, 1:-1].var()               # smoothing shrinks the variance
        assert not np.array_equal(shown(a, "dens"), narrow(fields["dens"], storage))
