"""GPU: relaxation to prior spread -- fluid_member_spread / fluid_relax_spread (include/fluid_amd.h, "relaxation to prior
spread"): the per-cell sample standard deviation of a field over the members as a dense device array, and the anomalies
of a field rescaled in place towards such an array.

Every expected value comes from tests/relax_model.py, the header's definition in numpy float64, applied to what
download_members (the pack) showed before the call.  Everything is compared bit for bit; a NaN is a NaN, its sign and
payload are not compared.  The only bound is the property test's (part 4); tests/test_relax_abi.py shows on the CPU that
the model itself keeps it.

Shapes: N = 14 is one partial block, N = 30 two blocks with a tail ((N + 2) * 9 = 288 work items), N = 66 with fp16 storage
the size at which vectors of 8 halves would end in a ragged one (the kernels take 4 columns per lane in both storage
types; the last vector of a row is ragged at all three sizes); M = 70 is past the 64 members the transforms stop at."""
import ctypes as C

import numpy as np
import pytest

from relax_model import F32, narrow, property_bound, property_inputs, relax_model, spread_model

pytestmark = pytest.mark.gpu
MEMBERS = [2, 3, 5, 64, 70]
MAIN = ("u", "v", "dens", "u_prev", "v_prev", "dens_prev")
DT = 0.016
SENTINEL = 0x7FC5A5A5              # a NaN: a pad or a gap read as data would show


def sizes(storage):
    return (14, 30, 66) if storage else (14, 30)


def F():
    import fluidsimulationcuda_amd as f
    return f


def torch_():
    import torch
    return torch


def solver(n, members, storage=0, **kw):
    return F().FluidSolver(n, members=members, storage=storage, **kw)


def dev(a):
    return torch_().from_numpy(np.ascontiguousarray(a, F32)).cuda()


def ints(*v):
    return (C.c_int * len(v))(*v)


def shown(s, field):
    """what the pack shows: every member of a field, the lazy state settled"""
    return s.download_members(field)


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
    """every bit, NaN payloads included: for memory the call must not have changed"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = got.view(np.uint8) != want.view(np.uint8)
    assert not bad.any(), "%s: %d of %d bytes changed; first at %s" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


# ---- the device's own layout: an ensemble on a torch arena, so that pad columns and stored bits can be looked at -----------
def layout(n):
    from fluidsimulationcuda_amd import capi
    pitch, xoff, ff = C.c_int(), C.c_int(), C.c_size_t()
    assert capi.lib().fluid_layout(n, C.byref(pitch), C.byref(xoff), C.byref(ff)) == 0
    return pitch.value, xoff.value, ff.value


def arena_ensemble(n, members, storage=0):
    from fluidsimulationcuda_amd import capi
    torch = torch_()
    nbytes = capi.lib().fluid_arena_bytes_ensemble(n, storage, members)
    arena = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return solver(n, members, storage, arena_ptr=arena.data_ptr(), arena_bytes=nbytes), arena


def stored_view(s, arena, field):
    """a torch view of a field as the device holds it, through fluid_field_ptr: (members, N+2, pitch) elements as integers"""
    torch = torch_()
    pitch, _, ff = layout(s.n)
    esz = 2 if s.storage else 4
    assert ff == (s.n + 2) * pitch
    off = s.field_ptr(field) - arena.data_ptr()
    assert off >= 0 and off % esz == 0
    words = arena[off:off + s.members * ff * esz].view(torch.int16 if s.storage else torch.int32)
    return words.view(s.members, s.n + 2, pitch)


def stored_bits(s, arena, field):
    s.synchronize()
    torch_().cuda.synchronize()
    return stored_view(s, arena, field).cpu().numpy().copy()


def plant_pads(s, arena, field):
    """every pad column of a field becomes a NaN pattern: a kernel that read one as data, or wrote one, shows"""
    _, xoff, _ = layout(s.n)
    s.synchronize()
    v = stored_view(s, arena, field)
    v[:, :, :xoff] = 0x7E5A if s.storage else SENTINEL
    v[:, :, xoff + s.n + 2:] = 0x7E5A if s.storage else SENTINEL
    torch_().cuda.synchronize()


def cells_of(raw, n):
    _, xoff, _ = layout(n)
    return raw[:, :, xoff:xoff + n + 2]


def pads_of(raw, n):
    _, xoff, _ = layout(n)
    return np.concatenate([raw[:, :, :xoff], raw[:, :, xoff + n + 2:]], axis=2)


# ---- data ------------------------------------------------------------------------------------------------------------------
def random_values(rng, shape, storage):
    """every cell and member different, magnitudes over some binades, both signs"""
    lo, hi = (-6, 4) if storage else (-20, 20)
    x = np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(lo, hi, shape[1:])) * rng.choice([-1.0, 1.0], shape)
    return narrow(x.astype(F32), storage)


def random_prior(rng, x):
    """around the spread the ensemble has: factors 1/2 .. 2, so that f spans 0.5 .. 2"""
    sd = spread_model(x)
    return (sd * rng.uniform(0.5, 2.0, sd.shape)).astype(F32)


# ---- 1. random values ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", MEMBERS)
def test_random_values_three_fields_and_a_stride(members, storage):
    """spread and relax_spread against the model in all of W x W, all members, three fields in one call; the dense arrays
    one float off their allocation's start and field_stride above W*W: the floats in between and around are untouched, and
    so is every pad column of the fields."""
    from fluidsimulationcuda_amd import capi
    torch = torch_()
    L = capi.lib()
    rng = np.random.default_rng(1000 * storage + members)
    names = ("dens", "u", "v_prev")
    ids = ints(*[capi.FIELD_NAMES.index(f) for f in names])
    for n in sizes(storage):
        w = n + 2
        cells, stride, lead = w * w, w * w + 5, 1
        what = "n=%d M=%d storage=%d" % (n, members, storage)
        s, arena = arena_ensemble(n, members, storage)
        with s:
            s.upload_members(**{f: random_values(rng, (members, w, w), storage) for f in MAIN})
            for f in MAIN:
                plant_pads(s, arena, f)
            before = {f: shown(s, f) for f in MAIN}
            raw_before = {f: stored_bits(s, arena, f) for f in MAIN}
            words = lead + 2 * stride + cells + 3
            # the spread: into a sentinel-filled buffer
            buf = torch.full((words,), SENTINEL, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            assert L.fluid_member_spread(s._h, ids, 3, buf.data_ptr() + 4 * lead, stride) == capi.OK, L.fluid_last_error()
            s.synchronize()
            got = buf.cpu().numpy()
            gap = np.ones(words, bool)
            for k, f in enumerate(names):
                at = lead + k * stride
                same(got[at:at + cells].view(F32).reshape(w, w), spread_model(before[f]), "%s: the spread of %s" % (what, f))
                gap[at:at + cells] = False
            assert (got[gap] == SENTINEL).all(), "%s: the spread wrote outside its three arrays" % what
            for f in MAIN:
                same_bits(stored_bits(s, arena, f), raw_before[f], "%s: %s after the spread" % (what, f))
            # ... the same through the solver: one contiguous tensor
            sd = s.spread(names)
            assert tuple(sd.shape) == (3, w, w) and sd.dtype == torch.float32
            for k, f in enumerate(names):
                same(sd[k].cpu().numpy(), spread_model(before[f]), "%s: spread() of %s" % (what, f))
            # the relaxation: priors in a strided buffer of the same shape
            prior = {f: random_prior(rng, before[f]) for f in names}
            host = np.full(words, SENTINEL, np.int32)
            for k, f in enumerate(names):
                at = lead + k * stride
                host[at:at + cells] = prior[f].view(np.int32).ravel()
            buf = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
            assert L.fluid_relax_spread(s._h, ids, 3, buf.data_ptr() + 4 * lead, stride, 0.75) == capi.OK, L.fluid_last_error()
            s.synchronize()
            same_bits(buf.cpu().numpy(), host, "%s: the priors after the relaxation" % what)
            for f in MAIN:
                raw = stored_bits(s, arena, f)
                same_bits(pads_of(raw, n), pads_of(raw_before[f], n), "%s: the pad columns of %s" % (what, f))
                if f in names:
                    want, stored = relax_model(before[f], prior[f], 0.75, storage)
                    assert stored.mean() > 0.9, what
                    same(shown(s, f), want, "%s: %s relaxed" % (what, f))
                else:
                    same_bits(raw, raw_before[f], "%s: %s was not listed" % (what, f))
            # ... and through the solver, on top of that
            again = {f: shown(s, f) for f in names}
            s.relax_spread(dev(np.stack([prior[f] for f in names])), 1.25, fields=names)
            for f in names:
                same(shown(s, f), relax_model(again[f], prior[f], 1.25, storage)[0], "%s: relax_spread() of %s" % (what, f))


def test_the_solver_refuses_tensors_of_the_wrong_kind():
    torch = torch_()
    n, members = 6, 3
    w = n + 2
    with solver(n, members) as s:
        x = np.random.default_rng(2).uniform(-1, 1, (members, w, w)).astype(F32)
        s.upload_members(u=x, v=x, dens=x)
        good = torch.ones((3, w, w), dtype=torch.float32, device="cuda")
        for bad in (torch.ones((2, w, w), dtype=torch.float32, device="cuda"), torch.ones((3, w, w + 1), dtype=torch.float32, device="cuda"),
                    torch.ones((3, w, 2 * w), dtype=torch.float32, device="cuda")[:, :, ::2],
                    torch.ones((3, w, w), dtype=torch.float64, device="cuda"), torch.ones((3, w, w), dtype=torch.float32)):
            with pytest.raises(ValueError):
                s.relax_spread(bad, 0.5)
            with pytest.raises(ValueError):
                s.spread(out=bad)
        with pytest.raises(TypeError):
            s.relax_spread(np.ones((3, w, w), F32), 0.5)
        for f in ("u", "v", "dens"):
            same(shown(s, f), x, "%s after the refused tensors" % f)
        assert s.spread(out=good) is good


# ---- 2. planted cells ----------------------------------------------------------------------------------------------------------
KINDS = ("equal -0", "equal value", "f == 1", "NaN member", "inf member", "inf prior", "NaN prior", "negative prior")


def planted(rng, n, members, storage):
    """random values and priors with one cell of every kind on the ghost ring and one inside, each at the start, inside or
    at the end of a lane's vector: (x, prior, {kind: [cells]})"""
    w = n + 2
    x = random_values(rng, (members, w, w), storage)
    prior = random_prior(rng, x)
    ring = [(0, 0), (0, w - 1), (w - 1, 0), (w - 1, w - 1), (0, w // 2), (w - 1, 5), (w // 2, 0), (7, w - 1)]
    inside = [(1, 1), (2, 4), (3, 5), (4, 8), (5, 9), (w - 2, w - 2), (6, w - 3), (w - 3, 3)]
    # members whose sample variance is an exact square: sa = 1 (M = 3, 5), sa = 2 (M = 64): the prior can equal it
    unit = {3: ([1, -1, 0], 1.0), 5: ([1, -1, 1, -1, 0], 1.0), 64: ([3, -3] * 14 + [0] * 36, 2.0)}[members]
    where = {k: [] for k in KINDS}
    for at, (i, j) in enumerate(ring + inside):
        kind = KINDS[at % len(KINDS)]
        where[kind].append((i, j))
        if kind == "equal -0":
            x[:, i, j] = -0.0
        elif kind == "equal value":
            x[:, i, j] = 0.375
        elif kind == "f == 1":
            x[:, i, j] = np.asarray(unit[0], F32) + F32(4.0 if at % 2 else 0.0)      # (a mean of 4 leaves the anomalies exact)
            prior[i, j] = unit[1]
        elif kind == "NaN member":
            x[at % members, i, j] = np.nan
        elif kind == "inf member":
            x[(at + 1) % members, i, j] = np.inf if at % 2 else -np.inf
        elif kind == "inf prior":
            prior[i, j] = np.inf
        elif kind == "NaN prior":
            prior[i, j] = np.nan
        elif kind == "negative prior":
            prior[i, j] = -prior[i, j]
    return x, prior, where


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", [3, 5, 64])
def test_planted_cells(members, storage):
    rng = np.random.default_rng(2000 * storage + members)
    for n in sizes(storage):
        what = "n=%d M=%d storage=%d" % (n, members, storage)
        x, prior, where = planted(rng, n, members, storage)
        with solver(n, members, storage) as s:
            s.upload_members(dens=x)
            before = shown(s, "dens")
            same(before, x, what + ": the upload")
            want_sd = spread_model(before)
            want, stored = relax_model(before, prior, 1.0, storage)
            # the model sees the cases the way they are meant
            for kind in ("equal -0", "equal value", "f == 1"):
                for i, j in where[kind]:
                    assert not stored[i, j], (what, kind)
            for i, j in where["f == 1"]:
                assert want_sd[i, j] == prior[i, j] and want_sd[i, j] > 0, what
            for kind in ("NaN member", "inf member"):
                for i, j in where[kind]:
                    assert np.isnan(want_sd[i, j]) and not np.isfinite(want[:, i, j]).any(), (what, kind)
            for kind in ("inf prior", "NaN prior"):
                for i, j in where[kind]:
                    assert np.isfinite(want_sd[i, j]) and not np.isfinite(want[:, i, j]).any(), (what, kind)
            for i, j in where["negative prior"]:
                assert np.isfinite(want[:, i, j]).all() and stored[i, j], what
            special = np.zeros(stored.shape, bool)
            for cells in where.values():
                for i, j in cells:
                    special[i, j] = True
            assert np.isfinite(want[:, ~special]).all() and np.isfinite(want_sd[~special]).all(), what     # their own cell only
            # the device
            same(s.spread(("dens",))[0].cpu().numpy(), want_sd, what + ": the spread")
            s.relax_spread(dev(prior[None]), 1.0, fields=("dens",))
            after = shown(s, "dens")
            same(after, want, what + ": relaxed")
            same_bits(after[:, ~stored], before[:, ~stored], what + ": the cells that are not stored")


# ---- 3. alpha = 0 and alpha = 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", MEMBERS)
def test_alpha_zero_keeps_every_bit_and_alpha_one_is_the_model(members, storage):
    rng = np.random.default_rng(3000 * storage + members)
    for n in sizes(storage):
        w = n + 2
        what = "n=%d M=%d storage=%d" % (n, members, storage)
        s, arena = arena_ensemble(n, members, storage)
        with s:
            x = random_values(rng, (members, w, w), storage)
            x[:, 3, 3] = -0.0
            x[1, 4, 4] = np.nan                                    # (alpha = 0 stores that cell: a NaN stays a NaN)
            s.upload_members(u=x)
            prior = random_prior(rng, x)
            prior[2, 2] = 0.0
            prior[5, 5] = 3.0e38
            raw = stored_bits(s, arena, "u")
            s.relax_spread(dev(prior[None]), 0.0, fields=("u",))
            got = stored_bits(s, arena, "u")
            keep = np.ones((w, w), bool)
            keep[4, 4] = False
            same_bits(cells_of(got, n)[:, keep], cells_of(raw, n)[:, keep], what + ": alpha = 0")
            same_bits(pads_of(got, n), pads_of(raw, n), what + ": alpha = 0, the pads")
            assert np.isnan(shown(s, "u")[:, 4, 4]).all(), what
            before = shown(s, "u")
            s.relax_spread(dev(prior[None]), 1.0, fields=("u",))
            same(shown(s, "u"), relax_model(before, prior, 1.0, storage)[0], what + ": alpha = 1")


# ---- 4. the property: alpha = 1 restores the prior spread -----------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", MEMBERS)
def test_alpha_one_restores_the_prior_spread(members, storage):
    """|sd' - sd_b| <= 2^-23 (max_m |y_m| + sd_b) per cell (fp16 storage: 2^-10): each stored member is off by at most half an
    ulp, 2^-24 |y|, which moves a sample standard deviation by at most sqrt(M / (M - 1)) <= sqrt(2) times that; the output's
    own rounding adds 2^-24 sd; the factor 2 covers the double roundings.  Once on the ensemble the prior was taken from,
    once on that ensemble with its anomalies halved -- what an analysis does."""
    for n in (14, 30):
        x = property_inputs(n, members, storage, seed=4000 + 100 * storage + members)
        what = "n=%d M=%d storage=%d" % (n, members, storage)
        with solver(n, members, storage) as s:
            s.upload_members(dens=x)
            same(shown(s, "dens"), x, what + ": the upload")
            sd_b = s.spread(("dens",))
            mean = x.mean(axis=0, dtype=np.float64)
            for case, start in (("as it is", None), ("anomalies halved", narrow(mean + 0.5 * (x - mean), storage))):
                if start is not None:
                    s.upload_members(dens=start)
                s.relax_spread(sd_b, 1.0, fields=("dens",))
                y = shown(s, "dens")
                sd = s.spread(("dens",))[0].cpu().numpy()
                b = sd_b[0].cpu().numpy()
                err = np.abs(sd.astype(np.float64) - b.astype(np.float64))
                bound = property_bound(y, b, storage)
                print("%s, %s: max |sd' - sd_b| = %.3g, the bound there %.3g" % (what, case, err.max(), bound.ravel()[err.argmax()]))
                assert (err <= bound).all(), "%s, %s: over the bound by %g at %s" % (
                    what, case, (err - bound).max(), np.unravel_index((err - bound).argmax(), err.shape))
                if start is not None:
                    assert (np.abs(spread_model(start).astype(np.float64) - b) > 4 * bound).mean() > 0.9, what      # it was off before


def slot_values(s, arena, slot):
    """the cells of all members of one of the arena's twelve field slots, fp16 storage, widened: what the device holds"""
    pitch, xoff, ff = layout(s.n)
    s.synchronize()
    torch_().cuda.synchronize()
    raw = arena.cpu().numpy()[:12 * s.members * ff * 2].view(np.float16).reshape(12, s.members, s.n + 2, pitch)
    return raw[slot, :, :, xoff:xoff + s.n + 2].astype(F32)


def scaled_slot(s, arena, values):
    """the slot that holds `values` (what the pack shows of a field) times one power of two, and that factor -- found in
    the arena itself: fluid_field_ptr would settle the scale away"""
    big = np.abs(values) > 2.0 ** -10
    for slot in range(12):
        raw = slot_values(s, arena, slot)
        with np.errstate(all="ignore"):
            ratio = np.unique(raw[big] / values[big])
        if ratio.size == 1 and np.isfinite(ratio[0]) and np.array_equal(raw, values * ratio[0]):
            return slot, float(ratio[0])
    return None, None


# ---- 5. an fp16 field held at a pressure scale -----------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [2, 5, 70])
def test_an_fp16_field_at_a_pressure_scale_keeps_it(members):
    rng = np.random.default_rng(5000 + members)
    for n in (30, 66):                         # (the library scales the pressure from N = 16 on)
        w = n + 2
        what = "n=%d M=%d" % (n, members)
        s, arena = arena_ensemble(n, members, 1)
        with s:
            s.upload_members(**{f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN})
            s.step(use_sources=True)               # fp16 storage: u_prev now holds the pressure, scaled
            before = shown(s, "u_prev")
            slot, scale = scaled_slot(s, arena, before)
            assert scale not in (None, 1.0), "%s: u_prev is not held at a scale other than 1 (%s)" % (what, scale)
            raw = slot_values(s, arena, slot)
            print("%s: u_prev is held at scale %g; %d of %d values it shows are no halves" % (
                what, scale, int((narrow(before, 1) != before).sum()), before.size))
            same(s.spread(("u_prev",))[0].cpu().numpy(), spread_model(before), what + ": the spread shows the pack's values")
            same_bits(slot_values(s, arena, slot), raw, what + ": the spread stores nothing")
            prior = random_prior(rng, before)
            # alpha = 0: nothing is stored; the field shows exactly what it showed, and holds the bits it held
            s.relax_spread(dev(prior[None]), 0.0, fields=("u_prev",))
            same_bits(shown(s, "u_prev"), before, what + ": alpha = 0")
            same_bits(slot_values(s, arena, slot), raw, what + ": alpha = 0, stored bits")
            # alpha = 0.9: narrow(y), held at the scale
            s.relax_spread(dev(prior[None]), 0.9, fields=("u_prev",))
            want, stored = relax_model(before, prior, 0.9, 1)
            assert stored.mean() > 0.9, what
            after = shown(s, "u_prev")
            same(after, want, what + ": alpha = 0.9")
            same(slot_values(s, arena, slot), after * F32(scale), what + ": the field is still held at its scale")
            s.step(use_sources=True)
            for f in ("u", "v", "dens"):
                assert np.isfinite(shown(s, f)).all(), "%s: %s a step later" % (what, f)


# ---- 6. the lazy state is settled first ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("case", ["source", "zero source"])
def test_the_lazy_state_is_settled_first(case, storage):
    rng = np.random.default_rng(6000 + storage)
    n, members = 30, 5
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    prior = rng.uniform(0.2, 1.0, (w, w)).astype(F32)

    def prepared():
        s = solver(n, members, storage)
        s.upload_members(**fields)
        if case == "zero source":
            s.step(use_sources=True)
            s.computeDivergenceAndPressure("u", "v", "dens_prev", "tmp0")       # its pressure is zero by definition: marked, not written
        s.add_source("dens", "dens_prev", DT)                                   # deferred: dens owes itself the increment
        return s

    with prepared() as a, prepared() as b, prepared() as c:
        before = shown(b, "dens")                                               # the twin: the calls never ran there
        if case == "source":
            assert not np.array_equal(before, narrow(fields["dens"], storage)), "the source does something"
        a.relax_spread(dev(prior[None]), 0.6, fields=("dens",))
        same(shown(a, "dens"), relax_model(before, prior, 0.6, storage)[0], "%s storage=%d: relaxed" % (case, storage))
        same(c.spread(("dens",))[0].cpu().numpy(), spread_model(before), "%s storage=%d: the spread" % (case, storage))
        same_bits(shown(c, "dens"), before, "%s storage=%d: the spread alters nothing" % (case, storage))
        for f in MAIN:
            if f != "dens":
                same_bits(shown(a, f), shown(b, f), "%s storage=%d: %s was not listed" % (case, storage, f))


# ---- 7. refusals on a live context ----------------------------------------------------------------------------------------------
def hip_runtime():
    """the HIP runtime this process already holds (the one libfluid_amd.so runs on)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime is loaded")


def test_refusals_change_nothing():
    torch = torch_()
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(7)
    n, members = 6, 5
    w = n + 2
    cells = w * w
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    hip = hip_runtime()
    exact = C.c_void_p()
    size = 1 << 20
    assert hip.hipMalloc(C.byref(exact), C.c_size_t(size)) == 0
    fits = exact.value + size - 3 * cells * 4             # three dense arrays that end with their allocation
    short = fits + 4                                      # ... and one float past it
    host = np.ones((3, w, w), F32)
    good = torch.full((3, w, w), 0.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    one, two = "fluid_member_spread", "fluid_relax_spread"

    def spread(hnd, ids, count=None, p=None, stride=0):
        return lambda: L.fluid_member_spread(hnd, ids, len(ids) if count is None else count, good.data_ptr() if p is None else p, stride)

    def relax(hnd, ids, count=None, p=None, stride=0, alpha=0.5):
        return lambda: L.fluid_relax_spread(hnd, ids, len(ids) if count is None else count, good.data_ptr() if p is None else p, stride, alpha)

    ids = ints(0, 1, 2)
    try:
        with solver(n, members) as s, solver(n, members) as twin:
            for c in (s, twin):
                c.timing_enable(True)
                c.upload_members(**fields)
                c.step(use_sources=True)
                c.add_source("dens", "dens_prev", DT)                      # a lazy state that must survive the refusals
            hnd = s._h
            null_fields = {one: lambda: L.fluid_member_spread(hnd, None, 3, good.data_ptr(), 0),
                           two: lambda: L.fluid_relax_spread(hnd, None, 3, good.data_ptr(), 0, 0.5)}
            refused = []
            for name, call in ((one, spread), (two, relax)):
                refused += [
                    (name, null_fields[name], (b"fields",)),
                    (name, call(hnd, ids, p=0), (b"out_dev" if call is spread else b"prior_dev",)),
                    (name, call(None, ids), (b"null context",)),
                    (name, call(hnd, ids, 0), (b"nfields 0",)),
                    (name, call(hnd, ids, 13), (b"nfields 13",)),
                    (name, call(hnd, ids, -1), (b"nfields -1",)),
                    (name, call(hnd, ints(0, 12)), (b"bad field id 12", b"fields[1]")),
                    (name, call(hnd, ints(-1, 2)), (b"bad field id -1", b"fields[0]")),
                    (name, call(hnd, ints(2, 1, 2)), (b"field 2", b"twice", b"fields[0]", b"fields[2]")),
                    (name, call(hnd, ids, stride=cells - 1), (b"field_stride %d" % (cells - 1),)),
                    (name, call(hnd, ids, stride=1), (b"field_stride 1",)),
                    (name, call(hnd, ids, p=host.ctypes.data), (b"not device memory",)),
                    (name, call(hnd, ids, p=short), (b"allocation ends",)),
                    (name, call(hnd, ids, p=fits, stride=cells + 1), (b"allocation ends",)),
                    (name, call(hnd, ids, p=fits + 2), ()),                                        # (misaligned, and short)
                ]
            refused += [(two, relax(hnd, ids, alpha=a), (b"alpha",)) for a in (-0.5, float("nan"), float("inf"), -float("inf"))]
            for name, call, words in refused:
                L.fluid_synchronize(None)                   # (an unrelated message in between)
                assert call() == capi.E_INVALID, (name, words)
                msg = L.fluid_last_error()
                assert name.encode() in msg and all(word in msg for word in words), (name, words, msg)
            s.synchronize()
            assert (good.cpu().numpy() == 0.5).all()
            ta, tb = s.timing_read(reset=False), twin.timing_read(reset=False)
            assert ta == {**tb, **{k: ta[k] for k in ta if k.endswith("_ms")}}             # every count; the times are times
            for f in capi.FIELD_NAMES:                      # every field of every member, and what they still owe themselves
                same_bits(shown(s, f), shown(twin, f), "%s after the refusals" % f)
            for c in (s, twin):
                c.step(use_sources=True)
            for f in ("u", "v", "dens"):
                same_bits(shown(s, f), shown(twin, f), "%s a step after the refusals" % f)
            # what is not refused: three arrays that end with their allocation, written and then read there
            assert L.fluid_member_spread(hnd, ids, 3, fits, 0) == capi.OK, L.fluid_last_error()
            assert L.fluid_relax_spread(hnd, ids, 3, fits, cells, 1.0) == capi.OK, L.fluid_last_error()
            s.synchronize()
        # one member: no spread
        with solver(n, 1) as s:
            x = rng.uniform(-1.0, 1.0, (1, w, w)).astype(F32)
            s.upload_members(u=x)
            for name, call in ((one, spread), (two, relax)):
                assert call(s._h, ints(0))() == capi.E_INVALID, name
                msg = L.fluid_last_error()
                assert name.encode() in msg and b"1 member" in msg, (name, msg)
            same_bits(shown(s, "u"), x, "u after the refused calls on one member")
        # row slabs
        with F().FluidSolver(n, rank=0, nranks=2) as s:
            for name, call in ((one, spread), (two, relax)):
                assert call(s._h, ints(0))() == capi.E_INVALID, name
                msg = L.fluid_last_error()
                assert name.encode() in msg and b"slab" in msg, (name, msg)
    finally:
        assert hip.hipFree(exact) == 0
