"""GPU: asynchronous observations -- fluid_observe_members_range, fluid_run_window and the three recorded analysis calls
(include/fluid_amd.h, "asynchronous observations").

Nothing is defined here but the record: a dense (M, stride) float32 array with h[m][p] at [m, p].  What a record must hold comes
from `observe_device`, what a Gram must be from `OB.operands` / `OB.exact_sums` or from the direct call, what an analysis must
be from `EK.composed`, what a windowed run must be from the loop of one-step `run`, `pack` and `observe_range` calls it is
defined as -- all imported from the tests of the direct calls or made of the solver's own methods, compared bit for bit (`==`
on dyadic data for the model of test 4).  `FromRecord` lets the imported helpers that take (solver, field) take (solver, record).

Shapes: N = 6 and 30; M = 5, 8, 17 (the Gram kernels pad them to 8, 8 and 32); P = 65 and 130: a full chunk of 64 points plus one,
and two chunks plus two; strides P and P + 3, the gap floats holding NaNs that must be neither read nor written."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_etkf as EK
import test_gpu_lattice_gram as LG
import test_gpu_network as NW
import test_gpu_observe as OB

pytestmark = pytest.mark.gpu
F32 = np.float32
STORAGES = pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
MEMBERS = [5, 8, 17]
POINTS = [65, 130]
COMBOS = [(None, None), ("y", None), (None, "sg"), ("y", "sg")]         # obs and sigma present or absent


def torch_():
    import torch
    return torch


class FromRecord:
    """a solver whose lattice Gram reads a record: `LG.call` and `EK.composed` take it for the solver, the record for the field"""

    def __init__(self, s, stride=0):
        self.s, self.stride = s, stride

    def observation_gram_lattice(self, record, *args, **kw):
        return self.s.observation_gram_lattice_recorded(record, *args, member_stride=self.stride, **kw)

    def __getattr__(self, name):
        return getattr(self.s, name)


def pattern(members, p, stride):
    """(M - 1) * stride + P floats, every one a NaN with its own payload: what a float nobody wrote still holds"""
    count = (members - 1) * stride + p
    return (np.uint32(0x7FC00000) + 1 + np.arange(count, dtype=np.uint32) % np.uint32(0x3FFFFF)).view(F32)


def device(a):
    torch = torch_()
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def rows_of(flat, members, p, stride):
    """the (M, P) values of a flat record"""
    return np.stack([flat[m * stride:m * stride + p] for m in range(members)])


def record_of(h, stride):
    """a flat record holding h (M, P), the gap floats NaN"""
    members, p = h.shape
    flat = pattern(members, p, stride).copy()
    for m in range(members):
        flat[m * stride:m * stride + p] = h[m]
    return device(flat)


def snapshot(s, names):
    return {f: s.download_members(f).view(np.uint32) for f in names}


def unchanged(s, before, what):
    for f, x in before.items():
        assert np.array_equal(s.download_members(f).view(np.uint32), x), "%s: the call changed %s" % (what, f)


# ---- 1. a range is observe_device's bits inside it, and nobody's outside ------------------------------------------------------------
@STORAGES
@pytest.mark.parametrize("n", [6, 30])
def test_a_range_writes_its_points_and_nothing_else(n, storage):
    w = n + 2
    rng = np.random.default_rng(51000 + 10 * n + storage)
    for members in MEMBERS:
        with OB.solver(n, members, storage) as s:
            s.upload_members(dens=rng.uniform(-4.0, 4.0, (members, w, w)).astype(F32), u=rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32),
                             v=rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32))
            s.vel_step()                               # fp16 storage, N >= 16: u_prev and v_prev are held scaled
            for p in POINTS:
                cols, rows = OB.network(n, p, rng)
                for names, field in ((None, "dens"), (None, "u_prev"), (NW.fields_of(p, NW.FIVE), None)):
                    s.set_observation_network(cols, rows, names)
                    before = snapshot(s, NW.FIVE)
                    for stride in (p, p + 3):
                        what = "n=%d M=%d storage=%d P=%d stride=%d field=%s" % (n, members, storage, p, stride, field)
                        empty = pattern(members, p, stride)
                        full = bits(s.observe_device(field, out=device(empty), member_stride=stride))
                        assert np.array_equal(rows_of(full, members, p, stride), s.observe(field).view(np.uint32)), what
                        for first, end in ((0, p), (0, 0), (64, 65), (1, 64), (63, p)):
                            rec = device(empty)
                            assert s.observe_range(first, end - first, rec, field, member_stride=stride) is rec
                            inside = np.zeros(empty.size, bool)
                            for m in range(members):
                                inside[m * stride + first:m * stride + end] = True
                            want = np.where(inside, full, empty.view(np.uint32))
                            got = bits(rec)
                            assert np.array_equal(got, want), "%s [%d, %d): %d floats differ" % (what, first, end, int((got != want).sum()))
                    unchanged(s, before, "observe_range")


# ---- 2. a record observe_device just wrote gives the direct calls' bits ----------------------------------------------------------------
@STORAGES
@pytest.mark.parametrize("members", MEMBERS)
def test_recorded_is_direct_bit_for_bit(members, storage):
    from fluidsimulationcuda_amd import capi
    rho, listed = 1.1, ("dens", "u", "v")
    for case, (n, p, stride, lat, c) in enumerate(((6, 65, 68, ((1, 3), (3, -5), 8), 3.0), (30, 130, 130, ((3, 3), (-8, 0), 16), 6.0),
                                                   (30, 65, 68, ((3, 3), (-8, 0), 16), 6.0), (6, 130, 130, ((1, 3), (3, -5), 8), 3.0))):
        rng = np.random.default_rng(52000 + 1000 * case + 100 * members + storage)
        w = n + 2
        if n == 30:
            fields, (cols, rows) = EK.start_fields(n, members, rng), EK.network(rng, p)
        else:
            fields, (cols, rows) = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in OB.MAIN}, OB.network(n, p, rng)
        names, field = ((NW.fields_of(p, NW.THREE), None), (None, "dens"))[case % 2]        # a typed network and an untyped one
        val = {"y": rng.uniform(0.2, 1.5, p).astype(F32), "sg": rng.uniform(2.0, 8.0, p).astype(F32), None: None}
        with EK.solver(n, members, storage) as a, EK.solver(n, members, storage) as b:
            for s in (a, b):
                s.upload_members(**fields)
                s.step(2, use_sources=True)                    # fp16: the pressure scale is live
                s.set_observation_network(cols, rows, names)
            record = a.observe_device(field, out=device(pattern(members, p, stride)), member_stride=stride)
            rec = FromRecord(a, stride)
            for centre in (False, True):
                for obs, sigma in COMBOS:
                    what = "M=%d storage=%d n=%d P=%d stride=%d centre=%s obs=%s sigma=%s" % (members, storage, n, p, stride, centre, obs, sigma)
                    y, sg = val[obs], val[sigma]
                    direct = OB.pack_results(members, a.observation_gram(field, obs=y, inv_sigma=sg, centre=centre))
                    got = OB.pack_results(members, a.observation_gram_recorded(record, obs=y, inv_sigma=sg, centre=centre, member_stride=stride))
                    OB.same_bits(got, direct, what + ": Gram")
                    # recorded and direct calls take turns on one lattice: the kept lists serve both
                    first = LG.call(rec, record, lat, c, y, sg, centre)
                    direct = LG.call(a, field, lat, c, y, sg, centre)
                    again = LG.call(rec, record, lat, c, y, sg, centre)
                    LG.check_shapes(first, lat, members)
                    for got in (first, again):
                        LG.same_bits(LG.flat(got), LG.flat(direct), what + ": lattice Gram")
                        assert np.array_equal(got[3], direct[3]), what + ": counts"
                    assert direct[3].sum() > 0
            for sg in (None, val["sg"]):
                a.analyse_lattice(field, lat[0], lat[1], lat[2], c, val["y"], inv_sigma=sg, rho=rho, fields=listed)
                b.analyse_lattice_recorded(record, lat[0], lat[1], lat[2], c, val["y"], inv_sigma=sg, rho=rho, fields=listed, wait=False,
                                           member_stride=stride)
                status = a.analyse_status()
                assert b.analyse_status() == status and status["solved"] >= 1, status
                EK.same_members(b, a, capi.FIELD_NAMES, "analyse_lattice_recorded, M=%d storage=%d n=%d P=%d" % (members, storage, n, p))
                changed = [f for f in listed if not np.array_equal(b.download_members(f).view(np.uint32), fields[f].view(np.uint32))]
                assert changed == list(listed)
                record = a.observe_device(field, out=record, member_stride=stride)          # the analysed state, for the second round
            got, empty = bits(record), pattern(members, p, stride).view(np.uint32)
            for m in range(members - 1):                        # the floats between two members: never written
                assert np.array_equal(got[m * stride + p:(m + 1) * stride], empty[m * stride + p:(m + 1) * stride])


# ---- 3. the record is what is read, not the fields ----------------------------------------------------------------------------------------
@STORAGES
@pytest.mark.parametrize("members,p", [(8, 65), (17, 130), (5, 130)])
def test_the_record_is_what_is_read(members, p, storage):
    from fluidsimulationcuda_amd import capi
    n = 30
    lat, c, rho, listed = ((3, 3), (-8, 0), 16), 6.0, 1.1, ("dens", "u", "v")
    rng = np.random.default_rng(53000 + 100 * members + storage)
    fields = EK.start_fields(n, members, rng)
    cols, rows = EK.network(rng, p)
    names = NW.fields_of(p, NW.THREE)
    y, sg = rng.uniform(0.2, 1.5, p).astype(F32), rng.uniform(2.0, 8.0, p).astype(F32)
    what = "M=%d storage=%d P=%d" % (members, storage, p)
    with EK.solver(n, members, storage) as a, EK.solver(n, members, storage) as twin:
        for s in (a, twin):
            s.upload_members(**fields)
            s.step(2, use_sources=True)
            s.set_observation_network(cols, rows, names)
        record = a.observe_device()
        saved = {centre: (OB.pack_results(members, a.observation_gram(obs=y, inv_sigma=sg, centre=centre)), LG.call(a, None, lat, c, y, sg, centre))
                 for centre in (False, True)}
        for s in (a, twin):                                    # the window goes on: the state at its end is another one
            s.step(1)
            s.noise(listed, 0.05, seed=7, sequence=3, mode=capi.NOISE_ADD)
        EK.same_members(a, twin, capi.FIELD_NAMES, what + ": the twin")
        for centre in (False, True):
            now = OB.pack_results(members, a.observation_gram(obs=y, inv_sigma=sg, centre=centre))
            assert not np.array_equal(now, saved[centre][0]), what + ": the change did not reach the observations"
            got = OB.pack_results(members, a.observation_gram_recorded(record, obs=y, inv_sigma=sg, centre=centre))
            OB.same_bits(got, saved[centre][0], what + " centre=%s: the recorded Gram after the change" % centre)
            got = LG.call(FromRecord(a), record, lat, c, y, sg, centre)
            LG.same_bits(LG.flat(got), LG.flat(saved[centre][1]), what + " centre=%s: the recorded lattice Gram after the change" % centre)
            assert np.array_equal(got[3], saved[centre][1][3])
        EK.same_members(a, twin, capi.FIELD_NAMES, what + ": the recorded Gram calls settle and change nothing")
        a.analyse_lattice_recorded(record, lat[0], lat[1], lat[2], c, y, inv_sigma=sg, rho=rho, fields=listed, wait=False)
        d, status, counts = EK.composed(FromRecord(twin), record, lat[0], lat[1], lat[2], c, y, sg, rho, listed)
        want = {"solved": int((status == 0).sum()), "empty": int((status == 1).sum()), "failed": int((status == 2).sum())}
        assert a.analyse_status() == want and want["solved"] >= 2 and want["failed"] == 0 and np.abs(d).max() > 1e-4, (what, want)
        EK.same_members(a, twin, capi.FIELD_NAMES, what + ": analyse_lattice_recorded against the chain")
        # ... and it is not what the fields give now
        with EK.solver(n, members, storage) as direct:
            direct.upload_members(**fields)
            direct.step(2, use_sources=True)
            direct.set_observation_network(cols, rows, names)
            direct.step(1)
            direct.noise(listed, 0.05, seed=7, sequence=3, mode=capi.NOISE_ADD)
            direct.analyse_lattice(None, lat[0], lat[1], lat[2], c, y, inv_sigma=sg, rho=rho, fields=listed)
            assert not np.array_equal(direct.download_members("dens"), a.download_members("dens")), what


# ---- 4. layout and model: a record nobody observed, exact sums -------------------------------------------------------------------------
@STORAGES
@pytest.mark.parametrize("members", MEMBERS)
def test_gram_of_a_dyadic_record_is_exact(members, storage):
    rng = np.random.default_rng(54000 + 100 * storage + members)
    for n, p in ((6, 65), (30, 130)):
        cols, rows = OB.network(n, p, rng)
        y = (rng.integers(-8, 9, p) / 4.0).astype(F32)
        sg = rng.choice(np.array([0.5, 1.0, 2.0], F32), p)
        val = {"y": y, "sg": sg, None: None}
        with OB.solver(n, members, storage) as s:
            s.set_observation_points(cols, rows)                     # the positions and P; the fields are zero and stay unread
            for stride in (p, p + 3):
                h = rng.choice(OB.COARSE, size=(members, p)).astype(F32)
                record = record_of(h, stride)
                for centre in (False, True):
                    if centre and not NW.power_of_two(members):  # a power of two: the mean, the anomalies and the products are exact
                        continue
                    for obs, sigma in COMBOS:
                        what = "M=%d storage=%d n=%d P=%d stride=%d centre=%s obs=%s sigma=%s" % (members, storage, n, p, stride, centre, obs, sigma)
                        g = s.observation_gram_recorded(record, obs=val[obs], inv_sigma=val[sigma], centre=centre, member_stride=stride)
                        am, d = OB.operands(h, val[obs], val[sigma], centre)
                        gram, rhs, dd = OB.exact_sums(am, d, 14)
                        OB.equal(g[0] if obs else g, gram, what)
                        OB.symmetric(g[0] if obs else g, what)
                        if obs:
                            OB.equal(g[1], rhs, what + ": rhs")
                            OB.equal(g[2], dd, what + ": dd")


# ---- 5. a windowed run is the loop it is defined as -------------------------------------------------------------------------------------
SLOT_FIRST = [3, 40, 64, 101, 101, 127]          # points 0 .. 2 and 127 .. 129 are in no slot; slot 3 is empty
SLOT_STEP = [1, 0, 4, 3, 1]                      # not in time order; slots 0 and 4 share step 1


@STORAGES
@pytest.mark.parametrize("factor", [0, 2])
@pytest.mark.parametrize("forced", [False, True], ids=["free", "forced"])
def test_a_windowed_run_is_the_sequence(forced, factor, storage):
    from fluidsimulationcuda_amd import capi
    torch = torch_()
    n, members, p, iters, nsteps, every = 14, 5, 130, 4, 4, 2
    stride, kept = p + 3, ("dens", "u")
    w = n + 2
    side = w // factor if factor else w
    coarse = factor or None
    rng = np.random.default_rng(55000 + 100 * factor + 10 * forced + storage)
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in OB.MAIN}
    cols, rows = OB.network(n, p, rng)
    names = NW.fields_of(p, NW.FIVE)
    dt = np.linspace(0.01, 0.02, members).astype(F32)
    diff = np.linspace(0.05, 0.15, members).astype(F32)
    visc = np.linspace(0.002, 0.003, members).astype(F32)
    sources = device(rng.uniform(0.0, 0.5, (3, members, w, w)).astype(F32)) if forced else None
    empty = pattern(members, p, stride)
    slots = [(SLOT_FIRST[k], SLOT_FIRST[k + 1] - SLOT_FIRST[k], SLOT_STEP[k]) for k in range(len(SLOT_STEP))]
    assert sorted(SLOT_STEP) == [0, 1, 1, 3, 4] and any(count == 0 for _, count, _ in slots)
    with OB.solver(n, members, storage) as a, OB.solver(n, members, storage) as b:
        for s in (a, b):
            s.upload_members(**fields)
            s.set_observation_network(cols, rows, names)
        record, snaps, written = a.run_window(nsteps, SLOT_FIRST, SLOT_STEP, record=device(empty), member_stride=stride, every=every,
                                              fields=kept, sources=sources, dt=dt, diff=diff, visc=visc, iters=iters, use_sources=True,
                                              coarse=coarse, wait=False)
        want_record = device(empty)
        want_snaps = torch.zeros((nsteps // every, len(kept), members, side, side), dtype=torch.float32, device="cuda")

        def observe_due(done):
            for first, count, step in slots:
                if step == done:
                    b.observe_range(first, count, want_record, member_stride=stride)

        observe_due(0)
        for z in range(nsteps):
            b.run(1, sources=sources, dt=dt, diff=diff, visc=visc, iters=iters, use_sources=z == 0)
            if (z + 1) % every == 0:
                for k, f in enumerate(kept):
                    b.pack(f, out=want_snaps[(z + 1) // every - 1, k], coarse=coarse)
            observe_due(z + 1)
        a.synchronize()
        what = "forced=%s factor=%d storage=%d" % (forced, factor, storage)
        assert written == nsteps // every and tuple(snaps.shape) == tuple(want_snaps.shape)
        got, want = bits(record), bits(want_record)
        assert np.array_equal(got, want), "%s: %d floats of the record differ" % (what, int((got != want).sum()))
        written_to = got != empty.view(np.uint32)
        for m in range(members):
            row = written_to[m * stride:m * stride + p]
            assert not row[:3].any() and not row[127:].any() and row[3:127].all(), what + ": the points of the slots, and no other"
            assert not written_to[m * stride + p:(m + 1) * stride].any(), what + ": the gap"
        assert np.array_equal(bits(snaps), bits(want_snaps)), what + ": the snapshots"
        EK.same_members(a, b, capi.FIELD_NAMES, what)
        # no slots: the plain run
        _, _, none = a.run_window(1, [], [], record=record, member_stride=stride, dt=dt, diff=diff, visc=visc, iters=iters)
        b.run(1, dt=dt, diff=diff, visc=visc, iters=iters)
        assert none == 0 and np.array_equal(bits(record), want)
        EK.same_members(a, b, capi.FIELD_NAMES, what + ": no slots")


# ---- 6. poisoning ------------------------------------------------------------------------------------------------------------------------
@STORAGES
def test_a_nan_in_the_record_poisons_what_a_nan_observation_would(storage):
    n, members, p, bad, at = 30, 5, 130, 2, 100
    lat, c = ((1, 3), (15, -1), 16), 8.0                  # nodes on row 15, columns -1, 15, 31; supports of radius 16
    rng = np.random.default_rng(56000 + storage)
    w = n + 2
    cols, rows = OB.network(n, p, rng)
    cols[at], rows[at] = 8.25, 15.5
    y, sg = rng.normal(size=p).astype(F32), rng.uniform(0.5, 2.0, p).astype(F32)
    wt, _, _ = LG.weights(cols, rows, *lat, c)
    assert wt[0, 0, at] != 0 and wt[0, 1, at] != 0 and wt[0, 2, at] == 0
    keep = np.ones((members, members), bool)
    keep[bad] = keep[:, bad] = False
    with OB.solver(n, members, storage) as s:
        s.upload_members(dens=rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32))
        s.set_observation_points(cols, rows)
        record = s.observe_device("dens")
        rec = FromRecord(s)
        clean_g = {centre: s.observation_gram_recorded(record, obs=y, inv_sigma=sg, centre=centre) for centre in (False, True)}
        clean = {centre: LG.call(rec, record, lat, c, y, sg, centre) for centre in (False, True)}
        assert all(np.isfinite(v).all() for k in clean for v in clean[k][:3]) and all(np.isfinite(clean_g[k][0]).all() for k in clean_g)
        record[bad, at] = float("nan")
        torch_().cuda.synchronize()
        g, rhs, dd = s.observation_gram_recorded(record, obs=y, inv_sigma=sg, centre=False)
        assert np.isnan(g[bad]).all() and np.isnan(g[:, bad]).all() and np.isnan(rhs[bad])
        assert np.array_equal(g.view(np.uint64)[keep], clean_g[False][0].view(np.uint64)[keep]), "a NaN in member 2 changed another entry"
        assert np.array_equal(np.delete(rhs, bad).view(np.uint64), np.delete(clean_g[False][1], bad).view(np.uint64))
        assert dd == clean_g[False][2]
        g, rhs, dd = s.observation_gram_recorded(record, obs=y, inv_sigma=sg, centre=True)
        assert np.isnan(g).all() and np.isnan(rhs).all() and np.isnan(dd)
        gram, rhs, dd, counts = LG.call(rec, record, lat, c, y, sg, False)
        for node in (0, 1):
            g = gram[0, node]
            assert np.isnan(g[bad]).all() and np.isnan(g[:, bad]).all() and np.isnan(rhs[0, node, bad])
            assert np.array_equal(g.view(np.uint64)[keep], clean[False][0][0, node].view(np.uint64)[keep]), "a NaN in member 2 changed another entry"
            assert np.array_equal(np.delete(rhs[0, node], bad).view(np.uint64), np.delete(clean[False][1][0, node], bad).view(np.uint64))
            LG.same_bits(dd[0, node], clean[False][2][0, node], "dd")
        for v, ref in zip((gram, rhs, dd), clean[False][:3]):
            LG.same_bits(v[0, 2], ref[0, 2], "centre=False: the node that does not see the point")
        gram, rhs, dd, counts = LG.call(rec, record, lat, c, y, sg, True)
        assert np.isnan(gram[0, :2]).all() and np.isnan(rhs[0, :2]).all() and np.isnan(dd[0, :2]).all()
        for v, ref in zip((gram, rhs, dd), clean[True][:3]):
            LG.same_bits(v[0, 2], ref[0, 2], "centre=True: the node that does not see the point")
        assert np.array_equal(counts, clean[True][3])
        # the recipe for a point that was left out: a zero in the record and inv_sigma 0 -- the point adds +0 to every sum
        record[bad, at] = 0.0
        torch_().cuda.synchronize()
        out = sg.copy()
        out[at] = 0.0
        g, rhs, dd = s.observation_gram_recorded(record, obs=y, inv_sigma=out, centre=True)
        assert np.isfinite(g).all() and np.isfinite(rhs).all() and np.isfinite(dd)


# ---- 7. refusals change nothing -----------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    torch = torch_()
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(57)
    n, members, p = 6, 5, 65
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in OB.MAIN}
    cols, rows = OB.network(n, p, rng)
    dp, fp, ip = C.POINTER(C.c_double), capi._MF, C.POINTER(C.c_int)
    gram, rhs, dd = np.full((members, members), 7.0), np.full(members, 7.0), np.full(1, 7.0)
    lgram, lrhs, ldd, lcounts = np.full((2, 2, members, members), 7.0), np.full((2, 2, members), 7.0), np.full((2, 2), 7.0), np.full((2, 2), 7, np.int32)
    dev = torch.full((members * p,), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    host = np.full(members * p, 7.0, F32)
    ones = np.ones(p, F32)
    par = np.full(members, 0.01, F32)
    listed = (C.c_int * 3)(0, 1, 2)
    g = lambda a: a.ctypes.data_as(dp)
    f = lambda a: a.ctypes.data_as(fp)
    i = lambda a: a.ctypes.data_as(ip)
    FOP = capi.FIELD_OF_POINT
    hip = OB.hip_runtime()
    exact, size = C.c_void_p(), 1 << 20
    assert hip.hipMalloc(C.byref(exact), C.c_size_t(size)) == 0
    short = exact.value + size - members * p * 4 + 4       # a record that ends one float past its allocation

    def refused(rc, *words):
        assert rc == capi.E_INVALID
        msg = L.fluid_last_error()
        assert all(word in msg for word in words), msg

    plan = capi.RunPlan(iters=4, nsteps=2)

    def window(field=2, first=(0, 30, p), step=(0, 2), record=None, stride=0, nslots=None):
        a, b = (C.c_int * len(first))(*first), (C.c_int * len(step))(*step)
        win = capi.ObsWindow(field=field, nslots=len(step) if nslots is None else nslots, slot_first=a, slot_step=b,
                             record_dev=dev.data_ptr() if record is None else record, member_stride=stride)
        win.keep = (a, b)
        return win

    def run(s, win, the_plan=plan, factor=0):
        return L.fluid_run_window(s._h, f(par), f(par), f(par), C.byref(the_plan), factor, C.byref(win), None)

    def the_five(s, *words, field=2, record=None, stride=0):
        """what all five refuse: the record and the state of the context"""
        r = dev.data_ptr() if record is None else record
        refused(L.fluid_observe_members_range(s._h, field, 0, 1, r, stride), b"fluid_observe_members_range", *words)
        refused(run(s, window(field=field, record=r, stride=stride)), b"fluid_run_window", *words)
        refused(L.fluid_observation_gram_recorded(s._h, r, stride, 1, f(ones), None, g(gram), g(rhs), g(dd)), b"fluid_observation_gram_recorded:", *words)
        refused(L.fluid_observation_gram_lattice_recorded(s._h, r, stride, 1, f(ones), None, 2, 2, 0, 0, 8, 4.0, g(lgram), g(lrhs), g(ldd), i(lcounts)),
                b"fluid_observation_gram_lattice_recorded:", *words)
        refused(L.fluid_analyse_lattice_recorded(s._h, r, stride, f(ones), None, 2, 2, 0, 0, 8, 4.0, 1.0, listed, 3),
                b"fluid_analyse_lattice_recorded:", *words)

    with OB.solver(n, members) as s, OB.solver(n, members) as twin:
        for c in (s, twin):
            c.timing_enable(True)
            c.upload_members(**fields)
            c.step(use_sources=True)
            c.add_source("dens", "dens_prev", OB.DT)                   # a lazy state that must survive the refusals
        the_five(s, b"no observation network")
        s.set_observation_points(cols, rows)
        # the record
        the_five(s, b"member_stride 64", b"65", stride=p - 1)
        the_five(s, b"record_dev", b"not device memory", record=host.ctypes.data)
        the_five(s, b"record_dev", record=short)
        # the field of the two observing calls
        for field in (12, -1, -3):
            refused(L.fluid_observe_members_range(s._h, field, 0, 1, dev.data_ptr(), 0), b"fluid_observe_members_range", b"bad field id %d" % field)
            refused(run(s, window(field=field)), b"fluid_run_window", b"bad field id %d" % field)
        refused(L.fluid_observe_members_range(s._h, FOP, 0, 1, dev.data_ptr(), 0), b"fluid_observe_members_range", b"typed network")
        refused(run(s, window(field=FOP)), b"fluid_run_window", b"typed network")
        # the range
        for first, count in ((-1, 1), (p + 1, 0), (0, -1), (0, p + 1), (p, 1), (64, 2), (1, 2 ** 31 - 1)):
            refused(L.fluid_observe_members_range(s._h, 2, first, count, dev.data_ptr(), 0), b"fluid_observe_members_range", b"%d" % first, b"%d" % count)
        # the window
        refused(run(s, window(first=(-1, 30, p))), b"fluid_run_window", b"slot 0")
        refused(run(s, window(first=(0, 30, 29))), b"fluid_run_window", b"slot 1")
        refused(run(s, window(first=(0, 30, p + 1))), b"fluid_run_window", b"slot 1", b"65")
        refused(run(s, window(step=(0, 3))), b"fluid_run_window", b"slot 1", b"nsteps = 2")
        refused(run(s, window(step=(-1, 2))), b"fluid_run_window", b"slot 0")
        refused(run(s, window(nslots=-1)), b"fluid_run_window", b"nslots = -1", b"65536")
        refused(run(s, window(nslots=capi.WINDOW_MAX_SLOTS + 1)), b"fluid_run_window", b"65537", b"65536")
        # the namesakes' own refusals, under the new names
        refused(run(s, window(), capi.RunPlan(iters=3, nsteps=2)), b"fluid_run_window", b"sweep count")
        refused(run(s, window(), capi.RunPlan(iters=4, nsteps=-1)), b"fluid_run_window", b"nsteps")
        refused(run(s, window(), plan, factor=3), b"fluid_run_window", b"factor 3")
        bad = par.copy()
        bad[3] = np.inf
        refused(L.fluid_run_window(s._h, f(par), f(bad), f(par), C.byref(plan), 0, C.byref(window()), None), b"fluid_run_window", b"member 3", b"diff")
        sig = ones.copy()
        sig[17] = np.inf
        refused(L.fluid_observation_gram_recorded(s._h, dev.data_ptr(), 0, 1, f(ones), f(sig), g(gram), g(rhs), g(dd)),
                b"fluid_observation_gram_recorded:", b"inv_sigma[17]")
        refused(L.fluid_observation_gram_lattice_recorded(s._h, dev.data_ptr(), 0, 1, f(ones), None, 2, 2, 0, 0, 12, 4.0, g(lgram), g(lrhs), g(ldd),
                                                          i(lcounts)), b"fluid_observation_gram_lattice_recorded:", b"step = 12")
        refused(L.fluid_analyse_lattice_recorded(s._h, dev.data_ptr(), 0, f(ones), None, 2, 2, 0, 0, 8, 4.0, -1.0, listed, 3),
                b"fluid_analyse_lattice_recorded:", b"rho")
        refused(L.fluid_analyse_lattice_recorded(s._h, dev.data_ptr(), 0, f(ones), None, 2, 2, 0, 0, 8, 4.0, 1.0, (C.c_int * 2)(1, 1), 2),
                b"fluid_analyse_lattice_recorded:", b"listed twice")
        assert (gram == 7.0).all() and (rhs == 7.0).all() and (dd == 7.0).all() and (host == 7.0).all()
        assert (lgram == 7.0).all() and (lrhs == 7.0).all() and (ldd == 7.0).all() and (lcounts == 7).all()
        assert (dev.cpu().numpy() == 7.0).all()
        ta, tb = s.timing_read(reset=False), twin.timing_read(reset=False)
        assert ta == {**tb, **{k: ta[k] for k in ta if k.endswith("_ms")}}             # every count; the times are times
        for name in capi.FIELD_NAMES:
            assert np.array_equal(s.download_members(name).view(np.uint32), twin.download_members(name).view(np.uint32)), name
        # a record that ends with its allocation is taken
        fits = short - 4
        assert L.fluid_observe_members_range(s._h, 2, 0, p, fits, 0) == capi.OK
        s.synchronize()
    assert hip.hipFree(exact) == 0
    # more members than the recorded calls take; the two observing calls take them
    many = capi.TRANSFORM_MAX_MEMBERS + 1
    big = torch.full((many * p,), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gram = np.full((many, many), 7.0)
    with OB.solver(n, many) as s:
        s.set_observation_points(cols, rows)
        refused(L.fluid_observation_gram_recorded(s._h, big.data_ptr(), 0, 1, f(ones), None, g(gram), None, None),
                b"fluid_observation_gram_recorded:", b"65 members", b"64")
        refused(L.fluid_observation_gram_lattice_recorded(s._h, big.data_ptr(), 0, 0, None, None, 1, 1, 0, 0, 8, 4.0, g(gram), None, None, None),
                b"fluid_observation_gram_lattice_recorded:", b"65 members", b"64")
        refused(L.fluid_analyse_lattice_recorded(s._h, big.data_ptr(), 0, f(ones), None, 1, 1, 0, 0, 8, 4.0, 1.0, listed, 3),
                b"fluid_analyse_lattice_recorded:", b"65 members", b"64")
        assert (gram == 7.0).all() and (big.cpu().numpy() == 7.0).all()
        s.observe_range(0, p, big, "dens")
        assert (big.cpu().numpy() == 0.0).all()
    # row slabs
    with OB.F().FluidSolver(n, rank=0, nranks=2) as s:
        one = torch.full((4,), 7.0, dtype=torch.float32, device="cuda")
        gram = np.full((1, 1), 7.0)
        refused(L.fluid_observe_members_range(s._h, 2, 0, 1, one.data_ptr(), 0), b"fluid_observe_members_range", b"slab")
        refused(L.fluid_run_window(s._h, f(par), f(par), f(par), C.byref(plan), 0, C.byref(window(record=one.data_ptr())), None),
                b"fluid_run_window", b"slab")
        refused(L.fluid_observation_gram_recorded(s._h, one.data_ptr(), 0, 1, None, None, g(gram), None, None), b"fluid_observation_gram_recorded:", b"slab")
        refused(L.fluid_observation_gram_lattice_recorded(s._h, one.data_ptr(), 0, 1, None, None, 1, 1, 0, 0, 8, 4.0, g(gram), None, None, None),
                b"fluid_observation_gram_lattice_recorded:", b"slab")
        refused(L.fluid_analyse_lattice_recorded(s._h, one.data_ptr(), 0, f(ones), None, 1, 1, 0, 0, 8, 4.0, 1.0, listed, 3),
                b"fluid_analyse_lattice_recorded:", b"slab")
        assert (one.cpu().numpy() == 7.0).all() and gram[0, 0] == 7.0
