"""GPU: screening observations -- fluid_observation_departures(_recorded), fluid_set_observation_qc, fluid_observation_qc_result
(include/fluid_amd.h, "screening observations").

Every expected value comes from tests/qc_model.py, the header's rules in numpy float64 one rounding per line, fed what
`observe()` shows; means, spreads, departures, ranks, flags and the three sums are compared bit for bit.  The sums are also held
against math.fsum: `==` on dyadic data, where every partial sum is representable, and on general data within the bound
tests/test_gpu_observe.py derives for a recursive double sum (`OB.gamma`).  The gate is held to its contract: a gated call is the
ungated call with inv_sigma zeroed at the model's flags, bit for bit, in every result and every field of every member."""
import ctypes as C
import math

import numpy as np
import pytest

import qc_model as QC
import test_gpu_etkf as EK
import test_gpu_network as NW
import test_gpu_observe as OB
import test_gpu_window as WD

pytestmark = pytest.mark.gpu
F32 = np.float32
STORAGES = pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
SIZES = [6, 30]
MEMBERS = [2, 5, 9, 33, 64]                 # the bye member, both sides of the padding at 8, past a padded count, the cap
POINTS = [1, 63, 65, 130]                   # the edges of a chunk of 64 points
THRESHOLDS = [0.0, 3.0, 5.0]
THREE = ("dens", "u", "u_prev")             # fp16 storage: u_prev, the pressure of a vel_step, is held at a scale
LATTICE = ((3, 3), (-8, 0), 16)             # n = 30: nodes on rows -8, 8, 24 and columns 0, 16, 32
HALF_WIDTH = 6.0


def ensemble(n, members, storage, rng):
    """a context after a vel_step, every field of order 1 with a spread of order 1"""
    w = n + 2
    s = OB.solver(n, members, storage)
    s.upload_members(dens=rng.uniform(-4.0, 4.0, (members, w, w)).astype(F32), u=rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32),
                     v=rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32))
    s.vel_step()
    return s


class Source:
    """where a call's h comes from: a field of an untyped network, the points' own fields of a typed one, or a record"""

    def __init__(self, field=None, record=None, stride=0):
        self.field, self.record, self.stride = field, record, stride

    def departures(self, s, **kw):
        return s.observation_departures(field=self.field, record=self.record, member_stride=self.stride, **kw)

    def gram(self, s, **kw):
        if self.record is None:
            return s.observation_gram(self.field, **kw)
        return s.observation_gram_recorded(self.record, member_stride=self.stride, **kw)

    def lattice(self, s, **kw):
        shape, origin, step = LATTICE
        if self.record is None:
            return s.observation_gram_lattice(self.field, shape, origin, step, HALF_WIDTH, **kw)
        return s.observation_gram_lattice_recorded(self.record, shape, origin, step, HALF_WIDTH, member_stride=self.stride, **kw)

    def analyse(self, s, y, **kw):
        shape, origin, step = LATTICE
        if self.record is None:
            return s.analyse_lattice(self.field, shape, origin, step, HALF_WIDTH, y, **kw)
        return s.analyse_lattice_recorded(self.record, shape, origin, step, HALF_WIDTH, y, member_stride=self.stride, **kw)


def sources(solvers, n, p, rng, kinds):
    """sets the network of every solver per kind and yields (kind, Source, h): h (M, P) is what solvers[0] observes now"""
    cols, rows = OB.network(n, p, rng)
    for kind in kinds:
        names = NW.fields_of(p, THREE) if kind == "typed" else None
        for s in solvers:
            s.set_observation_network(cols, rows, names)
        if kind == "typed":
            yield kind, Source(), solvers[0].observe(None)
        elif kind.startswith("record"):
            h = solvers[0].observe("dens")
            stride = p + int(kind[6:])
            yield kind, Source(record=WD.record_of(h, stride), stride=stride), h
        else:
            yield kind, Source(kind), solvers[0].observe(kind)


def planted(h, rng):
    """(y, inv_sigma, gross): observations at mean + (0.5 .. 1) sd on either side, ties y = h_k exactly at every seventh point,
    gross errors of 100 sd at up to three points; 1 / sigma of the order of 1 / sd, so that a gross error is one at any threshold
    here -- 10^4 sd^2 s^2 against t^2 (1 + sd^2 s^2), sd s >= 0.5 -- and nothing else is."""
    members, p = h.shape
    mean, var = QC.moments(h)
    assert np.isfinite(h).all()
    sd = np.where(var > 0, np.sqrt(var), 1.0)                            # (the members agree, as u does on a wall: any scale serves)
    y = (mean + rng.uniform(0.5, 1.0, p) * rng.choice([-1.0, 1.0], p) * sd).astype(F32)
    ties = np.arange(p) % 7 == 3
    nearest = np.abs(h.astype(np.float64) - mean).argmin(axis=0)        # (the member next to the mean: a tie is no outlier)
    y[ties] = h[nearest, np.arange(p)][ties]
    gross = np.zeros(p, bool)
    gross[[0, p // 2, p - 1]] = True
    y[gross] = (mean + 100.0 * sd * rng.choice([-1.0, 1.0], p)).astype(F32)[gross]
    sg = (rng.uniform(0.5, 2.0, p) / sd).astype(F32)
    return y, sg, gross


def same_screen(got, want, what):
    for key in ("mean", "spread", "departure", "sums"):
        if key in want:
            OB.same_bits(got[key], want[key], "%s: %s" % (what, key))
    for key in ("rank", "flag"):
        if key in want:
            assert got[key].dtype == np.uint8 and np.array_equal(got[key], want[key]), "%s: %s" % (what, key)
    assert set(got) == set(want) - {"d", "vs"}, what


# ---- 1. departures against the model, bit for bit ----------------------------------------------------------------------------------
@STORAGES
@pytest.mark.parametrize("members", MEMBERS)
def test_departures_against_the_model(members, storage):
    rng = np.random.default_rng(51000 + 100 * members + storage)
    for n in SIZES:
        with ensemble(n, members, storage, rng) as s:
            for p in POINTS:
                for kind, src, h in sources([s], n, p, rng, ("dens", "u_prev", "typed", "record0", "record3")):
                    y, sg, gross = planted(h, rng)
                    what = "n=%d M=%d storage=%d P=%d %s" % (n, members, storage, p, kind)
                    same_screen(src.departures(s), QC.screen(h), what + ": no obs")
                    for threshold in THRESHOLDS:
                        for sigma in (sg, None):
                            w = "%s t=%g sigma=%s" % (what, threshold, sigma is not None)
                            want = QC.screen(h, y, sigma, threshold)
                            same_screen(src.departures(s, obs=y, inv_sigma=sigma, threshold=threshold), want, w)
                            if sigma is not None:
                                assert np.array_equal(want["flag"] != 0, gross & (threshold > 0)), w + ": the model flags the planted points"
                    ties = np.arange(p) % 7 == 3
                    assert (want["rank"] <= members).all() and ((want["rank"] < members) | ~ties | gross).all()     # a tie is not below


# ---- 2. the sums ----------------------------------------------------------------------------------------------------------------------
@STORAGES
@pytest.mark.parametrize("members", [2, 64])
def test_sums_exact_on_dyadic_data(members, storage):
    """a power of two of members: the mean, the departures and their squares are dyadic, every partial sum is representable;
    two members: the variance is, too"""
    rng = np.random.default_rng(52000 + 100 * members + storage)
    n = 13
    with OB.solver(n, members, storage) as a, OB.solver(n, members, storage) as b:
        for p in POINTS + [64 * 16 + 70]:                               # ... and more chunks than the fold has lanes
            x, cols, rows, y, sg = OB.dyadic_case(rng, n, members, p)
            y[::5] += F32(64.0)                                         # rejected at threshold 3: |d| >= 24, var s^2 <= 4
            for c in (a, b):
                c.upload_members(dens=x)
                c.set_observation_points(cols, rows)
            h = a.observe("dens")
            for threshold in (0.0, 3.0):
                what = "M=%d storage=%d P=%d t=%g" % (members, storage, p, threshold)
                want = QC.screen(h, y, sg, threshold)
                keep = want["flag"] == 0
                assert keep.all() if threshold == 0 else not keep[::5].any(), what
                got = a.observation_departures("dens", obs=y, inv_sigma=sg, threshold=threshold)
                assert got["sums"][0] == keep.sum() and got["sums"][1] == math.fsum(want["d"][keep] ** 2), what
                if members == 2:
                    assert got["sums"][2] == math.fsum(want["vs"][keep]), what
                same_screen(got, want, what)
                OB.same_bits(a.observation_departures("dens", obs=y, inv_sigma=sg, threshold=threshold)["sums"], got["sums"], what + ": two calls")
                OB.same_bits(b.observation_departures("dens", obs=y, inv_sigma=sg, threshold=threshold)["sums"], got["sums"], what + ": two contexts")


@STORAGES
@pytest.mark.parametrize("n,members,p", [(6, 5, 65), (30, 9, 130), (30, 33, 63), (6, 64, 130), (30, 2, 64 * 16 + 70)])
def test_sums_general_data_within_the_summation_bound(n, members, p, storage):
    rng = np.random.default_rng(53000 + 100 * members + storage)
    with ensemble(n, members, storage, rng) as a, ensemble(n, members, storage, np.random.default_rng(1)) as b:
        for kind, src, h in sources([a], n, p, rng, ("dens", "typed", "record3")):
            y, sg, gross = planted(h, rng)
            for threshold in THRESHOLDS:
                what = "n=%d M=%d P=%d storage=%d %s t=%g" % (n, members, p, storage, kind, threshold)
                want = QC.screen(h, y, sg, threshold)
                keep = want["flag"] == 0
                got = src.departures(a, obs=y, inv_sigma=sg, threshold=threshold)["sums"]
                assert got[0] == keep.sum(), what
                for k, terms in ((1, want["d"][keep] ** 2), (2, want["vs"][keep])):         # (terms >= 0: the sum of |terms| is the sum)
                    exact = math.fsum(terms)
                    err, bound = abs(got[k] - exact), OB.gamma(p) * exact
                    print("%s: sum %d: error / bound = %.4f" % (what, k, err / bound))
                    assert err <= bound, what
                OB.same_bits(src.departures(a, obs=y, inv_sigma=sg, threshold=threshold)["sums"], got, what + ": two calls")
                if kind == "record3":                                    # a second context, with other fields: the record is what is read
                    b.set_observation_points(*OB.network(n, p, rng))
                    OB.same_bits(src.departures(b, obs=y, inv_sigma=sg, threshold=threshold)["sums"], got, what + ": two contexts")


# ---- 3. the gate ----------------------------------------------------------------------------------------------------------------------
def pack_lattice(got):
    return np.concatenate([np.asarray(v, np.float64).ravel() for v in got])


@STORAGES
@pytest.mark.parametrize("members", MEMBERS)
def test_a_gated_call_is_the_call_with_inv_sigma_zeroed_at_the_flags(members, storage):
    from fluidsimulationcuda_amd import capi
    n, p, threshold = 30, 130, 3.0
    rng = np.random.default_rng(54000 + 100 * members + storage)
    fields = EK.start_fields(n, members, rng)
    with OB.solver(n, members, storage) as a, OB.solver(n, members, storage) as b, OB.solver(n, members, storage) as plain:
        for s in (a, b, plain):
            s.upload_members(**fields)
            s.step(2, use_sources=True)                    # fp16: the pressure scale is live; the sources are marked zero
        a.set_observation_qc(threshold)
        assert a.observation_qc() == threshold and b.observation_qc() == 0.0
        for kind, src, h in sources([a, b, plain], n, p, rng, ("dens", "typed", "record3")):
            for given in (True, False):
                what = "M=%d storage=%d %s sigma=%s" % (members, storage, kind, given)
                h = a.observe(src.field) if src.record is None else h       # (an analysis has moved the fields since)
                y, sg, gross = planted(h, rng)
                sigma = sg if given else None
                zeroed, flag = QC.gated_inv_sigma(h, y, sigma, threshold)
                if given:
                    assert np.array_equal(flag != 0, gross), what + ": the flags are the planted points"
                for centre in (True, False):
                    OB.same_bits(OB.pack_results(members, src.gram(a, obs=y, inv_sigma=sigma, centre=centre)),
                                 OB.pack_results(members, src.gram(b, obs=y, inv_sigma=zeroed, centre=centre)), "%s: gram centre=%s" % (what, centre))
                    got = a.observation_qc_result()
                    assert np.array_equal(got[0], flag) and got[1:] == (p, int(flag.sum())), what
                    ga, gb = src.lattice(a, obs=y, inv_sigma=sigma, centre=centre), src.lattice(b, obs=y, inv_sigma=zeroed, centre=centre)
                    OB.same_bits(pack_lattice(ga[:3]), pack_lattice(gb[:3]), "%s: lattice gram centre=%s" % (what, centre))
                    assert np.array_equal(ga[3], gb[3]) and ga[3].sum() > 0, what + ": counts"
                    assert np.array_equal(a.observation_qc_result()[0], flag), what
                if given and kind == "dens":                # the ungated analysis of the same state, for the difference
                    EK.same_members(a, plain, capi.FIELD_NAMES, what + ": before the analysis")
                    src.analyse(plain, y, inv_sigma=sigma, rho=1.1, fields=("dens", "u", "v"))
                src.analyse(a, y, inv_sigma=sigma, rho=1.1, fields=("dens", "u", "v"), wait=False)
                src.analyse(b, y, inv_sigma=zeroed, rho=1.1, fields=("dens", "u", "v"), wait=False)
                assert a.analyse_status() == b.analyse_status() and a.analyse_status()["solved"] >= 4, what
                got = a.observation_qc_result()
                assert np.array_equal(got[0], flag) and got[1:] == (p, int(flag.sum())), what + ": after the analysis"
                EK.same_members(a, b, capi.FIELD_NAMES, what + ": the analysis")
                if given and kind == "dens":
                    assert not np.array_equal(a.download_members("dens").view(np.uint32), plain.download_members("dens").view(np.uint32)), \
                        what + ": the gate changed nothing"
        assert a.observation_qc() == threshold                           # the value survives every new network


def test_a_node_whose_points_are_all_rejected_is_solved_with_a_zero_gram():
    n, members, p = 30, 5, 65
    rng = np.random.default_rng(55000)
    fields = EK.start_fields(n, members, rng)
    cols, rows = rng.uniform(6.0, 10.0, p).astype(F32), rng.uniform(6.0, 10.0, p).astype(F32)      # all within reach of node (8, 8) only
    with OB.solver(n, members) as s:
        s.upload_members(**fields)
        s.set_observation_points(cols, rows)
        before = WD.snapshot(s, EK.MAIN)
        h = s.observe("dens")
        mean, var = QC.moments(h)
        y = (mean + 100.0 * np.sqrt(var) + 100.0).astype(F32)
        s.set_observation_qc(3.0)
        s.analyse_lattice("dens", (1, 1), (8, 8), 8, 4.0, y, rho=1.0, fields=("dens", "u", "v"))
        assert s.analyse_status() == {"solved": 1, "empty": 0, "failed": 0}
        flags, checked, rejected = s.observation_qc_result()
        assert flags.all() and (checked, rejected) == (p, p)
        WD.unchanged(s, before, "D = 0 at rho = 1")


# ---- 4. threshold 0 after a non-zero one; a call without obs ---------------------------------------------------------------------------
@STORAGES
def test_threshold_zero_restores_the_ungated_bits_and_a_call_without_obs_checks_nothing(storage):
    from fluidsimulationcuda_amd import capi
    n, members, p = 30, 9, 130
    rng = np.random.default_rng(56000 + storage)
    with ensemble(n, members, storage, rng) as a, ensemble(n, members, storage, np.random.default_rng(56000 + storage)) as b:
        (kind, src, h), = sources([a, b], n, p, rng, ("dens",))
        y, sg, gross = planted(h, rng)
        with pytest.raises(capi.FluidError, match="fluid_observation_qc_result.*no gated call"):
            a.observation_qc_result()
        ungated = OB.pack_results(members, src.gram(b, obs=y, inv_sigma=sg))
        a.set_observation_qc(5.0)
        gated = OB.pack_results(members, src.gram(a, obs=y, inv_sigma=sg))
        assert not np.array_equal(gated.view(np.uint64), ungated.view(np.uint64))
        flags = a.observation_qc_result()
        assert np.array_equal(flags[0] != 0, gross)
        # a call without obs checks nothing, gives the ungated bits and leaves the last result in place
        OB.same_bits(src.gram(a, inv_sigma=sg), src.gram(b, inv_sigma=sg), "obs null under the gate")
        OB.same_bits(src.lattice(a, inv_sigma=sg)[0], src.lattice(b, inv_sigma=sg)[0], "obs null under the gate: lattice")
        again = a.observation_qc_result()
        assert np.array_equal(again[0], flags[0]) and again[1:] == flags[1:]
        # departures do not touch the gate or its result
        src.departures(a, obs=y + F32(1000.0), inv_sigma=sg, threshold=1.0)
        assert np.array_equal(a.observation_qc_result()[0], flags[0]) and a.observation_qc() == 5.0
        a.set_observation_qc(0.0)
        OB.same_bits(OB.pack_results(members, src.gram(a, obs=y, inv_sigma=sg)), ungated, "threshold 0 after 5")
        OB.same_bits(OB.pack_results(members, src.gram(a, obs=y)), OB.pack_results(members, src.gram(b, obs=y)), "threshold 0, sigma null")
        OB.same_bits(pack_lattice(src.lattice(a, obs=y, inv_sigma=sg)[:3]), pack_lattice(src.lattice(b, obs=y, inv_sigma=sg)[:3]), "threshold 0: lattice")
        assert np.array_equal(a.observation_qc_result()[0], flags[0])    # still the last gated call's
        # the threshold survives a new network; the result does not
        a.set_observation_qc(3.0)
        a.set_observation_points(*OB.network(n, 65, rng))
        assert a.observation_qc() == 3.0
        with pytest.raises(capi.FluidError, match="fluid_observation_qc_result.*no gated call"):
            a.observation_qc_result()


# ---- 5. poisoning ---------------------------------------------------------------------------------------------------------------------
@STORAGES
def test_the_gated_call_poisons_what_the_zeroed_call_poisons(storage):
    n, members, p, bad = 30, 5, 130, 2
    rng = np.random.default_rng(57000 + storage)
    w = n + 2
    x = rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32)
    cols, rows = OB.network(n, p, rng)
    with OB.solver(n, members, storage) as a, OB.solver(n, members, storage) as b:
        for s in (a, b):
            s.upload_members(dens=x)
            s.set_observation_points(cols, rows)
        y, sg, gross = planted(a.observe("dens"), rng)
        i0, j0 = rows.astype(np.int64), cols.astype(np.int64)
        near = lambda q: (np.abs(i0 - i0[q]) <= 1) & (np.abs(j0 - j0[q]) <= 1)     # (a superset of the stencils that hold q's first tap)
        q = next(q for q in range(p) if not (near(q) & gross).any() and near(q).sum() < p // 2)
        x[bad, i0[q], j0[q]] = np.nan                                    # a NaN tap: the points whose stencil holds it
        for s in (a, b):
            s.upload_members(dens=x)
        h = a.observe("dens")
        hit = np.isnan(h).any(axis=0)
        assert hit.any() and not hit.all() and not (hit & gross).any()
        free = np.flatnonzero(~hit & ~gross)
        y[free[0]], y[free[1]] = np.nan, np.inf                          # a NaN obs rejects nothing; an inf obs is rejected, and inf * 0 is NaN
        a.set_observation_qc(3.0)
        src = Source("dens")
        for sigma in (sg, None):
            zeroed, flag = QC.gated_inv_sigma(h, y, sigma, 3.0)
            assert not flag[hit].any() and flag[free[0]] == 0 and flag[free[1]] == 1 and flag[gross].all()
            for centre in (False, True):
                what = "storage=%d sigma=%s centre=%s" % (storage, sigma is not None, centre)
                ga, gb = src.gram(a, obs=y, inv_sigma=sigma, centre=centre), src.gram(b, obs=y, inv_sigma=zeroed, centre=centre)
                OB.same_bits(OB.pack_results(members, ga), OB.pack_results(members, gb), what)
                assert np.isnan(ga[1]).all() and np.isnan(ga[2]) and np.isnan(ga[0][bad]).all(), what
                assert centre or np.isfinite(np.delete(np.delete(ga[0], bad, 0), bad, 1)).all(), what
                la, lb = src.lattice(a, obs=y, inv_sigma=sigma, centre=centre), src.lattice(b, obs=y, inv_sigma=zeroed, centre=centre)
                OB.same_bits(pack_lattice(la[:3]), pack_lattice(lb[:3]), what + ": lattice")
                assert np.array_equal(a.observation_qc_result()[0], flag), what
            same_screen(src.departures(a, obs=y, inv_sigma=sigma, threshold=3.0), QC.screen(h, y, sigma, 3.0), "departures with NaNs")


# ---- 6. lazy state --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,case", [(0, "pending"), (0, "zeros"), (1, "scaled"), (1, "pending"), (1, "zeros")])
def test_lazy_state_is_settled_and_nothing_is_altered(storage, case):
    from fluidsimulationcuda_amd import capi
    members, n, p = 3, 30, 130
    rng = np.random.default_rng(58000 * (storage + 1) + len(case))
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in OB.MAIN}
    cols, rows = OB.network(n, p, rng)
    y = rng.normal(size=p).astype(F32)
    a, f = OB.prepared(n, members, storage, fields, case)
    b, _ = OB.prepared(n, members, storage, fields, case)
    with a, b:
        a.set_observation_points(cols, rows)
        got = a.observation_departures(f, obs=y, threshold=3.0)
        a.set_observation_qc(3.0)
        a.observation_gram(f, obs=y)
        flags = a.observation_qc_result()[0]
        shown = a.download_members(f)
        if case == "zeros":
            assert not shown.view(np.uint32).any() and not got["mean"].view(np.uint32).any() and not got["spread"].view(np.uint32).any()
        else:
            assert np.abs(shown[:, 1:-1, 1:-1]).max() > 0
        want = QC.screen(OB.define_obs(shown, cols, rows), y, None, 3.0)
        same_screen(got, want, "storage=%d %s" % (storage, case))
        assert np.array_equal(flags, want["flag"])
        for name in capi.FIELD_NAMES:          # every field of every member, against the twin that never observed
            assert np.array_equal(a.download_members(name).view(np.uint32), b.download_members(name).view(np.uint32)), name
        ta, tb = a.timing_read(reset=False), b.timing_read(reset=False)
        assert {k: ta[k] for k in OB.COUNTS} == {k: tb[k] for k in OB.COUNTS}
        for s in (a, b):
            s.step(use_sources=True)
        for name in ("u", "v", "dens"):
            assert np.array_equal(a.download_members(name).view(np.uint32), b.download_members(name).view(np.uint32)), name + " a step later"
        ta, tb = a.timing_read(reset=False), b.timing_read(reset=False)
        assert {k: ta[k] for k in ta if not k.endswith("_ms")} == {k: tb[k] for k in tb if not k.endswith("_ms")}


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    import torch
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(59000)
    n, members, p = 6, 5, 65
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in OB.MAIN}
    cols, rows = OB.network(n, p, rng)
    fp, bp, dp = capi._MF, C.POINTER(C.c_ubyte), C.POINTER(C.c_double)
    outs = [np.full(p, 7.0, F32) for _ in range(3)]
    bytes_ = [np.full(p, 7, np.uint8) for _ in range(2)]
    sums = np.full(3, 7.0)
    record = torch.full((members * p,), 1.0, dtype=torch.float32, device="cuda")
    ones = np.ones(p, F32)
    sig = ones.copy()
    sig[17] = np.inf
    f = lambda v: v.ctypes.data_as(fp)
    tail = lambda: [f(outs[0]), f(outs[1]), f(outs[2]), bytes_[0].ctypes.data_as(bp), bytes_[1].ctypes.data_as(bp), sums.ctypes.data_as(dp)]

    def refused(rc, *words):
        assert rc == capi.E_INVALID
        msg = L.fluid_last_error()
        assert all(word in msg for word in words), msg

    with OB.solver(n, members) as s, OB.solver(n, members) as twin:
        for c in (s, twin):
            c.timing_enable(True)
            c.upload_members(**fields)
            c.step(use_sources=True)
            c.add_source("dens", "dens_prev", OB.DT)                      # a lazy state that must survive the refusals
        direct = lambda field=2, obs=ones, sigma=None, t=3.0: L.fluid_observation_departures(
            s._h, field, None if obs is None else f(obs), None if sigma is None else f(sigma), t, *tail())
        recorded = lambda ptr=record.data_ptr(), stride=0, obs=ones, sigma=None, t=3.0: L.fluid_observation_departures_recorded(
            s._h, ptr, stride, None if obs is None else f(obs), None if sigma is None else f(sigma), t, *tail())
        refused(direct(), b"fluid_observation_departures:", b"no observation network")
        refused(recorded(), b"fluid_observation_departures_recorded:", b"no observation network")
        refused(L.fluid_observation_qc_result(s._h, None, None, None), b"fluid_observation_qc_result", b"no gated call")
        s.set_observation_points(cols, rows)
        s.set_observation_qc(4.0)
        s.observation_gram("u", obs=ones)                                 # a gated call: a result to keep
        kept = s.observation_qc_result()
        for field in (12, -1):
            refused(direct(field=field), b"fluid_observation_departures:", b"bad field id %d" % field)
        refused(direct(field=capi.FIELD_OF_POINT), b"fluid_observation_departures:", b"typed network")
        refused(direct(sigma=sig), b"fluid_observation_departures:", b"inv_sigma[17]")
        refused(recorded(sigma=sig), b"fluid_observation_departures_recorded:", b"inv_sigma[17]")
        for bad in (np.nan, np.inf, -1.0):
            refused(direct(t=bad), b"fluid_observation_departures:", b"threshold")
            refused(recorded(t=bad), b"fluid_observation_departures_recorded:", b"threshold")
            refused(L.fluid_set_observation_qc(s._h, bad), b"fluid_set_observation_qc", b"threshold")
        refused(direct(obs=None, t=0.0), b"fluid_observation_departures:", b"departure", b"obs")
        refused(L.fluid_observation_departures(s._h, 2, None, None, 3.0, f(outs[0]), None, None, None, None, None),
                b"fluid_observation_departures:", b"threshold", b"obs")
        refused(recorded(stride=p - 1), b"fluid_observation_departures_recorded:", b"member_stride 64", b"65")
        refused(recorded(ptr=outs[0].ctypes.data), b"fluid_observation_departures_recorded:", b"not device memory")
        refused(recorded(ptr=None), b"fluid_observation_departures_recorded:", b"record_dev")
        refused(L.fluid_observation_qc(s._h, None), b"fluid_observation_qc", b"threshold")
        # a refused gated call leaves the flags alone
        refused(L.fluid_observation_gram(s._h, 2, 1, f(ones), f(sig), np.empty((members, members)).ctypes.data_as(dp), None, None), b"inv_sigma[17]")
        assert all((v == 7.0).all() for v in outs) and all((v == 7).all() for v in bytes_) and (sums == 7.0).all()
        assert (record.cpu().numpy() == 1.0).all()
        assert s.observation_qc() == 4.0
        again = s.observation_qc_result()
        assert np.array_equal(again[0], kept[0]) and again[1:] == kept[1:]
        s.set_observation_qc(0.0)
        twin.set_observation_points(cols, rows)
        twin.observation_gram("u", obs=ones)                              # (what the one accepted call of `s` settled)
        ta, tb = s.timing_read(reset=False), twin.timing_read(reset=False)
        assert ta == {**tb, **{k: ta[k] for k in ta if k.endswith("_ms")}}             # every count; the times are times
        for name in capi.FIELD_NAMES:
            assert np.array_equal(s.download_members(name).view(np.uint32), twin.download_members(name).view(np.uint32)), name
        for c in (s, twin):
            c.step(use_sources=True)
        for name in ("u", "v", "dens"):
            assert np.array_equal(s.download_members(name).view(np.uint32), twin.download_members(name).view(np.uint32)), name
        assert direct() == capi.OK and recorded() == capi.OK             # ... and the same arguments, accepted
        assert not (outs[0] == 7.0).any() and (sums != 7.0).all()
    # the member counts: one member, one too many (the message gives both numbers)
    for count, words in ((1, (b"1 members", b"[2,", b"64")), (capi.TRANSFORM_MAX_MEMBERS + 1, (b"65 members", b"[2,", b"64"))):
        with OB.solver(2, count) as s:
            s.set_observation_points([1.5], [2.25])
            one = np.ones(1, F32)
            refused(L.fluid_observation_departures(s._h, 0, f(one), None, 0.0, f(outs[0]), None, None, None, None, None),
                    b"fluid_observation_departures:", *words)
            if count == 1:
                refused(L.fluid_set_observation_qc(s._h, 3.0), b"fluid_set_observation_qc", b"below 2")
                assert s.observation_qc() == 0.0
    with OB.F().FluidSolver(n, rank=0, nranks=2) as s:
        one = np.ones(1, F32)
        refused(L.fluid_set_observation_qc(s._h, 3.0), b"fluid_set_observation_qc", b"slab")
        refused(L.fluid_observation_departures(s._h, 0, f(one), None, 0.0, None, None, None, None, None, None), b"fluid_observation_departures:", b"slab")
