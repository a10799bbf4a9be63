"""GPU: typed observation networks -- fluid_set_observation_network, fluid_observation_network_fields and FLUID_FIELD_OF_POINT in
the five observing calls (include/fluid_amd.h, "typed networks").

Nothing is defined here but one line: row p of the typed observations is `define_obs(x[field[p]], ...)[:, p]`, the definition of
tests/test_gpu_observe.py applied to the field the point names.  Everything after it -- `operands`, `exact_sums`, `within_bound`,
`weights`, `node_reference`, `composed`, `same_members` -- is imported from the tests of the untyped calls, with their comparisons
and tolerances unchanged: bit for bit for the observations and the analysis, `==` on dyadic data and the summation bound on general
data for the Grams.

Shapes: N = 6 and 30; M = 5, 8, 17 (the Gram kernels pad them to 8, 8 and 32: a class with padding members, a full one, the next
one); P = 65 and 130: a full chunk of 64 points and a short one, and more than one chunk per block.  At N = 6 a member is
64 cells, so the staging buffer of the host route holds 64 M floats and P = 65 or 130 points force it into several groups of
members: the typed launch then starts at a first member other than 0."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_etkf as EK
import test_gpu_lattice_gram as LG
import test_gpu_observe as OB

pytestmark = pytest.mark.gpu
F32 = np.float32
STORAGES = pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
MEMBERS = [5, 8, 17]
POINTS = [65, 130]
THREE = ("u", "v", "dens")
FIVE = ("u", "v_prev", "dens", "u_prev", "v")           # fp16 after a step: u_prev and v_prev are held at a scale, the others are not


def fields_of(p, names, lone=None):
    """one field name per point, cycling through `names`; lone = (at, name): the first chunk of 64 points all observe names[0]
    but the single point `at`, which observes `name`"""
    out = [names[k % len(names)] for k in range(p)]
    if lone is not None:
        out[:64] = [names[0]] * 64
        out[lone[0]] = lone[1]
    return out


def typed_obs(shown, names, cols, rows):
    """the model: h[m][p] from the field point p names.  shown: {name: (M, W, W) float32, what the pack shows}"""
    per_field = {f: OB.define_obs(shown[f], cols, rows) for f in set(names)}
    return np.stack([per_field[f][:, p] for p, f in enumerate(names)], axis=1)


def shown_of(s, names):
    return {f: s.download_members(f) for f in set(names)}


def power_of_two(m):
    return m & (m - 1) == 0


# ---- 1. / 2. observed values bit for bit; the device and the host route -----------------------------------------------------------
@STORAGES
@pytest.mark.parametrize("n", [6, 30])
def test_observed_values_bit_for_bit(n, storage):
    w = n + 2
    rng = np.random.default_rng(31000 + 10 * n + storage)
    for members in MEMBERS:
        with OB.solver(n, members, storage) as s:
            s.upload_members(dens=rng.uniform(-4.0, 4.0, (members, w, w)).astype(F32), u=rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32),
                             v=rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32))
            s.vel_step()                               # fp16 storage, N >= 16: u_prev and v_prev, the pressure and the divergence, are held scaled
            for p in POINTS:
                cols, rows = OB.network(n, p, rng)
                for names in (fields_of(p, THREE), fields_of(p, FIVE), fields_of(p, FIVE, lone=(37, "u_prev"))):
                    what = "n=%d M=%d storage=%d P=%d fields %s.." % (n, members, storage, p, names[36:39])
                    before = shown_of(s, names)
                    s.set_observation_network(cols, rows, names)
                    assert s.observation_points() == p and s.observation_fields() == set(names)
                    want = typed_obs(before, names, cols, rows)
                    dev = s.observe_device()
                    assert tuple(dev.shape) == (members, p)
                    OB.same_bits(dev.cpu().numpy(), want, what + ": the device route")
                    if n == 6:
                        assert (64 * members) // p < members, "the host route goes in several groups of members"
                    OB.same_bits(s.observe(), want, what + ": the host route")
                    OB.same_bits(s.observe("point"), want, what + ": field='point'")
                    for f in set(names):
                        assert np.array_equal(s.download_members(f).view(np.uint32), before[f].view(np.uint32)), "the call changed " + f


# ---- 3. the Gram matrix on dyadic data: exact, and the exact sum of the per-field results -------------------------------------------
@STORAGES
@pytest.mark.parametrize("members", MEMBERS)
def test_gram_exact_on_dyadic_data(members, storage):
    rng = np.random.default_rng(32000 + 100 * storage + members)
    for n, p in ((6, 65), (30, 130)):
        w = n + 2
        x = {f: rng.choice(OB.COARSE, size=(members, w, w)).astype(F32) for f in THREE}
        cols, rows = OB.network(n, p, rng, quarter=True)
        y = (rng.integers(-8, 9, p) / 4.0).astype(F32)
        sg = rng.choice(np.array([0.5, 1.0, 2.0], F32), p)
        names = fields_of(p, THREE, lone=(11, "dens"))
        of = np.array(names)
        with OB.solver(n, members, storage) as s:
            s.upload_members(**x)
            s.set_observation_network(cols, rows, names)
            h = typed_obs(x, names, cols, rows)            # multiples of 2^-6, exact in float32
            assert np.array_equal(s.observe(), h)
            got = {}
            for centre in (False, True):
                if centre and not power_of_two(members):   # a power of two: the mean, the anomalies and the products are exact
                    continue
                for obs, sigma in ((None, None), (y, None), (None, sg), (y, sg)):
                    what = "M=%d storage=%d N=%d P=%d centre=%s obs=%s sigma=%s" % (members, storage, n, p, centre, obs is not None, sigma is not None)
                    g = s.observation_gram(obs=obs, inv_sigma=sigma, centre=centre)
                    am, d = OB.operands(h, obs, sigma, centre)
                    gram, rhs, dd = OB.exact_sums(am, d, 14)
                    OB.equal(g[0] if obs is not None else g, gram, what)
                    OB.symmetric(g[0] if obs is not None else g, what)
                    if obs is not None:
                        OB.equal(g[1], rhs, what + ": rhs")
                        OB.equal(g[2], dd, what + ": dd")
                    OB.same_bits(OB.pack_results(members, s.observation_gram(None, obs=obs, inv_sigma=sigma, centre=centre)),
                                 OB.pack_results(members, g), what + ": two calls in a row")
                    got[(centre, obs is not None, sigma is not None)] = OB.pack_results(members, g)
            # the route a caller had before: one untyped sub-network per field, the matrices added on the host -- exact on this data
            total = {k: 0.0 for k in got}
            for f in THREE:
                idx = np.nonzero(of == f)[0]
                s.set_observation_points(cols[idx], rows[idx])
                assert s.observation_fields() == set()
                for centre, with_obs, with_sigma in got:
                    part = s.observation_gram(f, obs=y[idx] if with_obs else None, inv_sigma=sg[idx] if with_sigma else None, centre=centre)
                    total[(centre, with_obs, with_sigma)] = total[(centre, with_obs, with_sigma)] + OB.pack_results(members, part)
            for k in got:
                OB.equal(got[k], total[k], "M=%d storage=%d N=%d P=%d %s: the sum of the per-field results" % (members, storage, n, p, k))


# ---- 4. the Gram matrix on general data: the summation bound -------------------------------------------------------------------------
@STORAGES
@pytest.mark.parametrize("n,members,p", [(6, 5, 65), (30, 17, 130), (30, 8, 65)])
def test_gram_general_data_within_the_summation_bound(n, members, p, storage):
    rng = np.random.default_rng(33000 + 100 * storage + members)
    w = n + 2
    x = {f: (rng.uniform(0.25, 1.0, (members, w, w)) * rng.choice([-1.0, 1.0], (members, w, w)) + 50).astype(F32) for f in THREE}
    cols, rows = OB.network(n, p, rng)
    names = fields_of(p, THREE)
    y = (rng.normal(size=p) + 50).astype(F32)
    sg = rng.uniform(0.5, 20.0, p).astype(F32)
    with OB.solver(n, members, storage) as s:
        s.upload_members(**x)
        s.set_observation_network(cols, rows, names)
        h = typed_obs(shown_of(s, names), names, cols, rows)
        OB.same_bits(s.observe(), h, "the observations")
        for centre in (False, True):
            for obs, sigma in ((None, None), (y, None), (None, sg), (y, sg)):
                what = "n=%d M=%d P=%d storage=%d centre=%s obs=%s sigma=%s" % (n, members, p, storage, centre, obs is not None, sigma is not None)
                got = s.observation_gram(obs=obs, inv_sigma=sigma, centre=centre)
                OB.within_bound(got, *OB.operands(h, obs, sigma, centre), what)
                OB.symmetric(got[0] if obs is not None else got, what)


# ---- 5. / 6. every point names one field: the untyped call's bits; a concrete field on a typed network: the same ---------------------
@STORAGES
@pytest.mark.parametrize("members,p", [(5, 65), (8, 130), (17, 65)])
def test_one_field_typed_and_concrete_fields_are_the_untyped_call(members, p, storage):
    n = 30
    lat, c, rho, listed = ((3, 3), (-8, 0), 16), 6.0, 1.1, ("dens", "u", "v")
    rng = np.random.default_rng(35000 + 100 * members + storage)
    fields = EK.start_fields(n, members, rng)
    cols, rows = EK.network(rng, p)
    y = rng.uniform(0.2, 1.5, p).astype(F32)
    sg = rng.uniform(2.0, 8.0, p).astype(F32)
    with EK.solver(n, members, storage) as one, EK.solver(n, members, storage) as plain, EK.solver(n, members, storage) as mixed:
        for s in (one, plain, mixed):
            s.upload_members(**fields)
            s.step(2, use_sources=True)                    # fp16: the pressure scale is live
        plain.set_observation_points(cols, rows)
        mixed.set_observation_network(cols, rows, fields_of(p, FIVE))
        for f in ("u_prev", "dens"):                       # a field held at a scale with fp16 storage, and one that is not
            what = "M=%d P=%d storage=%d %s" % (members, p, storage, f)
            one.set_observation_network(cols, rows, [f] * p)
            assert one.observation_fields() == {f}
            want = plain.observe(f)
            assert np.abs(want).max() > 0
            OB.same_bits(one.observe(), want, what + ": observe, typed with one field")
            OB.same_bits(one.observe_device().cpu().numpy(), want, what + ": observe_device, typed with one field")
            OB.same_bits(mixed.observe(f), want, what + ": observe, a concrete field on a typed network")
            OB.same_bits(mixed.observe_device(f).cpu().numpy(), want, what + ": observe_device, a concrete field on a typed network")
            for centre in (False, True):
                g = OB.pack_results(members, plain.observation_gram(f, obs=y, inv_sigma=sg, centre=centre))
                OB.same_bits(OB.pack_results(members, one.observation_gram(obs=y, inv_sigma=sg, centre=centre)), g, what + ": Gram, one field")
                OB.same_bits(OB.pack_results(members, mixed.observation_gram(f, obs=y, inv_sigma=sg, centre=centre)), g, what + ": Gram, concrete")
                lg = LG.call(plain, f, lat, c, y, sg, centre)
                for s, who in ((one, None), (mixed, f)):
                    got = LG.call(s, who, lat, c, y, sg, centre)
                    LG.same_bits(LG.flat(got), LG.flat(lg), what + ": lattice Gram, " + ("one field" if who is None else "concrete"))
                    assert np.array_equal(got[3], lg[3])
        # the fused analysis, in every listed field of every member (dens is the field the points name)
        plain.analyse_lattice("dens", lat[0], lat[1], lat[2], c, y, inv_sigma=sg, rho=rho, fields=listed)
        one.analyse_lattice(None, lat[0], lat[1], lat[2], c, y, inv_sigma=sg, rho=rho, fields=listed)
        mixed.analyse_lattice("dens", lat[0], lat[1], lat[2], c, y, inv_sigma=sg, rho=rho, fields=listed)
        status = plain.analyse_status()
        assert status["solved"] >= 2 and status["failed"] == 0 and one.analyse_status() == status == mixed.analyse_status()
        EK.same_members(one, plain, EK.MAIN, "analyse_lattice, typed with one field")
        EK.same_members(mixed, plain, EK.MAIN, "analyse_lattice, a concrete field on a typed network")
        changed = [f for f in listed if not np.array_equal(one.download_members(f).view(np.uint32), fields[f].view(np.uint32))]
        assert changed == list(listed)


# ---- 7. the lattice Gram with every point's own field ---------------------------------------------------------------------------------
@STORAGES
@pytest.mark.parametrize("members", MEMBERS)
def test_lattice_gram_exact_on_dyadic_data(members, storage):
    rng = np.random.default_rng(37000 + 100 * storage + members)
    for n, p, lat in ((6, 65, ((1, 3), (3, -5), 8)), (30, 130, ((3, 2), (7, 9), 8))):
        w = n + 2
        x = {f: rng.choice(LG.COARSE, size=(members, w, w)).astype(F32) for f in THREE}
        y = (rng.integers(-8, 9, p) / 4.0).astype(F32)
        sg = rng.choice(np.array([0.5, 1.0, 2.0], F32), p)
        names = fields_of(p, THREE, lone=(50, "v"))
        with LG.solver(n, members, storage) as s:
            s.upload_members(**x)
            for round_ in range(2):                        # the second network: the same count, lattice and c -- the lists must not survive
                cols, rows = LG.dyadic_network(n, p, lat, rng)
                wt, r, _ = LG.weights(cols, rows, *lat, 1.0)
                assert (((r == 0) & (wt == 1)) | ((r >= 2.5) & (wt == 0))).all()
                s.set_observation_network(cols, rows, names)
                h = typed_obs(x, names, cols, rows)
                assert np.array_equal(s.observe(), h)
                s.set_observation_points(cols, rows)
                plain_counts = LG.call(s, "u", lat, 1.0)[3]
                s.set_observation_network(cols, rows, names)
                for centre in (False, True):
                    if centre and not power_of_two(members):
                        continue
                    for obs, sigma in ((None, None), (y, sg)):
                        what = "M=%d storage=%d N=%d P=%d network %d centre=%s obs=%s" % (members, storage, n, p, round_, centre, obs is not None)
                        got = LG.call(s, None, lat, 1.0, obs, sigma, centre)
                        LG.check_shapes(got, lat, members)
                        gram, rhs, dd, counts = got
                        assert np.array_equal(counts, plain_counts), what + ": the counts do not depend on the fields"
                        am, d = LG.operands(h, obs, sigma, centre)
                        seen = 0
                        for ia in range(lat[0][0]):
                            for ib in range(lat[0][1]):
                                idx = np.nonzero(wt[ia, ib])[0]
                                assert counts[ia, ib] == len(idx), what
                                want, _, _ = LG.node_reference(am, d, wt[ia, ib], idx)       # weights 0 and 1, dyadic operands: exact
                                LG.equal(LG.pack_node(members, gram[ia, ib], None if obs is None else rhs[ia, ib], None if obs is None else dd[ia, ib]),
                                         want, "%s node (%d, %d)" % (what, ia, ib))
                                LG.symmetric(gram[ia, ib], what)
                                if len(idx) == 0:
                                    LG.plus_zero(got, ia, ib, what)
                                seen += len(idx) > 0
                        assert seen > 0
                        LG.same_bits(LG.flat(LG.call(s, None, lat, 1.0, obs, sigma, centre)), LG.flat(got), what + ": the kept lists")
            for f in THREE:
                assert np.array_equal(s.download_members(f).view(np.uint32), x[f].view(np.uint32)), "the call changed " + f


# ---- 8. the fused analysis is the three calls ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("members,storage,p", [(8, 0, 65), (17, 0, 130), (5, 1, 130), (17, 1, 65)])
def test_the_fused_call_is_the_three_calls(members, storage, p):
    n = 30
    shape, origin, step, c, rho, listed = (3, 3), (-8, 0), 16, 6.0, 1.1, ("dens", "u", "v")
    rng = np.random.default_rng(38000 + 100 * members + storage)
    fields = EK.start_fields(n, members, rng)
    cols, rows = EK.network(rng, p)
    names = fields_of(p, THREE, lone=(9, "dens"))
    inv_sigma = rng.uniform(2.0, 8.0, p).astype(F32)
    y = rng.uniform(0.2, 1.5, p).astype(F32)
    what = "M=%d storage=%d P=%d" % (members, storage, p)
    with EK.solver(n, members, storage) as a, EK.solver(n, members, storage) as b:
        for s in (a, b):
            s.upload_members(**fields)
            s.step(2, use_sources=True)                    # fp16: the pressure scale is live; the sources are marked zero
            s.set_observation_network(cols, rows, names)
        a.analyse_lattice(None, shape, origin, step, c, y, inv_sigma=inv_sigma, rho=rho, fields=listed, wait=False)
        d, status, counts = EK.composed(b, None, shape, origin, step, c, y, inv_sigma, rho, listed)
        want = {"solved": int((status == 0).sum()), "empty": int((status == 1).sum()), "failed": int((status == 2).sum())}
        assert a.analyse_status() == want, what
        assert want["empty"] >= 3 and want["solved"] >= 2 and (counts[0] == 0).all(), counts
        assert want["failed"] == 0 and np.abs(d).max() > 1e-4
        EK.same_members(a, b, EK.MAIN, what)
        changed = [f for f in listed if not np.array_equal(a.download_members(f).view(np.uint32), fields[f].view(np.uint32))]
        assert changed == list(listed)
        for s in (a, b):
            s.step(1)
        EK.same_members(a, b, THREE, what + ": a step after the analysis")


# ---- 9. poisoning ---------------------------------------------------------------------------------------------------------------------
@STORAGES
def test_poisoning(storage):
    """a NaN in member 2 of u, in a cell that the stencils of a u point and of a dens point hold: inside the supports of nodes 0
    and 1 and outside node 2's"""
    n, members, p, bad, at = 30, 5, 130, 2, 100
    lat, c = ((1, 3), (15, -1), 16), 8.0                  # nodes on row 15, columns -1, 15, 31; supports of radius 16
    rng = np.random.default_rng(39000 + storage)
    w = n + 2
    x = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in THREE}
    cols, rows = OB.network(n, p, rng)
    names = fields_of(p, ("u", "dens"))
    cols[at], rows[at] = 8.25, 15.5                       # names[100] is u ...
    cols[at + 1], rows[at + 1] = 8.25, 15.5               # ... and the same position observes dens
    assert names[at] == "u" and names[at + 1] == "dens"
    y = rng.normal(size=p).astype(F32)
    sg = rng.uniform(0.5, 2.0, p).astype(F32)
    wt, r, _ = LG.weights(cols, rows, *lat, c)
    j0, i0 = cols.astype(np.int64), rows.astype(np.int64)
    touched = ((i0 == 15) | (i0 == 14)) & ((j0 == 8) | (j0 == 7))          # the points whose stencil holds cell (15, 8)
    hit = touched & (np.array(names) == "u")
    assert hit[at] and touched[at + 1] and not hit[at + 1] and (r[0, 2][touched] > 2.5).all()
    assert wt[0, 0, at] != 0 and wt[0, 1, at] != 0
    keep = np.ones((members, members), bool)
    keep[bad] = keep[:, bad] = False
    with OB.solver(n, members, storage) as s:
        s.upload_members(**x)
        s.set_observation_network(cols, rows, names)
        clean_h = s.observe()
        clean_g = {centre: s.observation_gram(obs=y, inv_sigma=sg, centre=centre) for centre in (False, True)}
        clean = {centre: LG.call(s, None, lat, c, y, sg, centre) for centre in (False, True)}
        assert np.isfinite(clean_h).all() and all(np.isfinite(v).all() for k in clean for v in clean[k][:3])
        x["u"][bad, 15, 8] = np.nan
        s.upload_members(u=x["u"])
        h = s.observe()
        OB.same_bits(h, typed_obs(shown_of(s, names), names, cols, rows), "with a NaN in u")
        assert np.isnan(h[bad][hit]).all()
        only = np.zeros_like(h, bool)
        only[bad, hit] = True
        assert np.array_equal(h.view(np.uint32)[~only], clean_h.view(np.uint32)[~only]), "the NaN reached a point that does not observe u"
        dens_points = np.array(names) == "dens"
        OB.same_bits(np.ascontiguousarray(h[:, dens_points]), np.ascontiguousarray(clean_h[:, dens_points]), "the pure-dens entries")
        # the Gram call
        g, rhs, dd = s.observation_gram(obs=y, inv_sigma=sg, centre=False)
        assert np.isnan(g[bad]).all() and np.isnan(g[:, bad]).all() and np.isnan(rhs[bad])
        assert np.array_equal(g.view(np.uint64)[keep], clean_g[False][0].view(np.uint64)[keep]), "a NaN in member 2 changed another entry"
        assert np.array_equal(np.delete(rhs, bad).view(np.uint64), np.delete(clean_g[False][1], bad).view(np.uint64))
        assert dd == clean_g[False][2]
        g, rhs, dd = s.observation_gram(obs=y, inv_sigma=sg, centre=True)
        assert np.isnan(g).all() and np.isnan(rhs).all() and np.isnan(dd)
        # the lattice call, per node
        gram, rhs, dd, counts = LG.call(s, None, lat, c, y, sg, False)
        for node in (0, 1):
            g = gram[0, node]
            assert np.isnan(g[bad]).all() and np.isnan(g[:, bad]).all() and np.isnan(rhs[0, node, bad])
            assert np.array_equal(g.view(np.uint64)[keep], clean[False][0][0, node].view(np.uint64)[keep]), "a NaN in member 2 changed another entry"
            assert np.array_equal(np.delete(rhs[0, node], bad).view(np.uint64), np.delete(clean[False][1][0, node], bad).view(np.uint64))
            LG.same_bits(dd[0, node], clean[False][2][0, node], "dd")
        for v, ref in zip((gram, rhs, dd), clean[False][:3]):
            LG.same_bits(v[0, 2], ref[0, 2], "centre=False: the node that does not see the point")
        gram, rhs, dd, counts = LG.call(s, None, lat, c, y, sg, True)
        assert np.isnan(gram[0, :2]).all() and np.isnan(rhs[0, :2]).all() and np.isnan(dd[0, :2]).all()
        for v, ref in zip((gram, rhs, dd), clean[True][:3]):
            LG.same_bits(v[0, 2], ref[0, 2], "centre=True: the node that does not see the point")
        assert np.array_equal(counts, clean[True][3])
        # a network whose u points all stay away from the cell: the dens point on it sees nothing of the NaN
        far = [("dens" if t else f) for t, f in zip(touched, names)]
        s.set_observation_network(cols, rows, far)
        assert np.isfinite(s.observe()).all() and np.isfinite(OB.pack_results(members, s.observation_gram(obs=y, inv_sigma=sg, centre=True))).all()


# ---- 10. lazy state ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,case", [(0, "pending"), (1, "pending"), (1, "scaled")])
def test_lazy_state_is_settled_and_nothing_is_altered(storage, case):
    """`pending` (tests/test_gpu_observe.py: prepared): dens owes itself a deferred add_source and dens_prev is zero by definition;
    `scaled`: fp16, u_prev is held at a scale.  The network observes both, and u."""
    from fluidsimulationcuda_amd import capi
    members, n, p = 5, 30, 130
    rng = np.random.default_rng(40000 * storage + len(case))
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in OB.MAIN}
    cols, rows = OB.network(n, p, rng)
    names = fields_of(p, ("dens", "dens_prev", "u") if case == "pending" else ("u_prev", "dens", "u"))
    a, _ = OB.prepared(n, members, storage, fields, case)
    b, _ = OB.prepared(n, members, storage, fields, case)
    lazy, _ = OB.prepared(n, members, storage, fields, case)
    with a, b, lazy:
        a.set_observation_network(cols, rows, names)
        got = a.observe_device().cpu().numpy()
        gram, rhs, dd = a.observation_gram(obs=np.zeros(p, F32), centre=False)
        shown = shown_of(a, names)
        if case == "pending":
            assert not shown["dens_prev"].view(np.uint32).any()
        want = typed_obs(shown, names, cols, rows)
        OB.same_bits(got, want, "storage=%d %s" % (storage, case))
        OB.same_bits(a.observe(), want, "storage=%d %s: the host call" % (storage, case))
        OB.within_bound((gram, rhs, dd), *OB.operands(want, np.zeros(p, F32), None, False), "storage=%d %s" % (storage, case))
        if case == "pending":
            # a field no point observes is not settled: settling dens is one launch of the source category
            lazy.set_observation_network(cols, rows, fields_of(p, ("u", "v")))
            lazy.observe_device()
            lazy.observation_gram(centre=True)
            tl, tb = lazy.timing_read(reset=False), b.timing_read(reset=False)
            assert {k: tl[k] for k in tl if not k.endswith("_ms")} == {k: tb[k] for k in tb if not k.endswith("_ms")}
            lazy.set_observation_network(cols, rows, names)
            lazy.observe_device()
            tl = lazy.timing_read(reset=False)
            assert tl["source_calls"] > tb["source_calls"], "the deferred add_source of dens was settled by a launch of its own"
        for name in capi.FIELD_NAMES:              # every field of every member, against the twin that never observed
            assert np.array_equal(a.download_members(name).view(np.uint32), b.download_members(name).view(np.uint32)), name
        ta, tb = a.timing_read(reset=False), b.timing_read(reset=False)
        assert {k: ta[k] for k in OB.COUNTS} == {k: tb[k] for k in OB.COUNTS}
        for s in (a, b):
            s.step(use_sources=True)
        for name in capi.FIELD_NAMES:
            assert np.array_equal(a.download_members(name).view(np.uint32), b.download_members(name).view(np.uint32)), name + " a step later"
        ta, tb = a.timing_read(reset=False), b.timing_read(reset=False)
        assert {k: ta[k] for k in ta if not k.endswith("_ms")} == {k: tb[k] for k in tb if not k.endswith("_ms")}


# ---- 11. refusals change nothing ------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    import torch
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(41)
    n, members, p = 6, 5, 65
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in OB.MAIN}
    cols, rows = OB.network(n, p, rng)
    ids = np.array([k % 3 for k in range(p)], np.int32)
    dp, fp, ip = C.POINTER(C.c_double), capi._MF, C.POINTER(C.c_int)
    gram, rhs, dd = np.full((members, members), 7.0), np.full(members, 7.0), np.full(1, 7.0)
    lgram, lrhs, ldd, lcounts = np.full((2, 2, members, members), 7.0), np.full((2, 2, members), 7.0), np.full((2, 2), 7.0), np.full((2, 2), 7, np.int32)
    host = np.full((members, p), 7.0, F32)
    dev = torch.full((members * p,), 7.0, dtype=torch.float32, device="cuda")
    ones = np.ones(p, F32)
    listed = (C.c_int * 3)(0, 1, 2)
    g = lambda a: a.ctypes.data_as(dp)
    f = lambda a: a.ctypes.data_as(fp)
    i = lambda a: a.ctypes.data_as(ip)
    FOP = capi.FIELD_OF_POINT
    assert FOP == -2

    def refused(rc, *words):
        assert rc == capi.E_INVALID
        msg = L.fluid_last_error()
        assert all(word in msg for word in words), msg

    def the_five(s, field, *words):
        refused(L.fluid_observe_members(s._h, field, dev.data_ptr(), 0), b"fluid_observe_members", *words)
        refused(L.fluid_observe_members_host(s._h, field, f(host)), b"fluid_observe_members_host", *words)
        refused(L.fluid_observation_gram(s._h, field, 1, f(ones), None, g(gram), g(rhs), g(dd)), b"fluid_observation_gram", *words)
        refused(L.fluid_observation_gram_lattice(s._h, field, 1, f(ones), None, 2, 2, 0, 0, 8, 4.0, g(lgram), g(lrhs), g(ldd), i(lcounts)),
                b"fluid_observation_gram_lattice", *words)
        refused(L.fluid_analyse_lattice(s._h, field, f(ones), None, 2, 2, 0, 0, 8, 4.0, 1.0, listed, 3), b"fluid_analyse_lattice", *words)

    with OB.solver(n, members) as s, OB.solver(n, members) as twin:
        for c in (s, twin):
            c.timing_enable(True)
            c.upload_members(**fields)
            c.step(use_sources=True)
            c.add_source("dens", "dens_prev", OB.DT)                   # a lazy state that must survive the refusals
        mask = C.c_uint(77)
        # no network: the message of each call as before
        the_five(s, FOP, b"no observation network")
        assert L.fluid_observation_network_fields(s._h, C.byref(mask)) == capi.OK and mask.value == 0
        # the network itself, under the new call's name
        refused(L.fluid_set_observation_network(s._h, f(cols), f(rows), i(ids), -1), b"fluid_set_observation_network", b"npoints -1")
        big = np.ones(capi.OBSERVE_MAX_POINTS + 1, F32)
        refused(L.fluid_set_observation_network(s._h, f(big), f(big), None, big.size), b"fluid_set_observation_network", b"1048577")
        refused(L.fluid_set_observation_network(s._h, None, f(rows), i(ids), p), b"fluid_set_observation_network", b"col")
        refused(L.fluid_set_observation_network(s._h, f(cols), None, i(ids), p), b"fluid_set_observation_network", b"row")
        for bad_at, value in ((17, 12), (0, -1), (64, FOP), (3, 1 << 20)):
            wrong = ids.copy()
            wrong[bad_at] = value
            refused(L.fluid_set_observation_network(s._h, f(cols), f(rows), i(wrong), p), b"fluid_set_observation_network",
                    b"point %d" % bad_at, b"field = %d" % value)
        outside = cols.copy()
        outside[2] = n + 0.51
        refused(L.fluid_set_observation_network(s._h, f(outside), f(rows), i(ids), p), b"fluid_set_observation_network: point 2: col")
        refused(L.fluid_observation_network_fields(s._h, None), b"fluid_observation_network_fields", b"mask")
        count = C.c_int(-1)
        assert L.fluid_observation_points(s._h, C.byref(count)) == capi.OK and count.value == 0
        # an untyped network, set either way: the sentinel needs a typed one
        s.set_observation_points(cols, rows)
        the_five(s, FOP, b"typed network")
        assert L.fluid_set_observation_network(s._h, f(cols), f(rows), None, p) == capi.OK
        the_five(s, FOP, b"typed network")
        assert L.fluid_observation_network_fields(s._h, C.byref(mask)) == capi.OK and mask.value == 0
        for field in (12, -1, -3):
            the_five(s, field, b"bad field id %d" % field)
        # a typed network: a refused replacement leaves it in place; other ids are bad field ids as ever
        assert L.fluid_set_observation_network(s._h, f(cols), f(rows), i(ids), p) == capi.OK            # (host work and copies: no launch)
        wrong = ids.copy()
        wrong[5] = 12
        refused(L.fluid_set_observation_network(s._h, f(cols), f(rows), i(wrong), p), b"point 5", b"field = 12")
        refused(L.fluid_set_observation_network(s._h, f(outside), f(rows), i(ids), p), b"point 2: col")
        assert L.fluid_observation_network_fields(s._h, C.byref(mask)) == capi.OK and mask.value == 0b111
        for field in (12, -1, -3):
            the_five(s, field, b"bad field id %d" % field)
        sig = ones.copy()
        sig[17] = np.inf
        refused(L.fluid_observation_gram(s._h, FOP, 1, f(ones), f(sig), g(gram), g(rhs), g(dd)), b"fluid_observation_gram", b"inv_sigma[17]")
        refused(L.fluid_observe_members(s._h, FOP, dev.data_ptr(), p - 1), b"fluid_observe_members", b"member_stride 64", b"65")
        refused(L.fluid_analyse_lattice(s._h, FOP, f(ones), None, 2, 2, 0, 0, 8, 4.0, -1.0, listed, 3), b"fluid_analyse_lattice", b"rho")
        assert (gram == 7.0).all() and (rhs == 7.0).all() and (dd == 7.0).all() and (host == 7.0).all()
        assert (lgram == 7.0).all() and (lrhs == 7.0).all() and (ldd == 7.0).all() and (lcounts == 7).all()
        assert (dev.cpu().numpy() == 7.0).all()
        ta, tb = s.timing_read(reset=False), twin.timing_read(reset=False)
        assert ta == {**tb, **{k: ta[k] for k in ta if k.endswith("_ms")}}             # every count; the times are times
        for name in capi.FIELD_NAMES:
            assert np.array_equal(s.download_members(name).view(np.uint32), twin.download_members(name).view(np.uint32)), name
        for c in (s, twin):
            c.step(use_sources=True)
        for name in THREE:
            assert np.array_equal(s.download_members(name).view(np.uint32), twin.download_members(name).view(np.uint32)), name
        shown = {name: s.download_members(name) for name in THREE}
        OB.same_bits(s.observe(), typed_obs(shown, [capi.FIELD_NAMES[k] for k in ids], cols, rows), "the network that survived the refusals")
    # row slabs: both calls
    with OB.F().FluidSolver(n, rank=0, nranks=2) as s:
        one, zero, mask = np.full(1, 1.5, F32), np.zeros(1, np.int32), C.c_uint(77)
        refused(L.fluid_set_observation_network(s._h, f(one), f(one), i(zero), 1), b"fluid_set_observation_network", b"slab")
        refused(L.fluid_set_observation_network(s._h, f(one), f(one), None, 1), b"fluid_set_observation_network", b"slab")
        refused(L.fluid_observation_network_fields(s._h, C.byref(mask)), b"fluid_observation_network_fields", b"slab")
        refused(L.fluid_observe_members_host(s._h, FOP, f(one)), b"fluid_observe_members_host", b"slab")
        assert mask.value == 77 and one[0] == 1.5


# ---- 12. the mask ---------------------------------------------------------------------------------------------------------------------
def test_the_mask_follows_the_network():
    from fluidsimulationcuda_amd import capi
    n, members = 6, 5
    rng = np.random.default_rng(42)
    cols, rows = OB.network(n, 65, rng)
    with OB.solver(n, members) as s:
        assert s.observation_fields() == set()
        s.set_observation_network(cols, rows, fields_of(65, THREE))
        assert s.observation_fields() == set(THREE)
        s.set_observation_network(cols, rows, [capi.FIELD_NAMES.index("tmp0")] * 64 + ["v_prev"])       # ids and names
        assert s.observation_fields() == {"tmp0", "v_prev"}
        mask = C.c_uint()
        assert capi.lib().fluid_observation_network_fields(s._h, C.byref(mask)) == capi.OK
        assert mask.value == (1 << capi.FIELD_NAMES.index("tmp0")) | (1 << capi.FIELD_NAMES.index("v_prev"))
        s.set_observation_points(cols, rows)                   # replaced by an untyped network
        assert s.observation_fields() == set() and s.observation_points() == 65
        s.set_observation_network(cols[:3], rows[:3], ["dens"] * 3)
        assert s.observation_fields() == {"dens"} and s.observation_points() == 3
        s.set_observation_network(cols, rows)                  # fields=None: set_observation_points
        assert s.observation_fields() == set() and s.observation_points() == 65
        s.set_observation_network(cols[:3], rows[:3], ["u"] * 3)
        s.set_observation_network([], [], [])                  # cleared
        assert s.observation_fields() == set() and s.observation_points() == 0
        with pytest.raises(capi.FluidError, match="fluid_observe_members_host.*no observation network"):
            s.observe()
