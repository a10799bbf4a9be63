"""GPU: every member count.  The ensemble kernels are templates on a padded member count -- transform_padded(M) = 1, 2, 4 .. 64
for the transforms and the table the ETKF solve writes, gram_padded(M) = 8, 16, 32, 64 for the Gram kernels and the solve --
and the modules that test them list a handful of counts each.  Here every M in 1 .. 64 is run, at the smallest grids: a
count that fills its padding leaves no zero column to hide behind, one below it has the odd-M bye pair of the solve live in
the last slot, and the counts in between fill the 16-member chunks of the lattice update to every level.

Nothing is defined here.  Every expected value comes from the numpy definitions next to the tests of each call
(tests/test_gpu_transform.py, _local, _lattice, _gram, _observe, _lattice_gram, _etkf), with their comparisons and their
tolerances unchanged: bit for bit for the transforms, `==` on dyadic data and the summation bound on general data for the
Grams, the tolerance of tests/test_gpu_etkf.py for the solve.  A test instance is a padded class, so a failure names its
instantiation; inside it runs every M of the class."""
import numpy as np
import pytest

import test_gpu_etkf as EK
import test_gpu_gram as GR
import test_gpu_lattice as LA
import test_gpu_lattice_gram as LG
import test_gpu_local as LO
import test_gpu_observe as OB
import test_gpu_transform as TR

pytestmark = pytest.mark.gpu
F32 = np.float32
CLASSES = {1: [1], 2: [2], 4: [3, 4], 8: list(range(5, 9)), 16: list(range(9, 17)), 32: list(range(17, 33)), 64: list(range(33, 65))}
PADDED = sorted(CLASSES)
STORAGES = pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
LATTICES = [c for c in LA.CASES if c[0] == 13]               # (13, (2, 2), 8, (3, 4)) and (13, (3, 4), 8, (-5, -10))
LATTICE_FILLS = (17, 31, 32, 47, 48, 49, 63)                 # the second, third and fourth chunk of 16: one member, one short, full
# (N, M): the smallest sizes at which k_member_gram cuts a row into whole chunks and a shorter last one, and at which the
# chunks outnumber the 1024 blocks so that a block strides; CH = 4096 / gram_padded(M) cells
SHORT_CHUNK = [(66, 33), (130, 32), (258, 16)]
STRIDE = [(514, 8), (342, 32), (514, 16)]
NODE_IDENTITY = {32: (17, 24, 31, 32), 64: (33, 48, 63, 64)}


def power_of_two(m):
    return m & (m - 1) == 0


def test_the_classes_are_the_paddings():
    counts = [m for p in PADDED for m in CLASSES[p]]
    assert counts == list(range(1, 65))
    for p, ms in CLASSES.items():
        for m in ms:
            assert p // 2 < m <= p and power_of_two(p)
    assert len(LATTICES) == 2 and {c[1] for c in LATTICES} == {(2, 2), (3, 4)}
    for n, m in SHORT_CHUNK + STRIDE:
        ch = 4096 // max(8, [p for p in PADDED if m <= p][0])
        per_row = -(-n // ch)
        assert per_row > 1 and n % ch
        assert (per_row * n > 1024) == ((n, m) in STRIDE)


# ---- a. transform and select --------------------------------------------------------------------------------------------------
@STORAGES
@pytest.mark.parametrize("padded", PADDED)
def test_transform_and_select(padded, storage):
    for members in CLASSES[padded]:
        rng = np.random.default_rng(11000 + 100 * storage + members)
        ids = np.arange(members)
        for n in (6, 13):
            w = n + 2
            what = "n=%d M=%d storage=%d" % (n, members, storage)
            with TR.solver(n, members, storage) as s:
                for zeros in (True, False):                  # the table with a mask; the table where every term is taken
                    s.upload_members(u=TR.mixed_values(rng, (members, w, w), storage))
                    before = TR.shown(s, "u")
                    t = TR.mixed_weights(rng, members, zeros)
                    s.transform(t, fields=("u",))
                    now = TR.shown(s, "u")
                    TR.same(now, TR.narrow(TR.define(before, t), storage), "%s zeros=%s" % (what, zeros))
                for src in (np.roll(ids, 1), rng.integers(0, members, members)):        # the M-cycle; resampling with repeats
                    s.select(src, fields=("u",))
                    want = TR.narrow(TR.define(now, TR.onehot(src)), storage)
                    now = TR.shown(s, "u")
                    TR.same(now, want, "%s source=%s" % (what, list(src)))


# ---- b. transform_local -------------------------------------------------------------------------------------------------------
@STORAGES
@pytest.mark.parametrize("padded", PADDED)
def test_transform_local(padded, storage):
    n = 13
    w = n + 2
    box = (2, w - 3, 3, w - 2)                               # strictly inside the array
    outside = np.ones((w, w), bool)
    outside[box[0]:box[1], box[2]:box[3]] = False
    for members in CLASSES[padded]:
        rng = np.random.default_rng(12000 + 100 * storage + members)
        what = "n=%d M=%d storage=%d" % (n, members, storage)
        with LO.solver(n, members, storage) as s:
            s.upload_members(u=LO.mixed_values(rng, (members, w, w), storage))
            g = LO.random_taper(rng, w)
            before, after = LO.apply_and_check(s, "u", LO.mixed_increments(rng, members, zeros=True), g, box, storage,
                                               what + ": a taper, a box, increments with zeros")
            LO.same_bits(after[:, outside], before[:, outside], what + ": cells outside the box")
            LO.same_bits(after[:, g == 0], before[:, g == 0], what + ": cells under a zero taper")
            s.upload_members(u=LO.mixed_values(rng, (members, w, w), storage))
            LO.apply_and_check(s, "u", LO.mixed_increments(rng, members, zeros=False), None, None, storage,
                               what + ": the null taper, no box, every term taken")


# ---- c. transform_lattice -----------------------------------------------------------------------------------------------------
def lattice_call(s, members, storage, case, d, x, what):
    """one lattice call on `u` against the definition, and the cells that sit on a node against that node's local call"""
    n, nodes, step, origin = case
    w = n + 2
    s.upload_members(u=x)
    before, after = LA.apply_and_check(s, "u", d, origin, step, storage, what)
    for ia in range(nodes[0]):
        for ib in range(nodes[1]):
            i, j = origin[0] + ia * step, origin[1] + ib * step
            if 0 <= i < w and 0 <= j < w:
                LA.same(after[:, i, j], LA.narrow(LA.define_local(before[:, i:i + 1, j:j + 1], d[ia, ib]), storage)[:, 0, 0],
                        what + ": the cell on node (%d, %d)" % (ia, ib))
    return before, after


@STORAGES
@pytest.mark.parametrize("padded", PADDED)
def test_transform_lattice(padded, storage):
    for members in CLASSES[padded]:
        rng = np.random.default_rng(13000 + 100 * storage + members)
        with LA.solver(13, members, storage) as s:
            for case, zeros in zip(LATTICES, (True, False)):       # masked increments for one lattice, dense for the other
                n, nodes, step, origin = case
                what = "n=%d M=%d storage=%d nodes %s origin %s zeros=%s" % (n, members, storage, nodes, origin, zeros)
                lattice_call(s, members, storage, case, LA.mixed_increments(rng, nodes, members, zeros),
                             LA.mixed_values(rng, (members, n + 2, n + 2), storage), what)


@STORAGES
def test_transform_lattice_only_the_last_chunk_has_terms(storage):
    """The lattice update takes the new members in chunks of 16 and skips a chunk without a term.  Increments that are
    non-zero in the columns of the last chunk alone: the members of the earlier chunks keep their bits, the last chunk's
    members match the definition -- at every fill of the second, third and fourth chunk."""
    case = LATTICES[1]
    n, nodes, step, origin = case
    for members in LATTICE_FILLS:
        rng = np.random.default_rng(13500 + 100 * storage + members)
        first = 16 * ((members - 1) // 16)
        assert 16 <= first < members <= first + 16
        d = LA.mixed_increments(rng, nodes, members)
        d[:, :, :, :first] = rng.choice([0.0, -0.0], nodes + (members, first))
        assert (d[:, :, :, first:] != 0).any(axis=(0, 1, 2)).all()
        what = "n=%d M=%d storage=%d: terms in members %d .. %d only" % (n, members, storage, first, members - 1)
        with LA.solver(n, members, storage) as s:
            before, after = lattice_call(s, members, storage, case, d, LA.mixed_values(rng, (members, n + 2, n + 2), storage), what)
            LA.same_bits(after[:first], before[:first], what + ": the members of the earlier chunks")
            stored = LA.stored_mask(d, n + 2, origin, step)
            assert stored[first:].any(axis=(1, 2)).all() and not stored[:first].any()


# ---- d. member_gram -----------------------------------------------------------------------------------------------------------
@STORAGES
@pytest.mark.parametrize("padded", PADDED)
def test_member_gram(padded, storage):
    n = 13
    w = n + 2
    for members in CLASSES[padded]:
        rng = np.random.default_rng(14000 + 100 * storage + members)
        with GR.solver(n, members, storage) as s:
            x = rng.choice(GR.COARSE, size=(members, w, w)).astype(F32)
            s.upload_members(dens=x)
            before = s.download_members("dens")
            assert np.array_equal(before.view(np.uint32), x.view(np.uint32))
            for centre in (False, True):
                if centre and not power_of_two(members):     # a power of two: mean, anomalies and products are exact
                    continue
                what = "n=%d M=%d storage=%d centre=%s" % (n, members, storage, centre)
                got = s.member_gram("dens", centre=centre)
                GR.equal(got, GR.exact_gram(GR.define(before, centre), 8 if centre else 2), what)
                GR.symmetric(got, what)
            if not power_of_two(members):                     # centred, general data: the summation bound
                y = rng.uniform(0.25, 1.0, (members, w, w)) * rng.choice([-1.0, 1.0], (members, w, w)) + 50
                s.upload_members(v=y.astype(F32))
                before = s.download_members("v")
                what = "n=%d M=%d storage=%d centre=True, general data" % (n, members, storage)
                got = s.member_gram("v", centre=True)
                GR.within_bound(got, GR.define(before, True), n, what)
                GR.symmetric(got, what)


# ---- e. member_gram: the shorter last chunk of a row, blocks that stride over their chunks ------------------------------------------
@pytest.mark.parametrize("n,members,storage", [(n, m, 0) for n, m in SHORT_CHUNK + STRIDE] + [(n, m, 1) for n, m in SHORT_CHUNK],
                         ids=lambda v: str(v))
def test_member_gram_chunk_edges(n, members, storage):
    rng = np.random.default_rng(15000 + 1000 * storage + n + members)
    w = n + 2
    with GR.solver(n, members, storage) as s:
        x = rng.choice(GR.COARSE, size=(members, w, w)).astype(F32)
        s.upload_members(dens=x)
        before = s.download_members("dens")
        assert np.array_equal(before.view(np.uint32), x.view(np.uint32))
        for centre in (False, True):
            what = "n=%d M=%d storage=%d centre=%s" % (n, members, storage, centre)
            got = s.member_gram("dens", centre=centre)
            if centre and not power_of_two(members):         # (33 members: the mean is rounded, the bound takes the place of ==)
                GR.within_bound(got, GR.define(before, centre), n, what)
            else:
                GR.equal(got, GR.exact_gram(GR.define(before, centre), 8 if centre else 2), what)
            GR.symmetric(got, what)


# ---- f. observation_gram ------------------------------------------------------------------------------------------------------
@STORAGES
@pytest.mark.parametrize("padded", PADDED)
def test_observation_gram(padded, storage):
    """P = 1, 64, 65, 130: one point, a full chunk of 64, a chunk and one, three chunks with the last one short.  check_dyadic
    compares the matrix, rhs and dd each on its own, with and without obs and inv_sigma; rhs and dd are the sums that ride on
    the lanes below the diagonal."""
    n = 13
    w = n + 2
    for members in CLASSES[padded]:
        rng = np.random.default_rng(16000 + 100 * storage + members)
        with OB.solver(n, members, storage) as a, OB.solver(n, members, storage) as b:
            for p in (1, 64, 65, 130):
                x, cols, rows, y, sg = OB.dyadic_case(rng, n, members, p)
                for c in (a, b):
                    c.upload_members(dens=x)
                    c.set_observation_points(cols, rows)
                what = "M=%d storage=%d P=%d" % (members, storage, p)
                OB.check_dyadic(a, b, x, cols, rows, y, sg, members, what)         # exact: centre off, or M a power of two
                if power_of_two(members):
                    continue
                z = rng.uniform(0.25, 1.0, (members, w, w)) * rng.choice([-1.0, 1.0], (members, w, w)) + 50
                a.upload_members(v=z.astype(F32))
                h = OB.define_obs(a.download_members("v"), cols, rows)
                yg = (rng.normal(size=p) + 50).astype(F32)
                sgg = rng.uniform(0.5, 20.0, p).astype(F32)
                for obs, sigma in ((None, None), (yg, None), (None, sgg), (yg, sgg)):
                    wh = "%s centre=True, general data, obs=%s sigma=%s" % (what, obs is not None, sigma is not None)
                    got = a.observation_gram("v", obs=obs, inv_sigma=sigma, centre=True)
                    OB.within_bound(got, *OB.operands(h, obs, sigma, True), wh)
                    OB.symmetric(got[0] if obs is not None else got, wh)


# ---- g. observation_gram_lattice ------------------------------------------------------------------------------------------------
@STORAGES
@pytest.mark.parametrize("padded", PADDED)
def test_observation_gram_lattice(padded, storage):
    dyadic = [d for d in LG.DYADIC if d[:2] in ((13, 65), (6, 64))]
    assert len(dyadic) == 2
    for members in CLASSES[padded]:
        rng = np.random.default_rng(17000 + 100 * storage + members)
        for n, p, lat in dyadic:
            x = rng.choice(LG.COARSE, size=(members, n + 2, n + 2)).astype(F32)
            cols, rows = LG.dyadic_network(n, p, lat, rng)
            y = (rng.integers(-8, 9, p) / 4.0).astype(F32)
            sg = rng.choice(np.array([0.5, 1.0, 2.0], F32), p)
            w, r, _ = LG.weights(cols, rows, *lat, 1.0)
            assert (((r == 0) & (w == 1)) | ((r >= 2.5) & (w == 0))).all()
            with LG.solver(n, members, storage) as s:
                s.upload_members(dens=x)
                s.set_observation_points(cols, rows)
                h = LG.define_obs(x, cols, rows)               # multiples of 2^-6, exact in float32
                assert np.array_equal(s.observe("dens"), h)
                for centre in (False, True):
                    if centre and not power_of_two(members):
                        continue
                    for obs, sigma in ((None, None), (y, None), (None, sg), (y, sg)):
                        what = "M=%d storage=%d N=%d P=%d lattice %s centre=%s obs=%s sigma=%s" % (
                            members, storage, n, p, lat, centre, obs is not None, sigma is not None)
                        got = LG.call(s, "dens", lat, 1.0, obs, sigma, centre)
                        LG.check_shapes(got, lat, members)
                        gram, rhs, dd, counts = got
                        am, d = LG.operands(h, obs, sigma, centre)
                        empty = 0
                        for ia in range(lat[0][0]):
                            for ib in range(lat[0][1]):
                                idx = np.nonzero(w[ia, ib])[0]
                                assert counts[ia, ib] == len(idx), what
                                LG.equal(LG.pack_node(members, gram[ia, ib], None if obs is None else rhs[ia, ib],
                                                      None if obs is None else dd[ia, ib]),
                                         LG.exact_node(am, d, idx), "%s node (%d, %d)" % (what, ia, ib))
                                LG.symmetric(gram[ia, ib], what)
                                if len(idx) == 0:
                                    LG.plus_zero(got, ia, ib, what)
                                    empty += 1
                        assert 0 < empty < lat[0][0] * lat[0][1], "the lattice has nodes with points and nodes without"
        if members in NODE_IDENTITY.get(padded, CLASSES[padded]):
            one_node_is_the_observation_gram(members, storage, rng)


def one_node_is_the_observation_gram(members, storage, rng):
    """a 1 x 1 lattice with every point on its node and c = 1: fluid_observation_gram's bits"""
    n, lat = 13, ((1, 1), (5, 7), 8)
    with LG.solver(n, members, storage) as s:
        for p in (1, 65, 513):
            x = rng.choice(LG.COARSE, size=(members, n + 2, n + 2)).astype(F32)
            y = (rng.integers(-8, 9, p) / 4.0).astype(F32)
            sg = rng.choice(np.array([0.5, 1.0, 2.0], F32), p)
            s.upload_members(dens=x)
            s.set_observation_points(np.full(p, 7.0, F32), np.full(p, 5.0, F32))
            for centre in (False, True):
                if centre and not power_of_two(members):
                    continue
                for obs, sigma in ((None, None), (y, None), (None, sg), (y, sg)):
                    what = "one node: M=%d storage=%d P=%d centre=%s obs=%s sigma=%s" % (members, storage, p, centre, obs is not None, sigma is not None)
                    gram, rhs, dd, counts = LG.call(s, "dens", lat, 1.0, obs, sigma, centre)
                    want = s.observation_gram("dens", obs=obs, inv_sigma=sigma, centre=centre)
                    assert counts[0, 0] == p
                    if obs is None:
                        LG.same_bits(gram[0, 0], want, what)
                    else:
                        LG.same_bits(gram[0, 0], want[0], what)
                        LG.same_bits(rhs[0, 0], want[1], what + ": rhs")
                        LG.same_bits(dd[0, 0], np.float64(want[2]), what + ": dd")


# ---- h. etkf_increments ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [p for p in PADDED if p >= 2])
def test_etkf_increments(padded):
    """Every M in 2 .. 64 against numpy.linalg.eigh within the tolerance of tests/test_gpu_etkf.py, its constant 64 included.
    tests/test_etkf_abi.py runs the kernel's own ordering in float64 at every M on the CPU: at most 14 of the 28 sweeps and
    within 0.91 of the 64 units of M 2^-53 kappa (sqrt(rho) + max |w_ref|), so a miss here is the kernel's.
    Largest GPU error observed on an MI355X over all 63 counts, three rho and six node kinds, after the float term
    2^-23 |D_ref| is taken off: 0.004 units of the 64 (M = 52, rho = 2, "P=64 scale 300"; 0.003 at M = 26; nothing beyond the
    float term up to M = 16).  As a share of its whole tolerance the largest error is 0.499 (M = 47, rho = 2, "P=5"), the
    half ulp of the one rounding to float; the five counts of tests/test_gpu_etkf.py had shown 0.497."""
    worst, share = (-np.inf, ""), (-np.inf, "")
    for members in CLASSES[padded]:
        gram, rhs = EK.node_inputs(members)
        with EK.solver(14, members) as s:
            for rho in EK.RHOS:
                d, status = s.etkf_increments(gram, rhs, rho=rho)
                assert d.dtype == F32 and d.shape == (6, members, members) and status.dtype == np.int32
                assert (status == 0).all(), (members, rho, status)
                for b in range(6):
                    d_ref, w_ref, kappa = EK.reference(gram[b], rhs[b], rho)
                    tol = EK.tolerance(d_ref, w_ref, kappa, members, rho)
                    err = np.abs(d[b].astype(np.float64) - d_ref)
                    over = float(((err - 2.0 ** -23 * np.abs(d_ref)) / EK.unit(w_ref, kappa, members, rho)).max())
                    part = float((err / np.maximum(tol, 1e-300)).max())
                    key = "M=%d rho=%g %s" % (members, rho, EK.KINDS[b])
                    worst, share = max(worst, (over, key)), max(share, (part, key))
                    assert (err <= tol).all(), (key, over, part)
                if rho == 1.0:
                    assert (d[5].view(np.uint32) == 0).all(), "M=%d: C = 0, rhs = 0, rho = 1: every entry +0" % members
    print("padded %d: worst %.3f units of 64 beyond the float term (%s); the largest error is %.3f of its tolerance (%s)" % (
        (padded, max(worst[0], 0.0), worst[1] if worst[0] > 0 else "none") + share))


# ---- i. the same bits whatever the batch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [17, 32, 63])
def test_etkf_the_same_bits_whatever_the_batch(members):
    gram, rhs = EK.node_inputs(members)
    rng = np.random.default_rng(7)
    pick = np.concatenate([np.arange(6), rng.integers(0, 6, 294)])
    rng.shuffle(pick)
    with EK.solver(14, members) as s, EK.solver(14, members) as other:
        base, _ = s.etkf_increments(gram, rhs, rho=1.1)
        many, status = s.etkf_increments(gram[pick], rhs[pick], rho=1.1)            # 300 blocks: more than the chip has CUs
        assert (status == 0).all()
        assert np.array_equal(many.view(np.uint32), base[pick].view(np.uint32)), "every copy has its original's bytes"
        for b in range(6):
            one, _ = s.etkf_increments(gram[b:b + 1], rhs[b:b + 1], rho=1.1)
            assert np.array_equal(one.view(np.uint32), base[b:b + 1].view(np.uint32)), "a batch of one"
        again, _ = s.etkf_increments(gram[pick], rhs[pick], rho=1.1)
        assert np.array_equal(again.view(np.uint32), many.view(np.uint32)), "a second call"
        far, _ = other.etkf_increments(gram[pick], rhs[pick], rho=1.1)
        assert np.array_equal(far.view(np.uint32), many.view(np.uint32)), "a second context"


# ---- j. the fused analysis against the three calls ----------------------------------------------------------------------------------
@pytest.mark.parametrize("members,storage", [(4, 0), (16, 0), (17, 0), (32, 0), (63, 0), (32, 1)])
def test_the_fused_call_is_the_three_calls(members, storage):
    n = 30
    shape, origin, step, c, rho, listed = (3, 3), (-8, 0), 16, 6.0, 1.1, ("dens", "u", "v")
    rng = np.random.default_rng(19000 + 100 * members + storage)
    fields = EK.start_fields(n, members, rng)
    cols, rows = EK.network(rng)
    inv_sigma = rng.uniform(2.0, 8.0, cols.size).astype(F32)
    y = rng.uniform(0.2, 1.5, cols.size).astype(F32)
    what = "M=%d storage=%d lattice %s fields %s" % (members, storage, shape, listed)
    with EK.solver(n, members, storage) as a, EK.solver(n, members, storage) as b:
        for s in (a, b):
            s.upload_members(**fields)
            s.step(2, use_sources=True)                    # fp16: the pressure scale is live; the sources are marked zero
            s.set_observation_points(cols, rows)
        a.analyse_lattice("dens", shape, origin, step, c, y, inv_sigma=inv_sigma, rho=rho, fields=listed, wait=False)
        d, status, counts = EK.composed(b, "dens", shape, origin, step, c, y, inv_sigma, rho, listed)
        want = {"solved": int((status == 0).sum()), "empty": int((status == 1).sum()), "failed": int((status == 2).sum())}
        assert a.analyse_status() == want, what
        assert want["empty"] >= 3 and want["solved"] >= 2 and (counts[0] == 0).all(), counts
        assert want["failed"] == 0 and np.abs(d).max() > 1e-4
        EK.same_members(a, b, EK.MAIN, what)
        changed = [name for name in listed if not np.array_equal(a.download_members(name).view(np.uint32), fields[name].view(np.uint32))]
        assert changed == list(listed)
