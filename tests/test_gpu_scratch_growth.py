"""GPU: the library-owned scratch of the ensemble calls (csrc/fluid_ctx.h: Scratch) when it is first allocated and when it
grows -- under an analysis still in flight, with a larger network, and with the first uses in either order.

A context whose buffers were allocated, grown or merely found large enough must return what a fresh context returns that
makes only the call in question from the same uploaded state.  Every comparison is of bits; no tolerance is involved."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = np.float32
NAMES = ("u", "v", "dens", "u_prev", "v_prev", "dens_prev")
SHAPES = [(13, 3), (30, 33)]                  # (N, members): 3 is padded to the kernels' member tiles, 33 crosses one
C_TAPER, STEP = 6.0, 8


def solver(n, members, storage=0):
    import fluidsimulationcuda_amd as f
    return f.FluidSolver(n, members=members, storage=storage)


def start_fields(n, members, rng):
    w = n + 2
    out = {"dens": rng.uniform(0.5, 2.0, (members, w, w)).astype(F32)}
    for name in ("u", "v"):
        out[name] = rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32)
    for name in ("u_prev", "v_prev", "dens_prev"):
        out[name] = rng.uniform(0.0, 0.5, (members, w, w)).astype(F32)
    return out


def put(s, fields):
    """member by member: fluid_upload_member goes through none of the scratch buffers"""
    for m in range(s.members):
        s.upload(member=m, **{name: a[m] for name, a in fields.items()})


def get(s):
    """all six fields, member by member (fluid_download_member: no scratch either)"""
    return tuple(np.stack([s.download(name, member=m) for m in range(s.members)]) for name in NAMES)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.kind == "f" else a


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (x, y) in enumerate(zip(got, want)):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert np.array_equal(bits(x), bits(y)), "%s: array %d differs" % (what, k)


def network(n, points, rng):
    """(cols, rows, obs, inv_sigma) of `points` points anywhere in the domain"""
    return (rng.uniform(0.5, n + 0.5, points).astype(F32), rng.uniform(0.5, n + 0.5, points).astype(F32),
            rng.uniform(0.2, 1.5, points).astype(F32), rng.uniform(2.0, 8.0, points).astype(F32))


# ---- 1. the node tables, the node results and the lists grow while an analysis may still be queued -------------------------
@pytest.mark.parametrize("storage", [0, 1])
@pytest.mark.parametrize("n,members", SHAPES)
def test_growth_under_an_analysis_in_flight(n, members, storage):
    rng = np.random.default_rng(10 * members + storage)
    fields = start_fields(n, members, rng)
    cols, rows, y, inv_sigma = network(n, 40, rng)
    small = ((2, 2), (4, 4))                               # shape, origin: 4 nodes
    large = ((4, 4), (-4, 0))                              # 16 nodes about another origin: every buffer of the call grows

    def analyse(s, lattice, wait):
        s.analyse_lattice("dens", lattice[0], lattice[1], STEP, C_TAPER, y, inv_sigma=inv_sigma, rho=1.1, fields=("dens", "u", "v"),
                          wait=wait)

    def prepared():
        s = solver(n, members, storage)
        put(s, fields)
        s.step(1, use_sources=True)                        # fp16: the pressure scale is live
        s.set_observation_points(cols, rows)
        return s

    with prepared() as a, prepared() as b:
        analyse(a, small, False)
        analyse(a, large, False)                           # at once: the first call's launches may still be queued
        a.synchronize()
        got = a.analyse_status()
        analyse(b, small, True)
        analyse(b, large, True)
        want = b.analyse_status()
        what = "N=%d M=%d storage=%d" % (n, members, storage)
        assert got == want, what
        assert want["solved"] >= 1 and sum(want.values()) == 16, want
        for name in NAMES:
            same((a.download_members(name),), (b.download_members(name),), "%s: %s" % (what, name))
        assert not np.array_equal(bits(a.download_members("dens")), bits(fields["dens"])), "the analyses changed nothing"


# ---- 2. a larger network grows the operands and the partials; a smaller one finds them large enough -----------------------
@pytest.mark.parametrize("n,members", SHAPES)
def test_point_growth(n, members):
    rng = np.random.default_rng(20 * members)
    fields = start_fields(n, members, rng)
    few, many = network(n, 65, rng), network(n, 513, rng)
    shape, origin = (3, 3), (2, 2)

    def lattice(s, net):
        return s.observation_gram_lattice("dens", shape, origin, STEP, C_TAPER, obs=net[2], inv_sigma=net[3], centre=True)

    def plain(s, net):
        g, rhs, dd = s.observation_gram("dens", obs=net[2], inv_sigma=net[3], centre=True)
        return g, rhs, np.float64(dd).reshape(1)

    def fresh(net, call):
        with solver(n, members) as s:
            put(s, fields)
            s.set_observation_points(net[0], net[1])
            return call(s, net)

    want = {("few", "lattice"): fresh(few, lattice), ("many", "lattice"): fresh(many, lattice), ("many", "plain"): fresh(many, plain)}
    assert want["few", "lattice"][3].sum() > 0 and want["many", "lattice"][3].sum() > want["few", "lattice"][3].sum()
    with solver(n, members) as s:
        put(s, fields)
        for name, net, calls in (("few", few, (lattice,)), ("many", many, (lattice, plain)), ("few", few, (lattice,))):
            s.set_observation_points(net[0], net[1])
            for call in calls:
                same(call(s, net), want[name, call.__name__], "N=%d M=%d: %d points, %s" % (n, members, net[0].size, call.__name__))


# ---- 3. no first-use allocation depends on another having happened first -------------------------------------------------------
def first_uses(n, members, rng):
    """name -> call: every call that allocates a buffer at its first use, each returning a tuple of arrays -- its results, or
    for a call that changes the fields, the six fields after it"""
    weights = (np.eye(members) + rng.uniform(-0.1, 0.1, (members, members))).astype(F32)
    increments = rng.uniform(-0.05, 0.05, (2, 2, members, members)).astype(F32)
    dt = np.linspace(0.01, 0.02, members).astype(F32)

    def transform(s):
        s.transform(weights, fields=("u", "dens"))
        return get(s)

    def transform_lattice(s):
        s.transform_lattice(increments, (4, 4), STEP, fields=("v", "dens"))
        return get(s)

    def step_members(s):                                   # one dt per member: the constants ring
        s.step(1, dt=dt)
        return get(s)

    return {"member_gram": lambda s: (s.member_gram("dens", centre=True),),
            "ensemble_stats": lambda s: s.ensemble_stats("u"),
            "member_moments": lambda s: s.member_moments("v"),
            "transform": transform,
            "transform_lattice": transform_lattice,
            "download_members": lambda s: (s.download_members("dens"),),
            "step_members": step_members}


@pytest.mark.parametrize("n,members", SHAPES)
def test_first_use_order_does_not_matter(n, members):
    """Three of the calls change the fields and do not commute, so every call of a sequence starts from the uploaded state,
    put back member by member (which touches no scratch): a call's result is then what a fresh context returns that makes
    only that call, whatever ran before it, and the fields a sequence leaves are those its last call leaves."""
    rng = np.random.default_rng(30 * members)
    fields = start_fields(n, members, rng)
    calls = first_uses(n, members, rng)
    want = {}
    for name, call in calls.items():
        with solver(n, members) as s:
            put(s, fields)
            want[name] = call(s)
    assert not np.array_equal(bits(want["transform"][0]), bits(want["step_members"][0]))
    for order in (list(calls), list(calls)[::-1]):
        with solver(n, members) as s:
            for name in order:
                put(s, fields)
                same(calls[name](s), want[name], "N=%d M=%d, %s in the order %s" % (n, members, name, order))
            last = want[order[-1]] if len(want[order[-1]]) == len(NAMES) else tuple(fields[k] for k in NAMES)
            same(get(s), last, "N=%d M=%d: the fields after %s" % (n, members, order))
