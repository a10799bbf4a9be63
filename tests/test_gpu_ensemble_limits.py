"""GPU: ensembles at the member counts and field sizes include/fluid_amd.h promises -- the envelope the other ensemble
files (16 members where a kernel steps, 64 for the statistics, 1100 tiny ones for pack / unpack) stay far inside.

1. M = 21845, the most a context takes (3 solves x 21845 = 65535 blocks in z of the fused Jacobi kernel), on grids of
   n = 1 and n = 14: steps, per-member parameters, the ensemble diagnostics, pack / unpack / run.
2. n = 254, M = 10925, fp32: a member is 393,216 B, a field 4,295,884,800 B.  Member 5462 starts past 2^31 bytes, member
   10922 ends past 2^32 and members 10923 and 10924 START past it -- two members more than the 10923 at which a field
   first passes 4 GiB, because a member base kept in 32-bit bytes wraps only for a member that starts there (up to 10922
   the base is at most 4,294,705,152): with them a narrowed base in any kernel, signed or unsigned, serves a marked
   member from another's rows.  The host's whole-field byte counts (memsets, the arena's field offsets) pass 2^32 too.
   What does NOT pass 2^32 at this shape: element offsets (a base is at most 1.07e9 elements) and the tile table's member
   stride (32 words per member).  fp16 storage cannot pass 4 GiB on the field side (M is capped): the same shape, 2 GiB.
3. n = 1022 with 17 members: the bulk host copies move two groups through the 64 MiB staging buffer, the second ragged
   (16 + 1).  test_gpu_ensemble_io's (4094, 2) also moves two groups, but of one member each: no group there is ragged
   and none holds more than one member, so the case is kept.

Who is checked against what.  An ensemble starts from K = 8 oracle states, member m from state m % 8.  The CHECKED
members -- the ends of the range, the members either side of every third of it (section 2: either side of 2 GiB and
4 GiB), and 200 seeded random ones -- get two cells of their own (`marks`), so that a member served from another member's
base shows; they are compared bit for bit with the oracle (fp16: test_gpu_f16_steps' rounded model) run on their own
arrays.  Every other member must equal, bit for bit and compared on the device over the packed field, the first
unmarked member that started from the same state and parameters (its TWIN), and those twins are oracle-checked too.
No tolerance anywhere.

Measured, CPU side: the oracle's two steps for all 21845 members take 1.9 s at n = 1 and 5.3 s at n = 14 --
so at n = 1 with fp32 storage every member is marked and oracle-checked, at n = 14 the fixed set; the fp16 model costs
milliseconds per member and takes the fixed set at both sizes.

Measured on an MI355X (`--durations=0`): the 52 cases take 12.7 s together.  The slowest is the n = 1, fp32, fused case of
test_two_steps (2.7 s: it computes the all-member oracle reference the stream case then reuses), then
test_fp16_step_past_2_gib (1.25 s) and the n = 14 fp16 stream case (0.97 s); every other case is below 0.7 s -- the steps
past 4 GiB 0.4 s each, the 29 operator cases there 0.04-0.2 s, the section's fixture 0.15 s.  Section 2's peak device
memory is 80.2 GB: the 51.55 GB arena and 28.6 GB of torch tensors (six dense initial arrays of 2.86 GB, a pack, its
gather by twin and the comparison); the fixture prints that line under `-s` when it is torn down."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_ensemble import OPERATOR_NAMES, member_fields, operator_cases, play_ensemble, solver
from test_gpu_ensemble_io import bulk_against_the_loop, layout, mem_free, torch_
from test_gpu_ensemble_reduce import fsums, stats_model, stored
from test_gpu_f16_steps import model_of
from test_gpu_lazy_state import COARSE, NAMES, Model, absmax32, residual32, same_bits

pytestmark = pytest.mark.gpu
F32 = np.float32
DT, VISC, DIFF = 0.016, 0.0025, 0.1
M_MAX = 21845
K = 8
STATE_KINDS = ("parameters", "uniform", "coarse", "subnormal")      # finite: the oracle's own advection is defined on them
ENDS_AND_THIRDS = (0, 1, 7281, 7282, 14563, 14564, 21843, 21844)
# four values each, not one per member: every distinct beta costs a 2^32-input proof on the device (see the docstring of
# test_member_parameters_at_the_maximum_member_count)
DT_POOL = np.array([0.016, 0.1, 0.05, 0.008], F32)
DIFF_POOL = np.array([0.1, 0.0, 1e-4, 0.02], F32)
VISC_POOL = np.array([0.0025, 0.3, 0.0, 0.01], F32)
ALPHA_POOL = np.array([1.0, 0.36, 0.3, 2.25], F32)
BETA_POOL = np.array([4.0, 2.44, 2.0, 10.0], F32)


def fixed_set(members=M_MAX):
    extra = np.random.default_rng(members).choice(members, 200, replace=False)
    return np.unique(np.concatenate([np.array(ENDS_AND_THIRDS), extra]))


def marks(m, n):
    """a marked member's own two cells: (row, column, value for dens, value for u).  The pair of values is different for
    every member below 2^15, and each is a 9-bit dyadic number in [1, 2): exact in fp16 storage as well"""
    m = np.asarray(m)
    p = m % (n * n)
    return 1 + p // n, 1 + p % n, (1 + (m % 128) / 128).astype(F32), (1 + (m // 128) / 256).astype(F32)


class Plan:
    """An ensemble's initial state and who answers for whom."""

    def __init__(self, oracle, n, members, checked, seed, dyadic=False):
        self.n, self.members = n, members
        self.checked = np.unique(np.asarray(checked, np.int64))
        self.marked = np.zeros(members, bool)
        self.marked[self.checked] = True
        if dyadic:
            rng = np.random.default_rng(seed)
            self.states = [{k: rng.choice(COARSE, size=(n + 2, n + 2)).astype(F32) for k in NAMES} for _ in range(K)]
        else:
            self.states = member_fields(oracle, n, K, seed, kinds=STATE_KINDS)
        self._host = None

    def fields_of(self, m):
        f = {k: v.copy() for k, v in self.states[m % K].items()}
        if self.marked[m]:
            i, j, a, b = marks(m, self.n)
            f["dens"][i, j], f["u"][i, j] = a, b
        return f

    def host(self):
        """the six dense (members, W, W) host arrays"""
        if self._host is None:
            who = np.arange(self.members) % K
            out = {k: np.stack([st[k] for st in self.states])[who] for k in NAMES}
            i, j, a, b = marks(self.checked, self.n)
            out["dens"][self.checked, i, j] = a
            out["u"][self.checked, i, j] = b
            self._host = out
        return self._host

    def device(self, k):
        """one dense (members, W, W) array, built on the device"""
        torch = torch_()
        base = torch.from_numpy(np.stack([st[k] for st in self.states])).cuda()
        out = base[torch.arange(self.members, device="cuda") % K]
        if k in ("dens", "u"):
            i, j, a, b = marks(self.checked, self.n)
            at = [torch.from_numpy(np.asarray(x, np.int64)).cuda() for x in (self.checked, i, j)]
            out[at[0], at[1], at[2]] = torch.from_numpy(a if k == "dens" else b).cuda()
        return out

    def twins(self, pool=None):
        """(twin_of, answerable): twin_of[m] = the first unmarked member of m's class (state, and index into the parameter
        pools if there is one) for an unmarked m, m itself for a marked one; answerable = the marked members and those
        twins, the members the oracle is asked about"""
        cls = np.arange(self.members) % K
        if pool is not None:
            cls = cls + K * np.asarray(pool)
        twin_of = np.arange(self.members)
        plain = np.flatnonzero(~self.marked)
        if plain.size == 0:
            return twin_of, self.checked
        classes, first = np.unique(cls[plain], return_index=True)
        assert np.array_equal(classes, np.unique(cls)), "a class without an unmarked member"
        lut = np.zeros(cls.max() + 1, np.int64)
        lut[classes] = plain[first]
        twin_of[plain] = lut[cls[plain]]
        return twin_of, np.union1d(self.checked, plain[first])


class Shared:
    """What the cases of section 1 share, made once per module (the fixture `shared`): the plans of the 21845-member
    ensembles, and the two-step references, which cost up to 2 s of CPU each.  A reference is keyed by what it depends on
    -- the fp32 oracle does not depend on the Jacobi variant, the fp16 model does -- and is never modified."""

    def __init__(self, oracle):
        self.oracle, self.plans, self.refs = oracle, {}, {}

    def plan(self, n, everyone=False, dyadic=False):
        key = (n, everyone, dyadic)
        if key not in self.plans:
            self.plans[key] = Plan(self.oracle, n, M_MAX, np.arange(M_MAX) if everyone else fixed_set(), seed=n + 3, dyadic=dyadic)
        return self.plans[key]

    def two_steps(self, plan, who, n, storage, variant, params, calls):
        key = (n, storage, variant if storage else None)
        if key not in self.refs:
            ref = Reference(self.oracle, plan, who, storage, variant, params)
            for call in calls:
                self.refs[key] = ref.step(*call)
        return self.refs[key]


@pytest.fixture(scope="module")
def shared(oracle):
    return Shared(oracle)


def pool_index(members):
    return (np.arange(members) // K) % 4


def members_match(got, want, who, what):
    """got: (members, W, W) as downloaded; want: (len(who), W, W), the model's fields of the members `who`"""
    g = got[who]
    bad = (g.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(g) & np.isnan(want))
    if bad.any():
        rows = np.flatnonzero(bad.reshape(len(who), -1).any(1))
        same_bits(g[rows[0]], want[rows[0]], "%s: member %d (%d of the %d members asked about differ: %s ...)" % (
            what, who[rows[0]], rows.size, len(who), who[rows[:8]].tolist()))


def twins_agree(s, twin_of, what, fields=NAMES):
    """on the device, over the packed field: every member holds the bits of its twin"""
    torch = torch_()
    twin = torch.from_numpy(twin_of).cuda()
    for k in fields:
        p = s.pack(k).view(torch.int32).flatten(1)
        same = (p == p[twin]).all(1)
        if not bool(same.all()):
            bad = torch.nonzero(~same).flatten().cpu().numpy()
            raise AssertionError("%s: %s of %d members differs from the member that started equal to it; the first: %s (their twins %s)" % (
                what, k, bad.size, bad[:8].tolist(), twin_of[bad[:8]].tolist()))
        del p, same


class Reference:
    """The members `who`, each on its own arrays with its own scalars: the oracle (fp32 storage) or test_gpu_f16_steps'
    rounded model (fp16).  step() -> {field: (len(who), W, W)} as a download shows the fields after it."""

    def __init__(self, oracle, plan, who, storage, variant, params):
        self.o, self.who, self.storage, self.n = oracle, who, storage, plan.n
        fields = [plan.fields_of(int(m)) for m in who]
        self.mods = [model_of(oracle, plan.n, f, params, variant) for f in fields] if storage else fields

    def step(self, src, dt, diff, visc):
        out = {k: np.empty((len(self.who), self.n + 2, self.n + 2), F32) for k in NAMES}
        for r, (m, mod) in enumerate(zip(self.who, self.mods)):
            a = dict(dt=float(dt[m]), diff=float(diff[m]), visc=float(visc[m]))
            if self.storage:
                mod.step(src, a["dt"], a["diff"], a["visc"], 40)
                f = {k: mod.download(k) for k in NAMES}
            else:
                f = mod
                (self.o.step_src if src else self.o.step)(f["u"], f["v"], f["dens"], f["u_prev"], f["v_prev"], f["dens_prev"], **a)
            for k in NAMES:
                out[k][r] = f[k]
        return out


def constant(members, dt=DT, diff=DIFF, visc=VISC):
    return tuple(np.full(members, v, F32) for v in (dt, diff, visc))


# ---- 1. the maximum member count on tiny grids ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [3, 0], ids=["fused", "stream"])
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n", [1, 14])
def test_two_steps_at_the_maximum_member_count(oracle, shared, n, storage, variant):
    """A sourced step and a plain one on 21845 members, gridDim.z = 65535 in the three-solve launches, the fused kernel
    forced on (TB_MIN_CELLS = 0) and the single-sweep kernels (variant 0); download_members of all six fields against the
    oracle / the rounded model, the twins on the device, and the counters against a one-member context: the same
    launches, M times the sweeps -- and, for the fused kernel, that launches of three fields and several sweeps were
    among them (30 launches, 50 field launches, 400 sweeps for the two steps of one member)."""
    from fluidsimulationcuda_amd import capi
    params = {capi.PARAM_TB_MIN_CELLS: 0}
    plan = shared.plan(n, everyone=(n == 1 and storage == 0))
    twin_of, who = plan.twins()
    calls = [(True,) + constant(M_MAX), (False,) + constant(M_MAX)]
    want = shared.two_steps(plan, who, n, storage, variant, params, calls)
    counts = {}
    for members in (M_MAX, 1):
        with solver(n, members, params=params, variant=variant, storage=storage) as s:
            if members == 1:
                s.upload(**plan.fields_of(0))
            else:
                s.upload_members(**plan.host())
            s.timing_enable(True)
            s.timing_read(reset=True)
            s.step(1, use_sources=True)
            s.step(1)
            counts[members] = s.timing_read(reset=True)
            if members == 1:
                continue
            what = "n=%d M=%d storage=%d variant=%d" % (n, members, storage, variant)
            got = {k: s.download_members(k) for k in NAMES}
            twins_agree(s, twin_of, what)
    for k in NAMES:
        members_match(got[k], want[k], who, "%s: %s" % (what, k))
    one, all_ = counts[1], counts[M_MAX]
    print("\n%s: counters of one member %s" % (what, {k: v for k, v in one.items() if not k.endswith("_ms")}))
    if variant == 3:
        # That the fused kernel ran, and with all of z.  A step's solves are the batch of three diffusions -- one launch per
        # round of sweeps, or one per solve where their division modes differ (batch_sweep) -- and two pressure solves of one
        # field: every three-field launch counts one launch and three field launches, every other launch one of each.  So
        # the difference is twice the number of three-field launches, whose gridDim.z is 3 x 21845 = 65535 in the ensemble;
        # and a launch of the fused kernel makes at least two sweeps, where the single-sweep kernels make one.
        three, odd = divmod(one["jacobi_field_launches"] - one["jacobi_launches"], 2)
        assert three > 0 and odd == 0, "no launch swept three fields: %s" % one
        assert 2 * one["jacobi_field_launches"] <= one["sweeps"], "launches of a single sweep: %s" % one
    assert one["jacobi_launches"] > 0 and all_["jacobi_launches"] == one["jacobi_launches"], (one, all_)
    for k in ("jacobi_field_launches", "sweeps", "pressure_sweeps"):
        assert all_[k] == M_MAX * one[k] and one[k] > 0, (k, one, all_)
    for k in ("solves", "source_calls", "advection_calls", "projection_calls", "divergence_calls"):
        assert all_[k] == one[k], (k, one, all_)


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_member_parameters_at_the_maximum_member_count(oracle, shared, storage):
    """dt, diff and visc arrays of 21845 entries: the table of a three-solve launch is 3 x 21845 records of 40 bytes.

    The values come from pools of FOUR, member m taking entry (m // 8) % 4 of each.  That is a property of the library
    to know, not a shortcut of the test: fluid_division_mode proves every new (mode, beta) on the device over all 2^32
    float inputs, about 2.7 ms and a stream synchronise each (include/fluid_amd.h), once per process -- 21845 distinct
    viscosities and diffusivities would put two minutes of proofs in front of the first step.

    Three sourced steps (each consumes what the one before left in the *_prev fields, so every launch has the same form):
    a first call; the identical call again, whose tables' bytes are already in the ring -- the library has no counter a
    test could read for that, so what is held here is that the reused tables give the right bits; the call with ONE
    entry changed, member 7282's viscosity, which must change that member and nobody else."""
    from fluidsimulationcuda_amd import capi
    n = 14
    params = {capi.PARAM_TB_MIN_CELLS: 0}
    plan = shared.plan(n)
    q = pool_index(M_MAX)
    twin_of, who = plan.twins(pool=q)
    dt, diff, visc = DT_POOL[q], DIFF_POOL[q], VISC_POOL[q]
    visc2 = visc.copy()
    visc2[7282] = VISC_POOL[(q[7282] + 1) % 4]
    assert plan.marked[7282] and visc2[7282] != visc[7282]
    calls = [(True, dt, diff, visc), (True, dt, diff, visc), (True, dt, diff, visc2)]
    ref = Reference(oracle, plan, who, storage, 3, params)
    with solver(n, M_MAX, params=params, storage=storage) as s:
        s.upload_members(**plan.host())
        for c, (src, a, b, v) in enumerate(calls):
            s.step(1, use_sources=src, dt=a, diff=b, visc=v)
            what = "member parameters, storage=%d, call %d" % (storage, c + 1)
            want = ref.step(src, a, b, v)
            for k in NAMES:
                members_match(s.download_members(k), want[k], who, "%s: %s" % (what, k))
            twins_agree(s, twin_of, what)


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_diagnostics_at_the_maximum_member_count(oracle, shared, storage):
    """grids (blocks, 21845): the atomics of k_residual / k_absmax2 with one result word per member, k_member_moments
    with moment_blocks() clamped to one block per member, k_fold_moments over 21845 members, the statistics' member loop"""
    n = 14
    plan = shared.plan(n)
    q = pool_index(M_MAX)
    twin_of, who = plan.twins(pool=q)
    alpha, beta = ALPHA_POOL[q], BETA_POOL[q]
    host = plan.host()
    with solver(n, M_MAX, storage=storage) as s:
        s.upload_members(**host)
        for x, x0 in (("u", "u_prev"), ("dens", "v")):
            per = s.residual_members(x, x0, alpha, beta)
            same = s.residual_members(x, x0, 0.5, 3.0)
            assert per.dtype == F32 and per.shape == (M_MAX,) and not np.isnan(per).any()
            for m in who:
                fx, fx0 = stored(host[x][m], storage), stored(host[x0][m], storage)
                for got, a, b in ((per[m], alpha[m], beta[m]), (same[m], 0.5, 3.0)):
                    w = residual32(fx, fx0, a, b)
                    assert got.view(np.uint32) == w.view(np.uint32), "residual(%s, %s) of member %d: %r, the float model %r" % (x, x0, m, got, w)
            assert np.array_equal(per.view(np.uint32), per[twin_of].view(np.uint32)), "residual(%s, %s): a member differs from its twin" % (x, x0)
            assert np.array_equal(same.view(np.uint32), same[twin_of].view(np.uint32))
            assert F32(same.max()) == F32(s.residual(x, x0, 0.5, 3.0))
        per = s.absmax_velocity_members("u", "v")
        for m in who:
            w = absmax32(stored(host["u"][m], storage), stored(host["v"][m], storage))
            assert per[m].view(np.uint32) == w.view(np.uint32), "absmax of member %d: %r, the float model %r" % (m, per[m], w)
        assert np.array_equal(per.view(np.uint32), per[twin_of].view(np.uint32))
        assert F32(per.max()) == F32(s.absmax_velocity("u", "v"))
        # statistics across the 21845 members: the header's definition as a numpy loop, every cell (256 of them)
        x = stored(host["u"], storage)
        want_mean, want_var = stats_model(x)
        mean, var = s.ensemble_stats("u")
        same_bits(mean, want_mean, "mean over %d members" % M_MAX)
        same_bits(var, want_var, "variance over %d members" % M_MAX)
        # moments on dyadic data: every partial sum is representable, so the sum is exact in any order -- numpy's for all
        # members, math.fsum for the marked ones
        dyadic = shared.plan(n, dyadic=True)
        d = dyadic.host()["dens"]
        s.upload_members(dens=d)
        sums, squares = s.member_moments("dens")
        inner = d[:, 1:-1, 1:-1].astype(np.float64)
        assert sums.dtype == np.float64 and np.array_equal(sums, inner.sum((1, 2))) and np.array_equal(squares, (inner * inner).sum((1, 2)))
        for m in dyadic.checked:
            assert (sums[m], squares[m]) == fsums(d[m]), "moments of member %d: (%r, %r), fsum %r" % (m, sums[m], squares[m], fsums(d[m]))


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_moving_the_maximum_member_count(oracle, shared, storage):
    """pack / unpack over all 21845 members and over the ranges [21844, +1) and [7000, 9000); run and run_members recording two
    snapshots of one field (four steps, one snapshot after every second: nsteps / every cannot be 2 with three steps),
    against the call-by-call loop on a second context"""
    torch = torch_()
    n, iters = 14, 8
    plan = shared.plan(n)
    host = plan.host()
    u, v = stored(host["u"], storage), stored(host["v"], storage)
    q = pool_index(M_MAX)

    def bits(t):
        return t.contiguous().view(torch.int32)

    with solver(n, M_MAX, storage=storage) as s, solver(n, M_MAX, storage=storage) as loop:
        s.upload_members(**host)
        loop.upload_members(**host)
        dev_u = torch.from_numpy(u).cuda()
        assert torch.equal(bits(s.pack("u")), bits(dev_u)), "pack of all members"
        same_bits(s.download_members("u").reshape(-1, n + 2), u.reshape(-1, n + 2), "download_members")
        for first, count in ((M_MAX - 1, 1), (M_MAX - 1, 0), (7000, 2000)):
            got = s.pack("u", first=first, count=count)
            moved = count or M_MAX - first
            assert tuple(got.shape) == (moved, n + 2, n + 2) and torch.equal(bits(got), bits(dev_u[first:first + moved])), "pack [%d, +%d)" % (first, count)
        want = u.copy()
        for first, count in ((7000, 2000), (M_MAX - 1, 1)):
            s.unpack("u", torch.from_numpy(host["v"][first:first + count]).cuda(), first=first, count=count)
            want[first:first + count] = v[first:first + count]
            assert torch.equal(bits(s.pack("u")), bits(torch.from_numpy(want).cuda())), "unpack [%d, +%d)" % (first, count)
        s.unpack("u", torch.from_numpy(host["u"]).cuda())
        assert torch.equal(bits(s.pack("u")), bits(dev_u)), "unpack of all members"
        del dev_u
        for kind, args in (("run", dict(dt=DT, diff=DIFF, visc=VISC)), ("run_members", dict(dt=DT_POOL[q], diff=DIFF_POOL[q], visc=VISC_POOL[q]))):
            got, written = s.run(4, every=2, fields=("dens",), iters=iters, use_sources=True, **args)
            assert written == 2 and tuple(got.shape) == (2, 1, M_MAX, n + 2, n + 2)
            for z in range(4):
                loop.step(1, use_sources=(z == 0), iters=iters, **args)
                if z % 2 == 1:
                    assert torch.equal(bits(got[z // 2, 0]), bits(loop.pack("dens"))), "%s: snapshot %d" % (kind, z // 2)
            for k in NAMES:
                assert torch.equal(bits(s.pack(k)), bits(loop.pack(k))), "%s: %s after the run" % (kind, k)
            del got


def test_one_member_too_many_allocates_nothing():
    """21846 members: refused by fluid_create_ensemble, size 0 from fluid_arena_bytes_ensemble (tests/test_ensemble_abi.py
    holds both without a device), and on a live device no memory has gone: hipMemGetInfo before and after, within the
    16 MiB of test_destroy_frees_the_staging_buffer (one member fewer takes 2 GiB less 32 KiB)"""
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    with solver(14, 2):
        pass
    torch_().cuda.synchronize()
    before = mem_free()
    cfg = capi.Config(n=14, rank=0, nranks=1, halo=0, jacobi_variant=3, stream=None, arena=None, arena_bytes=0, storage=0)
    h = C.c_void_p(0x1234)
    assert L.fluid_create_ensemble(C.byref(cfg), M_MAX + 1, C.byref(h)) == capi.E_INVALID and not h.value
    assert b"members" in L.fluid_last_error()
    assert L.fluid_arena_bytes_ensemble(14, 0, M_MAX + 1) == 0 and L.fluid_arena_bytes_ensemble(14, 0, M_MAX) == 12 * M_MAX * 8192 + 256
    assert abs(mem_free() - before) <= 16 << 20


# ---- 2. a field past 2 GiB and 4 GiB ---------------------------------------------------------------------------------------------
BIG_N, BIG_M = 254, 10925
# either side of 2 GiB (member 5462 is the first that starts past 2^31 bytes) and of 4 GiB (10922 straddles 2^32, 10923 is
# the first that starts past it)
BIG_CHECKED = (0, 1, 5461, 5462, 5463, 10921, 10922, 10923, 10924)


class Big:
    pass


@pytest.fixture(scope="module")
def big(oracle):
    """one context of 10925 members of 254^2 for the whole section, its six dense initial arrays on the device; every
    case starts by unpacking them (an unpack of all members replaces the field and drops what it owed itself)"""
    from fluidsimulationcuda_amd import capi
    torch = torch_()
    pitch, xoff, ff = layout(BIG_N)
    assert pitch == 384 and ff * 4 == 393216
    assert 5461 * ff * 4 < 1 << 31 < 5462 * ff * 4 and 10922 * ff * 4 < 1 << 32 < 10923 * ff * 4 and BIG_M == 10925
    arena = capi.lib().fluid_arena_bytes_ensemble(BIG_N, 0, BIG_M)
    dense = BIG_M * (BIG_N + 2) ** 2 * 4
    need = arena + 12 * dense            # six initial arrays, and room for a pack, its gather and the float64 mean
    free, total = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("n=254, M=10925 needs %.1f GB of device memory (arena %.1f GB), %.1f GB of %.1f GB are free" % (
            need / 1e9, arena / 1e9, free / 1e9, total / 1e9))
    torch.cuda.reset_peak_memory_stats()
    b = Big()
    b.free0 = free
    b.low = free
    b.plan = Plan(oracle, BIG_N, BIG_M, BIG_CHECKED, seed=254)
    b.dense = {k: b.plan.device(k) for k in NAMES}
    b.s = solver(BIG_N, BIG_M, params={capi.PARAM_TB_MIN_CELLS: 0})

    def fresh():
        for k in NAMES:
            b.s.unpack(k, b.dense[k])

    def done():
        b.low = min(b.low, torch.cuda.mem_get_info()[0])

    b.fresh, b.done = fresh, done
    yield b
    b.s.close()
    # (shown with -s.  The peak is the library's arena plus the most torch had allocated at one time since the fixture began --
    # the dense arrays, a pack, the comparisons' scratch; "taken from the device" is what left the device's free memory by
    # the end of some case, torch's cache of freed blocks included)
    peak = arena + torch.cuda.max_memory_allocated()
    print("\nsection 2: peak device memory %.1f GB (arena %.1f GB + torch %.1f GB); taken from the device %.1f GB of the %.1f GB free before" % (
        peak / 1e9, arena / 1e9, (peak - arena) / 1e9, (b.free0 - b.low) / 1e9, b.free0 / 1e9))


def big_compare(b, models, who, twin_of, what, fields=NAMES):
    for m, mod in zip(who, models):
        for k in fields:
            same_bits(b.s.download(k, member=int(m)), mod.f[k], "%s: member %d, %s" % (what, m, k))
    twins_agree(b.s, twin_of, what, fields)
    b.done()


@pytest.mark.parametrize("name", OPERATOR_NAMES)
def test_operator_past_4_gib(oracle, big, name):
    """every operator of test_gpu_ensemble's table on the 4.3 GB fields: the marked members and the eight twins against
    the oracle, everyone else against its twin on the device"""
    _, cases = operator_cases(*oracle.coefficients(BIG_N, DT, VISC))
    twin_of, who = big.plan.twins()
    models = [Model(oracle, big.plan.fields_of(int(m))) for m in who]
    big.fresh()
    for op in cases[name]:
        play_ensemble(big.s, models, op, name)
    big_compare(big, models, who, twin_of, name)


@pytest.mark.parametrize("fast_div", [2, 1])
def test_steps_past_4_gib(oracle, big, fast_div):
    """a sourced and a plain step through the fused kernel; TB_FAST_DIVISION = 1 puts the viscous solves on the two-term
    reciprocal, whose tile minima lie member x tile_mstride words into their table"""
    from fluidsimulationcuda_amd import capi
    twin_of, who = big.plan.twins()
    models = [Model(oracle, big.plan.fields_of(int(m))) for m in who]
    big.fresh()
    big.s.set_param(capi.PARAM_TB_FAST_DIVISION, fast_div)
    try:
        if fast_div == 1:
            assert big.s.division_mode(*oracle.coefficients(BIG_N, DT, VISC)) == 3, "the two-term division was not proven"
        for src in (True, False):
            big.s.step(1, use_sources=src)
            for mod in models:
                mod.step(src, DT, DIFF, VISC, 40)
            big_compare(big, models, who, twin_of, "fast_div %d, %s step" % (fast_div, "sourced" if src else "plain"))
    finally:
        big.s.set_param(capi.PARAM_TB_FAST_DIVISION, 2)


def test_member_parameter_step_past_4_gib(oracle, big):
    """fluid_step_members with the pooled parameters: 32 classes of twins, each member's own scalars for the oracle"""
    q = pool_index(BIG_M)
    twin_of, who = big.plan.twins(pool=q)
    dt, diff, visc = DT_POOL[q], DIFF_POOL[q], VISC_POOL[q]
    models = [Model(oracle, big.plan.fields_of(int(m))) for m in who]
    big.fresh()
    big.s.step(1, use_sources=True, dt=dt, diff=diff, visc=visc)
    for m, mod in zip(who, models):
        mod.step(True, float(dt[m]), float(diff[m]), float(visc[m]), 40)
    big_compare(big, models, who, twin_of, "per-member parameters")


def dyadic_field(oracle, big):
    """a dyadic (members, W, W) array on the device -- eight coarse states, the marked members' own cells -- and its plan"""
    plan = Plan(oracle, BIG_N, BIG_M, BIG_CHECKED, seed=255, dyadic=True)
    return plan, plan.device("dens")


def test_maxima_and_moments_past_4_gib(oracle, big):
    q = pool_index(BIG_M)
    twin_of, who = big.plan.twins(pool=q)
    alpha, beta = ALPHA_POOL[q], BETA_POOL[q]
    big.fresh()
    s = big.s
    per = s.residual_members("u", "u_prev", alpha, beta)
    vel = s.absmax_velocity_members("u", "v")
    for m in who:
        f = big.plan.fields_of(int(m))
        w = residual32(f["u"], f["u_prev"], alpha[m], beta[m])
        assert per[m].view(np.uint32) == w.view(np.uint32), "residual of member %d: %r, the float model %r" % (m, per[m], w)
        w = absmax32(f["u"], f["v"])
        assert vel[m].view(np.uint32) == w.view(np.uint32), "absmax of member %d: %r, the float model %r" % (m, vel[m], w)
    for a in (per, vel):
        assert np.array_equal(a.view(np.uint32), a[twin_of].view(np.uint32)), "a member's maximum differs from its twin's"
    same = s.residual_members("u", "u_prev", 0.5, 3.0)
    assert F32(same.max()) == F32(s.residual("u", "u_prev", 0.5, 3.0)) and F32(vel.max()) == F32(s.absmax_velocity("u", "v"))
    plan, dense = dyadic_field(oracle, big)
    s.unpack("dens", dense)
    sums, squares = s.member_moments("dens")
    plain_twin, answerable = plan.twins()
    for m in answerable:
        assert (sums[m], squares[m]) == fsums(plan.fields_of(int(m))["dens"]), "moments of member %d" % m
    assert np.array_equal(sums, sums[plain_twin]) and np.array_equal(squares, squares[plain_twin])
    big.done()


def test_mean_field_past_4_gib(oracle, big):
    """dyadic data: the sum over the 10925 members is exact in double whatever the order, so the mean field equals torch's
    float64 mean of the packed array bit for bit (sum / M in double, rounded to float once)"""
    torch = torch_()
    plan, dense = dyadic_field(oracle, big)
    big.s.unpack("dens", dense)
    packed = big.s.pack("dens")
    assert torch.equal(packed.view(torch.int32), dense.view(torch.int32))
    want = (packed.double().sum(0) / float(BIG_M)).float().cpu().numpy()
    del packed
    mean, var = big.s.ensemble_stats("dens")
    same_bits(mean, want, "mean over %d members of 254^2" % BIG_M)
    assert np.isfinite(var).all() and (var >= 0).all()
    big.done()


def test_fp16_step_past_2_gib(oracle):
    """fp16 storage at the same shape: a field is 2,147,942,400 B -- past 2 GiB; past 4 GiB it cannot go, M is capped.  The
    same fill and one sourced step: the marked members and the twins against the rounded model, the rest on the device."""
    from fluidsimulationcuda_amd import capi
    torch = torch_()
    pitch, xoff, ff = layout(BIG_N)
    assert 10922 * ff * 2 < 1 << 31 < 10923 * ff * 2 <= BIG_M * ff * 2
    arena = capi.lib().fluid_arena_bytes_ensemble(BIG_N, capi.STORAGE_F16, BIG_M)
    dense = BIG_M * (BIG_N + 2) ** 2 * 4
    free, total = torch.cuda.mem_get_info()
    if free < arena + 4 * dense:
        pytest.skip("fp16, n=254, M=10925 needs %.1f GB of device memory, %.1f GB are free" % ((arena + 4 * dense) / 1e9, free / 1e9))
    params = {capi.PARAM_TB_MIN_CELLS: 0}
    plan = Plan(oracle, BIG_N, BIG_M, BIG_CHECKED, seed=254)
    twin_of, who = plan.twins()
    with solver(BIG_N, BIG_M, params=params, storage=capi.STORAGE_F16) as s:
        for k in NAMES:
            d = plan.device(k)
            s.unpack(k, d)
            del d
        s.step(1, use_sources=True)
        for m in who:
            mod = model_of(oracle, BIG_N, plan.fields_of(int(m)), params)
            mod.step(True, DT, DIFF, VISC, 40)
            for k in NAMES:
                same_bits(s.download(k, member=int(m)), mod.download(k), "fp16: member %d, %s" % (m, k))
        twins_agree(s, twin_of, "fp16 past 2 GiB")


# ---- 3. staging groups -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", [17, 3])
def test_bulk_copies_in_ragged_groups(members, storage):
    """n = 1022: a member is 4 MiB dense, the staging buffer holds 16 -- 17 members go as a group of 16 and a group of
    one; 3 members are the one-group control"""
    assert (64 << 20) // (1024 * 1024 * 4) == 16
    bulk_against_the_loop(1022, members, storage, seed=1022 + members)
