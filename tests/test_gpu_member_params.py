"""GPU: one dt, diff and visc (alpha, beta) PER MEMBER of an ensemble -- fluid_step_members and its kin, reached through
FluidSolver by passing a sequence where a scalar went.

The rule: after any sequence of calls member m holds, in every field, exactly the bits the oracle (a one-member context where
the oracle cannot be asked: fp16 storage, the large grid) gives for the same calls with member m's own scalars.  Bit for bit,
NaN where the oracle has NaN; no tolerance and no case left out on data grounds.  And all members go through the same
launches: the counters of a per-member call equal those of the scalar call on a twin context.

Timings of the whole file on an MI355X are in DESIGN.md section 9."""
import ctypes as C
import zlib

import numpy as np
import pytest

from conftest import rnd
from test_gpu_ensemble import KINDS, STEP_CASES, STEP_SEQUENCE, compare_all, member_fields, solver, upload_all
from test_gpu_f16_steps import make_fields
from test_gpu_lazy_state import NAMES, Model, same_bits

pytestmark = pytest.mark.gpu
F32 = np.float32
# the values test_gpu_random_configs.py draws from
DTS, DIFFS, VISCS = (0.016, 0.1), (0.1, 0.0, 1e-4), (0.0025, 0.0, 0.3)


def triples(members, seed):
    """(dt, diff, visc) as three float32 arrays: member m takes the values above in rotation (starting at `seed`), diff and
    visc times 1 + m / 8, so the betas of the members whose coefficient is not 0 are all distinct (0 stays 0: beta 1)"""
    m = np.arange(members)
    factor = (1.0 + m / 8.0)
    dt = np.array([DTS[(seed + k) % 2] for k in m], F32)
    diff = (np.array([DIFFS[(seed + k) % 3] for k in m]) * factor).astype(F32)
    visc = (np.array([VISCS[(seed + 2 * k) % 3] for k in m]) * factor).astype(F32)
    return dt, diff, visc


def run_members(s, models, P, iters, what, sequence=STEP_SEQUENCE, compare=True):
    """test_gpu_ensemble.run_sequence with member m's own scalars: the library once, the model per member"""
    dt, diff, visc = P
    for k, call in enumerate(sequence):
        if call[0] == "step":
            s.step(1, use_sources=call[1], dt=dt, diff=diff, visc=visc, iters=iters)
        elif call[0] == "vel_step":
            s.vel_step(visc, dt, iters)
        else:
            s.dens_step(diff, dt, iters)
        for m, mod in enumerate(models):
            a = (float(dt[m]), float(diff[m]), float(visc[m]))
            if call[0] == "step":
                mod.step(call[1], a[0], a[1], a[2], iters)
            elif call[0] == "vel_step":
                mod.vel_step(a[2], a[0], iters)
            else:
                mod.dens_step(a[1], a[0], iters)
        if compare:
            compare_all(s, models, "%s: call %d %r" % (what, k + 1, call))


# ---- 1. steps against the oracle per member ---------------------------------------------------------------------------
@pytest.mark.parametrize("n, iters, members", STEP_CASES)
def test_steps_match_oracle_per_member(oracle, n, iters, members):
    fields = member_fields(oracle, n, members, seed=n + iters)
    models = [Model(oracle, f) for f in fields]
    P = triples(members, n + iters)
    with solver(n, members) as s:
        upload_all(s, fields)
        run_members(s, models, P, iters, "n=%d iters=%d M=%d %r" % (n, iters, members, P))


def knob_cases():
    from fluidsimulationcuda_amd import capi
    out = [("variant", v, {}) for v in (0, 1, 2)]
    out += [("fuse_add_source", 3, {capi.PARAM_FUSE_ADD_SOURCE: v}) for v in (0, 1)]
    out += [("fast_division", 3, {capi.PARAM_TB_FAST_DIVISION: v}) for v in (0, 1, 2, 3)]
    out += [("min_cells", 3, {capi.PARAM_TB_MIN_CELLS: 1 << 30})]           # the single-sweep path
    out += [("lane_columns", 3, {capi.PARAM_TB_LANE_COLUMNS: v}) for v in (2, 4)]
    out += [("deep_launches", 3, {capi.PARAM_TB_T16_MIN_CELLS: 0})]         # 16 + 12 + 12, ADDSRC at 16
    return out


KNOBS = knob_cases()


@pytest.mark.parametrize("case", range(len(KNOBS)), ids=["%s-%s" % (k[0], "-".join(str(v) for v in k[2].values()) or k[1]) for k in KNOBS])
def test_knob_with_member_parameters(oracle, case):
    name, variant, params = KNOBS[case]
    n, iters, members = 129, 40, 5
    fields = member_fields(oracle, n, members, seed=case)
    models = [Model(oracle, f) for f in fields]
    P = triples(members, case)
    with solver(n, members, params=params, variant=variant) as s:
        upload_all(s, fields)
        run_members(s, models, P, iters, "%s %r %r" % (name, params, P))


# ---- 2. same launches ---------------------------------------------------------------------------------------------------
COUNTERS = ("jacobi_launches", "jacobi_field_launches", "sweeps", "solves", "pressure_sweeps", "source_calls", "diffusion_calls",
            "divergence_calls", "projection_calls", "advection_calls")


@pytest.mark.parametrize("variant", [3, 0])
@pytest.mark.parametrize("fuse_add_source", [0, 1])
def test_member_step_issues_the_scalar_steps_launches(oracle, variant, fuse_add_source):
    from fluidsimulationcuda_amd import capi
    n, iters, members = 61, 20, 4
    fields = member_fields(oracle, n, members, seed=2, kinds=("parameters", "uniform"))
    P = triples(members, 1)
    counts = []
    for args in (dict(dt=0.016, diff=0.1, visc=0.0025), dict(dt=P[0], diff=P[1], visc=P[2])):
        with solver(n, members, variant=variant, params={capi.PARAM_FUSE_ADD_SOURCE: fuse_add_source}) as s:
            upload_all(s, fields)
            s.timing_enable(True)
            s.timing_read(reset=True)
            s.step(1, use_sources=True, iters=iters, **args)
            s.step(2, iters=iters, **args)
            s.vel_step(args["visc"], args["dt"], iters)
            s.dens_step(args["diff"], args["dt"], iters)
            s.add_source("u", "u_prev", args["dt"])
            s.diffuse(1, "u", "u_prev", 1.5 if np.ndim(args["dt"]) == 0 else [1.5, 0.5, 1.0, 0.25],
                      7.0 if np.ndim(args["dt"]) == 0 else [7.0, 3.0, 4.0, 2.0], iters)
            s.advect(0, "dens", "dens_prev", "u", "v", args["dt"])
            counts.append(s.timing_read(reset=True))
    scalar, per_member = counts
    assert scalar["jacobi_launches"] > 0
    for k in COUNTERS:
        assert per_member[k] == scalar[k], (k, scalar, per_member)


@pytest.mark.parametrize("variant", [3, 0])
def test_constant_arrays_leave_the_scalar_calls_bits(oracle, variant):
    n, iters, members = 113, 20, 3
    fields = member_fields(oracle, n, members, seed=7)
    got = []
    for arrays in (False, True):
        def val(x):
            return np.full(members, x, F32) if arrays else x
        with solver(n, members, variant=variant) as s:
            upload_all(s, fields)
            s.step(1, use_sources=True, dt=val(0.016), diff=val(0.1), visc=val(0.0025), iters=iters)
            s.step(1, dt=val(0.1), diff=val(1e-4), visc=val(0.3), iters=iters)
            s.vel_step(val(0.3), val(0.016), iters)
            s.dens_step(val(0.0), val(0.1), iters)
            s.add_source("u", "u_prev", val(0.25))
            s.diffuse(2, "v", "v_prev", val(0.75), val(4.0), iters)
            s.jacobi_sweep(0, "dens", "dens_prev", "u_prev", val(0.5), val(3.0))
            s.advect(1, "v_prev", "v", "u", "dens", val(0.05))
            got.append([{k: s.download(k, member=m) for k in NAMES} for m in range(members)])
    for m in range(members):
        for k in NAMES:
            same_bits(got[1][m][k], got[0][m][k], "member %d %s: constant arrays against the scalar calls" % (m, k))


# ---- 3. operators ---------------------------------------------------------------------------------------------------------
# member 0: the pressure form (mode 4 on its own); 1 and 3: general betas; 2: a power-of-two beta with alpha != 1
OP_ALPHA = np.array([1.0, 0.36, 0.3, 2.25], F32)
OP_BETA = np.array([4.0, 2.44, 2.0, 10.0], F32)
OP_DT = np.array([0.016, 0.1, -0.25, 0.0], F32)


@pytest.mark.parametrize("variant", [3, 0])
@pytest.mark.parametrize("iters", [0, 2, 8, 20, 40])
def test_diffuse_with_member_coefficients(oracle, iters, variant):
    n, members = 61, 4
    fields = member_fields(oracle, n, members, seed=iters, kinds=("uniform", "coarse", "parameters", "subnormal"))
    models = [Model(oracle, f) for f in fields]
    with solver(n, members, variant=variant) as s:
        upload_all(s, fields)
        for b, x, x0 in ((1, "u", "u_prev"), (0, "dens", "dens_prev"), (2, "v", "v_prev")):
            s.diffuse(b, x, x0, OP_ALPHA, OP_BETA, iters)
            for m, mod in enumerate(models):
                oracle.diffuse(b, mod.f[x], mod.f[x0], float(OP_ALPHA[m]), float(OP_BETA[m]), iters)
        compare_all(s, models, "diffuse, %d sweeps, variant %d" % (iters, variant))


@pytest.mark.parametrize("variant", [3, 0])
def test_operators_with_member_values(oracle, variant):
    n, members = 61, 4
    fields = member_fields(oracle, n, members, seed=5, kinds=("uniform", "coarse", "parameters", "subnormal"))
    models = [Model(oracle, f) for f in fields]
    with solver(n, members, variant=variant) as s:
        upload_all(s, fields)
        # a real source; then a source that is zero by definition (the divergence's p), whose increment stays pending until
        # the diffusion takes it as its right-hand side; then one that a plain reader settles
        s.add_source("u", "u_prev", OP_DT)
        s.computeDivergenceAndPressure("u", "v", "dens_prev", "v_prev")
        s.add_source("dens", "dens_prev", OP_DT)
        s.diffuse(0, "u_prev", "dens", OP_ALPHA, OP_BETA, 8)
        s.add_source("v", "dens_prev", -OP_DT)
        s.jacobi_sweep(1, "v", "u", "dens", OP_ALPHA, OP_BETA)
        s.advect(2, "v_prev", "u_prev", "u", "v", OP_DT)
        for m, mod in enumerate(models):
            f, dt, a, b = mod.f, float(OP_DT[m]), float(OP_ALPHA[m]), float(OP_BETA[m])
            oracle.add_source(f["u"], f["u_prev"], dt)
            oracle.divergence(f["u"], f["v"], f["dens_prev"], f["v_prev"])
            oracle.add_source(f["dens"], f["dens_prev"], dt)
            oracle.diffuse(0, f["u_prev"], f["dens"], a, b, 8)
            oracle.add_source(f["v"], f["dens_prev"], -dt)
            oracle.jacobi_sweep(1, f["v"], f["u"], f["dens"], a, b)
            mod.advect(2, f["v_prev"], f["u_prev"], f["u"], f["v"], dt)
        compare_all(s, models, "operators, variant %d" % variant)


# ---- 4. values that steer the host logic ------------------------------------------------------------------------------------
# dt of 0, -0 and a negative dt beside ordinary ones; visc = diff = 0; a negative beta (alpha -576, beta -2303 at N = 30)
HOST_TRIPLES = [(0.016, 0.1, 0.0025), (0.0, 0.1, 0.0025), (-0.0, 0.1, 0.0025), (-0.016, 0.1, 0.0025), (0.016, 0.0, 0.0),
                (0.016, -40.0, -40.0), (0.1, 1e-4, 0.3), (-0.0, 0.0, 0.0)]


def host_fields(oracle, n, members):
    """fields that hold -0: the coarse class (an eighth of its cells), all -0, and ordinary ones in rotation"""
    out = []
    for m in range(members):
        rng = np.random.default_rng(40 + m)
        if m % 3 == 0:
            out.append(make_fields("coarse", n, rng, oracle))
        elif m % 3 == 1:
            out.append({k: np.full((n + 2, n + 2), -0.0, F32) for k in NAMES})
        else:
            out.append(make_fields("uniform", n, rng, oracle))
    return out


@pytest.mark.parametrize("variant", [3, 0])
@pytest.mark.parametrize("fuse_add_source", [0, 1])
def test_values_that_steer_the_host_logic(oracle, fuse_add_source, variant):
    from fluidsimulationcuda_amd import capi
    n, iters, members = 30, 8, len(HOST_TRIPLES)
    a, b = oracle.coefficients(n, 0.016, -40.0)
    assert (a, b) == (-576.0, -2303.0)
    P = tuple(np.array([t[k] for t in HOST_TRIPLES], F32) for k in range(3))
    assert np.signbit(P[0][2]) and P[0][2] == 0
    sequence = (("step", False), ("step", True), ("step", False), ("vel_step",), ("dens_step",))
    params = {capi.PARAM_FUSE_ADD_SOURCE: fuse_add_source}
    for shift in (0, 1):                          # every triple meets a field class with -0 in it
        fields = host_fields(oracle, n, members + shift)[shift:]
        models = [Model(oracle, f) for f in fields]
        with solver(n, members, params=params, variant=variant) as s:
            upload_all(s, fields)
            run_members(s, models, P, iters, "shift %d" % shift, sequence=sequence)
        for mod in models:
            for k in NAMES:
                assert np.isfinite(mod.f[k]).all(), "the oracle left a non-finite %s: this case must stay finite" % k
        # ... and each member against a one-member context given its scalars
        for m in range(members):
            with solver(n, 1, params=params, variant=variant) as one:
                one.upload(**fields[m])
                dt, diff, visc = (float(P[k][m]) for k in range(3))
                for call in sequence:
                    if call[0] == "step":
                        one.step(1, use_sources=call[1], dt=dt, diff=diff, visc=visc, iters=iters)
                    elif call[0] == "vel_step":
                        one.vel_step(visc, dt, iters)
                    else:
                        one.dens_step(diff, dt, iters)
                for k in NAMES:
                    same_bits(one.download(k), models[m].f[k], "one-member context with member %d's scalars, %s" % (m, k))


# ---- 5. queued calls ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [3, 0])
def test_queued_calls_with_different_arrays(oracle, variant):
    """Twelve per-member calls in a row, no synchronise between them, each with other values, and the caller's arrays
    overwritten in place the moment a call returns.  64 members: a solve's table is 7.5 KiB, the calls' tables together
    several times the ring they are staged in, so slots are reused while earlier launches are still queued."""
    n, iters, members, calls = 14, 4, 64, 12
    fields = member_fields(oracle, n, members, seed=3, kinds=("uniform", "coarse", "parameters"))
    models = [Model(oracle, f) for f in fields]
    rng = np.random.default_rng(17)
    dt, diff, visc = (np.empty(members, F32) for _ in range(3))
    used = []
    with solver(n, members, variant=variant) as s:
        upload_all(s, fields)
        for k in range(calls):
            dt[:] = rng.choice([0.016, 0.1, 0.05, 0.0], members)
            diff[:] = rng.uniform(0.0, 0.2, members)
            visc[:] = rng.uniform(0.0, 0.3, members)
            used.append((dt.copy(), diff.copy(), visc.copy()))
            s.step(1, use_sources=(k % 3 == 0), dt=dt, diff=diff, visc=visc, iters=iters)
            for a in (dt, diff, visc):
                a[:] = np.nan                     # what a caller may do with its own memory once the call is back
        for k, P in enumerate(used):
            for m, mod in enumerate(models):
                mod.step(k % 3 == 0, float(P[0][m]), float(P[1][m]), float(P[2][m]), iters)
        compare_all(s, models, "after %d queued calls" % calls)


# ---- 6. lazy state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 8, 20])
@pytest.mark.parametrize("fuse_add_source", [0, 1])
@pytest.mark.parametrize("field", ["u_prev", "dens_prev", "u", "dens"])
def test_member_upload_against_per_member_marks(oracle, field, fuse_add_source, iters):
    """test_gpu_ensemble.test_member_upload_against_shared_marks_after_steps after per-member steps: what a field is owed is
    now a value per member (dt[m] * 0 with dt's sign, or dt[m] times a source), and the members that were not uploaded must
    end up with their own"""
    from fluidsimulationcuda_amd import capi
    n, members = 61, 3
    fields = member_fields(oracle, n, members, seed=3, kinds=("uniform", "coarse", "parameters"))
    for f in fields:
        f["dens"][::2] = -0.0                     # -0 where the pending increment's sign decides
        f["u"][:, ::3] = -0.0
    models = [Model(oracle, f) for f in fields]
    new = rnd(np.random.default_rng(2), n)
    P = (np.array([0.016, -0.016, -0.0], F32), np.array([0.1, 0.05, 0.2], F32), np.array([0.0025, 0.3, 0.01], F32))
    with solver(n, members, params={capi.PARAM_FUSE_ADD_SOURCE: fuse_add_source}) as s:
        upload_all(s, fields)
        for k, (first, then) in enumerate(((False, True), (True, True), (True, False))):
            run_members(s, models, P, iters, "", sequence=(("step", first),), compare=False)
            who = k % members
            s.upload(member=who, **{field: new})
            models[who].f[field][...] = new
            run_members(s, models, P, iters, "", sequence=(("step", then),), compare=False)
            compare_all(s, models, "round %d: %s of member %d uploaded between per-member steps" % (k, field, who))


def test_member_upload_against_per_member_operator_marks(oracle):
    """the operator API's marks: dens owing dt[m] * (+0); an upload of one member must leave the others their own increment"""
    n, members = 30, 3
    a, b = oracle.coefficients(n, 0.016, 0.1)
    dts = np.array([0.016, -0.5, -0.0], F32)
    for target in ("dens_prev", "dens"):
        fields = [{k: np.full((n + 2, n + 2), -0.0, F32) for k in NAMES} for _ in range(members)]
        for f in fields:
            f["dens_prev"][...] = 0.75              # stale memory behind the zero mark
        models = [Model(oracle, f) for f in fields]
        new = rnd(np.random.default_rng(8), n)
        with solver(n, members) as s:
            upload_all(s, fields)
            s.computeDivergenceAndPressure("u", "v", "dens_prev", "v_prev")
            s.add_source("dens", "dens_prev", dts)
            for m, mod in enumerate(models):
                oracle.divergence(mod.f["u"], mod.f["v"], mod.f["dens_prev"], mod.f["v_prev"])
                oracle.add_source(mod.f["dens"], mod.f["dens_prev"], float(dts[m]))
            s.upload(member=1, **{target: new})
            models[1].f[target][...] = new
            s.diffuse(0, "u_prev", "dens", [a, a, 1.0], [b, b, 4.0], 8)
            s.add_source("u", "dens_prev", -dts)
            for m, mod in enumerate(models):
                oracle.diffuse(0, mod.f["u_prev"], mod.f["dens"], *((a, b) if m < 2 else (1.0, 4.0)), 8)
                oracle.add_source(mod.f["u"], mod.f["dens_prev"], -float(dts[m]))
            compare_all(s, models, "upload of member 1's %s" % target)


@pytest.mark.parametrize("variant", [3, 0])
def test_scalar_and_member_calls_interleave(oracle, variant):
    """Scalar and per-member calls on the same ensemble, crossing where one kind leaves something owed and the other takes it
    over: (a) a per-member pending increment consumed by a scalar solve, and one settled by a reader and then overwritten by
    a scalar writer; (b) the mirror image -- uniform increments consumed by per-member solves -- and then a per-member step
    followed by a scalar one, so that what the per-member step left per member must not outlive the scalar step's marks.
    The fields are all -0 (dens_prev: stale memory behind the zero mark), so each increment's sign shows."""
    n, members, iters = 30, 3, 8
    a, b = oracle.coefficients(n, 0.016, 0.1)
    dts = np.array([0.016, -0.5, -0.0], F32)
    ma, mb = [a, a, 1.0], [b, b, 4.0]
    P = (dts, np.array([0.1, 0.05, 0.2], F32), np.array([0.0025, 0.3, 0.01], F32))

    def fresh():
        fields = [{k: np.full((n + 2, n + 2), -0.0, F32) for k in NAMES} for _ in range(members)]
        for f in fields:
            f["dens_prev"][...] = 0.75
        return fields, [Model(oracle, f) for f in fields]

    def operators(s, models, dt, dt5, alpha, beta):
        """dt, dt5, alpha, beta: a scalar or one value per member each"""
        s.computeDivergenceAndPressure("u", "v", "dens_prev", "v_prev")
        s.add_source("dens", "dens_prev", dt)
        s.diffuse(0, "u_prev", "dens", alpha, beta, iters)
        s.add_source("v", "dens_prev", dt)
        s.add_source("v", "u", dt5)
        s.jacobi_sweep(1, "v", "u", "dens", alpha, beta)
        for m, mod in enumerate(models):
            f = mod.f
            d, d5, al, be = (float(np.broadcast_to(np.asarray(x, F32), (members,))[m]) for x in (dt, dt5, alpha, beta))
            oracle.divergence(f["u"], f["v"], f["dens_prev"], f["v_prev"])
            oracle.add_source(f["dens"], f["dens_prev"], d)
            oracle.diffuse(0, f["u_prev"], f["dens"], al, be, iters)
            oracle.add_source(f["v"], f["dens_prev"], d)
            oracle.add_source(f["v"], f["u"], d5)
            oracle.jacobi_sweep(1, f["v"], f["u"], f["dens"], al, be)

    fields, models = fresh()
    with solver(n, members, variant=variant) as s:
        upload_all(s, fields)
        operators(s, models, dts, 0.25, a, b)
        compare_all(s, models, "(a) per-member state, scalar consumers, variant %d" % variant)
    fields, models = fresh()
    with solver(n, members, variant=variant) as s:
        upload_all(s, fields)
        operators(s, models, 0.016, dts, ma, mb)
        compare_all(s, models, "(b) uniform state, per-member consumers, variant %d" % variant)
        run_members(s, models, P, iters, "(b) then a per-member step", sequence=(("step", False),))
        s.step(1, dt=0.016, diff=0.1, visc=0.0025, iters=iters)
        for mod in models:
            mod.step(False, 0.016, 0.1, 0.0025, iters)
        compare_all(s, models, "(b) then a scalar step, variant %d" % variant)


# ---- 7. isolation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [3, 0])
def test_a_member_that_divides_by_zero_stays_alone(oracle, variant):
    """N = 32, dt = 2^-6, visc = diff = -2^-6: alpha = -0.25 and beta = 0 exactly.  That member's solves divide by zero and
    fill its fields with inf and NaN; it must equal its model (whose numpy advection defines the NaN back-trace as the
    kernels do), and every other member its own."""
    n, iters = 32, 8
    assert oracle.coefficients(n, 2.0 ** -6, -2.0 ** -6) == (-0.25, 0.0)
    for where in (0, 2, 4):
        members = 5
        P = [np.array(a, F32) for a in triples(members, where)]
        P[0][where], P[1][where], P[2][where] = 2.0 ** -6, -2.0 ** -6, -2.0 ** -6
        fields = member_fields(oracle, n, members, seed=where, kinds=("uniform", "parameters", "coarse"))
        models = [Model(oracle, f) for f in fields]
        with solver(n, members, variant=variant) as s:
            upload_all(s, fields)
            run_members(s, models, tuple(P), iters, "the dividing member is %d" % where, sequence=STEP_SEQUENCE[:3])
        assert not np.isfinite(models[where].f["u"][1:-1, 1:-1]).any(), "the member meant to divide by zero did not"
        for m, mod in enumerate(models):
            if m != where:
                assert np.isfinite(mod.f["u"]).all() and np.isfinite(mod.f["dens"]).all(), "member %d's model is not finite" % m


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_non_finite_entries_are_refused_and_change_nothing(oracle):
    from fluidsimulationcuda_amd import capi
    n, members, iters = 30, 3, 8
    L = capi.lib()
    fields = member_fields(oracle, n, members, seed=6, kinds=("uniform", "coarse", "parameters"))
    models = [Model(oracle, f) for f in fields]
    P = triples(members, 0)
    good = np.array([0.016, 0.1, 0.05], F32)

    def ptr(a):
        return a.ctypes.data_as(capi._MF)

    with solver(n, members) as s:
        upload_all(s, fields)
        run_members(s, models, P, iters, "", sequence=(("step", False),), compare=False)   # leaves marks and increments owed
        h = s._h
        for who in range(members):
            for value in (np.nan, np.inf, -np.inf):
                bad = good.copy()
                bad[who] = value
                calls = {
                    "fluid_step_members": [lambda: L.fluid_step_members(h, ptr(bad), ptr(good), ptr(good), iters, 1, 1),
                                           lambda: L.fluid_step_members(h, ptr(good), ptr(bad), ptr(good), iters, 1, 0),
                                           lambda: L.fluid_step_members(h, ptr(good), ptr(good), ptr(bad), iters, 1, 0)],
                    "fluid_vel_step_members": [lambda: L.fluid_vel_step_members(h, ptr(bad), ptr(good), iters),
                                               lambda: L.fluid_vel_step_members(h, ptr(good), ptr(bad), iters)],
                    "fluid_dens_step_members": [lambda: L.fluid_dens_step_members(h, ptr(bad), ptr(good), iters),
                                                lambda: L.fluid_dens_step_members(h, ptr(good), ptr(bad), iters)],
                    "fluid_op_add_source_members": [lambda: L.fluid_op_add_source_members(h, 0, 3, ptr(bad))],
                    "fluid_op_jacobi_sweep_members": [lambda: L.fluid_op_jacobi_sweep_members(h, 0, 0, 3, 2, ptr(bad), ptr(good)),
                                                      lambda: L.fluid_op_jacobi_sweep_members(h, 0, 0, 3, 2, ptr(good), ptr(bad))],
                    "fluid_op_diffuse_members": [lambda: L.fluid_op_diffuse_members(h, 0, 0, 3, ptr(bad), ptr(good), iters),
                                                 lambda: L.fluid_op_diffuse_members(h, 0, 0, 3, ptr(good), ptr(bad), iters)],
                    "fluid_op_advect_members": [lambda: L.fluid_op_advect_members(h, 0, 2, 5, 0, 1, ptr(bad))],
                }
                for name, forms in calls.items():
                    for call in forms:
                        assert call() == capi.E_INVALID, (name, who, value)
                        msg = L.fluid_last_error()
                        assert name.encode() in msg and ("member %d" % who).encode() in msg, (name, who, msg)
        with pytest.raises(capi.FluidError):
            s.step(1, dt=[0.016, np.nan, 0.016], iters=iters)
        # nothing was launched and nothing owed was dropped: the fields as the step left them, and the next step on top
        compare_all(s, models, "after the refused calls")
        run_members(s, models, P, iters, "a step after the refused calls", sequence=(("step", True), ("step", False)))


def test_members_call_on_a_one_member_context_is_the_scalar_call(oracle):
    n, iters = 61, 20
    f = make_fields("uniform", n, np.random.default_rng(1), oracle)
    got = []
    for seq in (False, True):
        def val(x):
            return [x] if seq else x
        with solver(n, 1) as s:
            s.upload(**f)
            s.step(1, use_sources=True, dt=val(0.1), diff=val(1e-4), visc=val(0.3), iters=iters)
            s.step(1, dt=val(0.016), diff=val(0.1), visc=val(0.0025), iters=iters)
            s.vel_step(val(0.3), val(0.016), iters)
            s.dens_step(val(0.0), val(0.1), iters)
            s.add_source("u", "u_prev", val(0.25))
            s.diffuse(2, "v", "v_prev", val(0.75), val(4.0), iters)
            s.jacobi_sweep(0, "dens", "dens_prev", "u_prev", val(0.5), val(3.0))
            s.advect(1, "v_prev", "v", "u", "dens", val(0.05))
            got.append({k: s.download(k) for k in NAMES})
    for k in NAMES:
        same_bits(got[1][k], got[0][k], "%s: sequences of one against scalars" % k)
    m = Model(oracle, f)
    m.step(True, 0.1, 1e-4, 0.3, iters)
    m.step(False, 0.016, 0.1, 0.0025, iters)
    m.vel_step(0.3, 0.016, iters)
    m.dens_step(0.0, 0.1, iters)
    oracle.add_source(m.f["u"], m.f["u_prev"], 0.25)
    oracle.diffuse(2, m.f["v"], m.f["v_prev"], 0.75, 4.0, iters)
    oracle.jacobi_sweep(0, m.f["dens"], m.f["dens_prev"], m.f["u_prev"], 0.5, 3.0)
    m.advect(1, m.f["v_prev"], m.f["v"], m.f["u"], m.f["dens"], 0.05)
    for k in NAMES:
        same_bits(got[1][k], m.f[k], "%s: sequences of one against the oracle" % k)


@pytest.mark.parametrize("jacobi", [0, 3])
def test_members_call_on_a_slab_context_is_the_scalar_call(jacobi):
    from test_gpu_slab import run_ranks, synthetic
    n, nranks, halo, iters = 126, 3, 8, 20
    fields = synthetic(n, seed=3)

    def scalar(s):
        s.step(1, use_sources=True, dt=0.1, diff=1e-4, visc=0.3, iters=iters)
        s.step(1, iters=iters)
        s.vel_step(0.3, 0.016, iters)
        s.dens_step(0.0, 0.1, iters)

    def sequences(s):
        assert s.member_count() == 1
        s.step(1, use_sources=True, dt=[0.1], diff=[1e-4], visc=[0.3], iters=iters)
        s.step(1, dt=[0.016], diff=[0.1], visc=[0.0025], iters=iters)
        s.vel_step([0.3], [0.016], iters)
        s.dens_step([0.0], [0.1], iters)

    want, fab0 = run_ranks(n, nranks, halo, fields, scalar, jacobi=jacobi)
    got, fab1 = run_ranks(n, nranks, halo, fields, sequences, jacobi=jacobi)
    for k in NAMES:
        same_bits(got[k], want[k], "%s on %d slabs" % (k, nranks))
    assert fab1.log[0] == fab0.log[0], "the per-member calls issued other exchanges than the scalar calls"


# ---- 9. fp16 storage ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 113, 254])
def test_fp16_members_equal_one_member_contexts(oracle, n):
    from fluidsimulationcuda_amd import capi
    members, iters = 3, 20
    fields = member_fields(oracle, n, members, seed=n, kinds=("parameters", "uniform", "subnormal", "large", "coarse"))
    dt, diff, visc = triples(members, n)
    want = []
    for m in range(members):
        with solver(n, 1, storage=capi.STORAGE_F16) as one:
            one.upload(**fields[m])
            snaps = []
            for call in STEP_SEQUENCE:
                if call[0] == "step":
                    one.step(1, use_sources=call[1], dt=float(dt[m]), diff=float(diff[m]), visc=float(visc[m]), iters=iters)
                elif call[0] == "vel_step":
                    one.vel_step(float(visc[m]), float(dt[m]), iters)
                else:
                    one.dens_step(float(diff[m]), float(dt[m]), iters)
                snaps.append({k: one.download(k) for k in NAMES})
            want.append(snaps)
    with solver(n, members, storage=capi.STORAGE_F16) as s:
        upload_all(s, fields)
        for k, call in enumerate(STEP_SEQUENCE):
            if call[0] == "step":
                s.step(1, use_sources=call[1], dt=dt, diff=diff, visc=visc, iters=iters)
            elif call[0] == "vel_step":
                s.vel_step(visc, dt, iters)
            else:
                s.dens_step(diff, dt, iters)
            for m in range(members):
                for name in NAMES:
                    same_bits(s.download(name, member=m), want[m][k][name], "fp16 n=%d member %d %s after call %d" % (n, m, name, k + 1))


# ---- 10. large ------------------------------------------------------------------------------------------------------------------
def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.float32).view(np.uint8).reshape(-1))


def test_large_members_equal_one_member_contexts(oracle):
    """N = 2046, three members with three distinct triples: the CRC-32 of every field per member equals that of a
    one-member context given the member's scalars"""
    from fluidsimulationcuda_amd.harness import initialize_parameters
    n, members = 2046, 3
    dens, dens0, u, u0, v, v0 = oracle.initialize_glibc(n, seed=1)
    fields = [dict(u=u, v=v, dens=dens, u_prev=u0, v_prev=v0, dens_prev=dens0), initialize_parameters(n, seed=9),
              initialize_parameters(n, seed=4)]
    dt = np.array([0.016, 0.1, 0.016], F32)
    diff = np.array([0.1, 1e-4, 0.0], F32)
    visc = np.array([0.0025, 0.3, 0.01], F32)
    want = []
    for m in range(members):
        with solver(n, 1) as one:
            one.upload(**fields[m])
            snaps = []
            for use in (True, False):
                one.step(1, use_sources=use, dt=float(dt[m]), diff=float(diff[m]), visc=float(visc[m]))
                snaps.append({k: crc(one.download(k)) for k in NAMES})
            want.append(snaps)
    with solver(n, members) as s:
        upload_all(s, fields)
        for k, use in enumerate((True, False)):
            s.step(1, use_sources=use, dt=dt, diff=diff, visc=visc)
            for m in range(members):
                for name in NAMES:
                    assert crc(s.download(name, member=m)) == want[m][k][name], "n=%d member %d %s after step %d" % (n, m, name, k + 1)


def test_table_uploads_stop_in_a_stepping_loop(oracle):
    """the steady state of a loop with the same arrays every call adds neither copies nor waits: measured here by the bits
    alone (the tables are reused), over enough steps to wrap the staging ring many times if they were not"""
    n, iters, members = 33, 4, 8
    fields = member_fields(oracle, n, members, seed=9, kinds=("uniform", "parameters"))
    models = [Model(oracle, f) for f in fields]
    P = triples(members, 4)
    with solver(n, members) as s:
        upload_all(s, fields)
        run_members(s, models, P, iters, "", sequence=(("step", True),) + (("step", False),) * 40, compare=False)
        compare_all(s, models, "41 steps with the same arrays")
