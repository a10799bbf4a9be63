"""GPU: an ensemble context (fluid_create_ensemble, FluidSolver(n, members=M)) -- M simulations of the same size going
through every call together, in the same kernel launches.

The rule everything here holds the library to: member m of an ensemble equals, bit for bit (NaN where the oracle has NaN),
the oracle run on member m's arrays through the same call sequence -- all six fields, fp32 storage.  With fp16 storage, and
at the sizes where the oracle is too slow to be asked for every member, member m equals a one-member context given the same
uploads (test_gpu_f16_steps.py / test_gpu_large.py tie that context to the model and the reference).  No tolerance
anywhere.

The members of one ensemble get different seeds and different input classes (test_gpu_f16_steps.make_fields), so that a
kernel that read another member's rows, tiles or lazy-state marks would show."""
import json
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, rnd
from test_gpu_f16_steps import make_fields
from test_gpu_lazy_state import COARSE, NAMES, Model, absmax32, check_residual, draw_fields, draw_sequence, play, same_bits
from test_gpu_random_configs import random_params

pytestmark = pytest.mark.gpu
DT, VISC, DIFF = 0.016, 0.0025, 0.1
F32 = np.float32
KINDS = ("parameters", "uniform", "coarse", "subnormal", "large", "nonfinite")
# more seeds for a one-off soak: FLUID_FUZZ_ENSEMBLE=500 FLUID_FUZZ_ENSEMBLE_SEQUENCES=500
N_RANDOM = int(os.environ.get("FLUID_FUZZ_ENSEMBLE", "32"))
N_SEQ = int(os.environ.get("FLUID_FUZZ_ENSEMBLE_SEQUENCES", "96"))


def solver(n, members, params=None, variant=3, storage=0):
    import fluidsimulationcuda_amd as F
    return F.FluidSolver(n, members=members, jacobi=variant, params=params, storage=storage)


def member_fields(oracle, n, members, seed, kinds=KINDS):
    """one set of six fields per member: different seeds, the input classes in rotation (starting at `seed`)"""
    return [make_fields(kinds[(seed + m) % len(kinds)], n, np.random.default_rng(977 * seed + m), oracle) for m in range(members)]


def upload_all(s, fields):
    for m, f in enumerate(fields):
        s.upload(member=m, **f)


def compare_all(s, models, what):
    for m, mod in enumerate(models):
        for k in NAMES:
            same_bits(s.download(k, member=m), mod.f[k], "member %d of %d, %s -- %s" % (m, len(models), k, what))


STEP_SEQUENCE = (("step", True), ("step", False), ("step", False), ("step", True), ("vel_step",), ("dens_step",))


def run_sequence(s, models, iters, what, dt=DT, diff=DIFF, visc=VISC, sequence=STEP_SEQUENCE):
    """a sourced step, two plain ones, a sourced step that consumes what the last one left in *_prev, then vel_step and
    dens_step on their own: the library once, the model per member, every member compared after each call"""
    for k, call in enumerate(sequence):
        if call[0] == "step":
            s.step(1, use_sources=call[1], dt=dt, diff=diff, visc=visc, iters=iters)
            for mod in models:
                mod.step(call[1], dt, diff, visc, iters)
        elif call[0] == "vel_step":
            s.vel_step(visc, dt, iters)
            for mod in models:
                mod.vel_step(visc, dt, iters)
        else:
            s.dens_step(diff, dt, iters)
            for mod in models:
                mod.dens_step(diff, dt, iters)
        compare_all(s, models, "%s: call %d %r" % (what, k + 1, call))


# ---- 4. steps ---------------------------------------------------------------------------------------------------------
# N: the fused kernel's window widths and the smallest grids; iters 0 / 2 / 6 / 10 / 14 / 40 and M 2 / 3 / 5 / 16 spread
# over them (the oracle's cost grows with N^2 x M)
STEP_CASES = [(1, 40, 16), (2, 14, 5), (3, 10, 3), (5, 6, 2), (14, 2, 16), (61, 0, 5), (112, 40, 3), (113, 14, 2),
              (127, 10, 16), (128, 6, 5), (129, 2, 3), (241, 40, 2), (254, 14, 16), (510, 10, 5), (1022, 40, 2),
              (61, 40, 16), (254, 0, 3), (1022, 6, 3), (14, 40, 5), (129, 40, 16)]


@pytest.mark.parametrize("n, iters, members", STEP_CASES)
def test_steps_match_oracle_per_member(oracle, n, iters, members):
    fields = member_fields(oracle, n, members, seed=n + iters)
    models = [Model(oracle, f) for f in fields]
    with solver(n, members) as s:
        assert s.member_count() == members
        upload_all(s, fields)
        run_sequence(s, models, iters, "n=%d iters=%d M=%d" % (n, iters, members))


# ---- 5. every operator of the header, and fluid_fill ---------------------------------------------------------------------
class NoLibrary:
    """play() with this as the solver applies an operator to the model alone"""

    def __init__(self, n):
        self.n = n

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: None


def play_ensemble(s, models, op, what):
    """one library call on the ensemble, the same operator on every member's model; the two reductions return the maximum
    over the members"""
    got = play(s, None, op, what)
    if op[0] not in ("absmax", "residual"):
        for mod in models:
            play(NoLibrary(mod.n), mod, op, what)
    if op[0] == "absmax":
        want = F32(np.fmax.reduce([absmax32(mod.f[op[1]], mod.f[op[2]]) for mod in models]))
        assert F32(got) == want, "%s: %r: %r, the members' maximum %r" % (what, op, got, want)
    if op[0] == "residual":
        x, x0, alpha, beta = op[1:]

        def res64(mod):
            a, b = mod.f[x].astype(np.float64), mod.f[x0].astype(np.float64)
            with np.errstate(all="ignore"):
                nb = a[1:-1, :-2] + a[1:-1, 2:] + a[:-2, 1:-1] + a[2:, 1:-1]
                r = np.abs(beta * a[1:-1, 1:-1] - alpha * nb - b[1:-1, 1:-1])
            r = r[~np.isnan(r)]
            return float(r.max()) if r.size else 0.0

        top = max(models, key=res64)                 # what check_residual accepts for the member with the largest one
        check_residual(got, top.f[x], top.f[x0], alpha, beta, "%s: %r" % (what, op))
    return got


OPERATOR_N = 61


def operator_cases(a1=0.0, b1=1.0):
    """a1, b1: the viscosity's coefficients at OPERATOR_N (the defaults serve the collection of the names alone)"""
    n = OPERATOR_N
    ops = {"set_bnd.%d" % b: [("set_bnd", b, "u")] for b in (0, 1, 2)}
    ops["add_source"] = [("add_source", "u", "u_prev", DT)]
    ops["add_source.zero_source"] = [("divergence", "u", "v", "dens_prev", "v_prev"), ("add_source", "dens", "dens_prev", DT),
                                     ("diffuse", 0, "u_prev", "dens", a1, b1, 8)]
    for b in (0, 1, 2):
        ops["jacobi_sweep.%d" % b] = [("jacobi", b, "u", "u_prev", "dens", a1, b1)]
        ops["diffuse.general.%d" % b] = [("diffuse", b, "u", "u_prev", a1, b1, 20)]
        ops["diffuse.pressure.%d" % b] = [("diffuse", b, "v", "v_prev", 1.0, 4.0, 20)]
    ops["diffuse.zero_iters"] = [("diffuse", 1, "u", "u_prev", a1, b1, 0)]
    for b in (0, 1, 2):
        ops["advect.%d" % b] = [("advect", b, "dens", "dens_prev", "u", "v", DT)]
    ops["advect.self"] = [("advect", 1, "u_prev", "u", "u", "v", DT)]
    ops["divergence"] = [("divergence", "u", "v", "u_prev", "v_prev")]
    ops["subtract_gradient"] = [("gradient", "u", "v", "dens")]
    ops["projection"] = [("divergence", "u", "v", "u_prev", "v_prev"), ("diffuse", 0, "u_prev", "v_prev", 1.0, 4.0, 20),
                         ("gradient", "u", "v", "u_prev")]
    ops["fill.zero"] = [("fill", "dens", 0.0), ("add_source", "u", "dens", DT)]
    ops["fill.minus_zero"] = [("fill", "dens", -0.0)]
    ops["fill.value"] = [("fill", "v_prev", 0.5), ("add_source", "v", "v_prev", DT)]
    ops["residual"] = [("residual", "u", "u_prev", a1, b1)]
    ops["absmax"] = [("absmax", "u", "v")]
    return n, ops


OPERATOR_NAMES = sorted(operator_cases()[1])


@pytest.mark.parametrize("variant", [3, 0])
@pytest.mark.parametrize("name", OPERATOR_NAMES)
def test_operator_on_an_ensemble(oracle, name, variant):
    n, cases = operator_cases(*oracle.coefficients(OPERATOR_N, DT, VISC))
    kinds = ("uniform", "coarse", "parameters", "subnormal")
    fields = member_fields(oracle, n, 4, seed=OPERATOR_NAMES.index(name), kinds=kinds)
    models = [Model(oracle, f) for f in fields]
    with solver(n, 4, variant=variant) as s:
        upload_all(s, fields)
        for op in cases[name]:
            play_ensemble(s, models, op, name)
        compare_all(s, models, "%s variant %d" % (name, variant))


# ---- 6. knobs, one at a time, on an ensemble of 3 ------------------------------------------------------------------------
def knob_cases():
    from fluidsimulationcuda_amd import capi
    out = [("variant", v, {}) for v in (0, 1, 2, 3)]
    out += [("max_sweeps", 3, {capi.PARAM_TB_MAX_SWEEPS: t, capi.PARAM_TB_T16_MIN_CELLS: 0}) for t in (16, 12, 8, 4, 2)]
    out += [("lane_columns", 3, {capi.PARAM_TB_LANE_COLUMNS: v}) for v in (2, 4)]
    out += [("fast_division", 3, {capi.PARAM_TB_FAST_DIVISION: v}) for v in (0, 1, 2, 3)]
    out += [("rows", 3, {capi.PARAM_TB_ROWS: v}) for v in (0, 1, 5, 17, 1000)]
    out += [("edge_rows_pct", 3, {capi.PARAM_TB_EDGE_ROWS_PCT: v}) for v in (0, 40, 100)]
    out += [("autotune", 3, {capi.PARAM_TB_AUTOTUNE: v}) for v in (0, 1)]
    out += [("fill", 3, {capi.PARAM_TB_FILL: v}) for v in (0, 1)]
    out += [("fuse_divergence", 3, {capi.PARAM_FUSE_DIVERGENCE: v}) for v in (0, 1)]
    out += [("fuse_add_source", 3, {capi.PARAM_FUSE_ADD_SOURCE: v}) for v in (0, 1)]
    out += [("min_cells", 3, {capi.PARAM_TB_MIN_CELLS: v}) for v in (0, 1 << 30)]
    return out


KNOBS = knob_cases()


@pytest.mark.parametrize("case", range(len(KNOBS)), ids=["%s-%s" % (k[0], "-".join(str(v) for v in k[2].values()) or k[1]) for k in KNOBS])
def test_knob_on_an_ensemble(oracle, case):
    """n = 129: two windows of the 2-column lanes, one of the 4-column ones; 40 sweeps: 16 + 12 + 12 where allowed"""
    name, variant, params = KNOBS[case]
    n, iters, members = 129, 40, 3
    fields = member_fields(oracle, n, members, seed=case)
    models = [Model(oracle, f) for f in fields]
    with solver(n, members, params=params, variant=variant) as s:
        upload_all(s, fields)
        run_sequence(s, models, iters, "%s %r" % (name, params), sequence=STEP_SEQUENCE[:2] + STEP_SEQUENCE[3:4])


def test_division_mode_3_tiles_are_per_member(oracle):
    """TB_FAST_DIVISION = 1 gives the viscosity's beta the two-term reciprocal wherever |x0| >= beta * 2^-72 on every tile
    a wave touches.  Member 0's right-hand side is everywhere >= 1 (its waves take the two-term path), member 1's holds
    exact zeros and values below the threshold, where that path is an ulp off, member 2's is tiny throughout: a wave
    that took the path on another member's minima would show in member 1 or 2."""
    from fluidsimulationcuda_amd import capi
    n, iters = 254, 16
    a, b = oracle.coefficients(n, DT, VISC)
    rng = np.random.default_rng(5)
    x0 = [rnd(rng, n, 1.0, 2.0), rnd(rng, n), (rnd(rng, n) * F32(2.0 ** -120)).astype(F32)]
    x0[0][rng.random(x0[0].shape) < 0.5] *= F32(-1)
    x0[1][rng.random(x0[1].shape) < 0.3] = 0.0
    x0[1][rng.random(x0[1].shape) < 0.3] *= F32(2.0 ** -110)
    x = [rnd(rng, n) for _ in range(3)]
    x[2] = (x[2] * F32(2.0 ** -118)).astype(F32)
    for order in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        with solver(n, 3, params={capi.PARAM_TB_FAST_DIVISION: 1, capi.PARAM_TB_T16_MIN_CELLS: 0}) as s:
            assert s.division_mode(a, b) == 3, "the two-term division was not proven for beta = %r" % b
            for m, k in enumerate(order):
                s.upload(member=m, u=x[k], u_prev=x0[k])
            s.diffuse(1, "u", "u_prev", a, b, iters)
            for m, k in enumerate(order):
                want = x[k].copy()
                oracle.diffuse(1, want, x0[k], a, b, iters)
                same_bits(s.download("u", member=m), want, "member %d (right-hand side %d)" % (m, k))


# ---- 7. isolation ------------------------------------------------------------------------------------------------------
def test_members_do_not_leak_into_each_other(oracle):
    """one member all NaN, one with +-inf islands and values beyond 2^104 (the scaled-residual division's second pass, which
    is decided per wave), one all zeros of both signs, one ordinary: three steps, each member its own oracle's bits"""
    n, iters = 129, 20
    rng = np.random.default_rng(11)
    shape = (n + 2, n + 2)
    nan = {k: np.full(shape, np.nan, F32) for k in NAMES}
    wild = {k: rnd(rng, n) for k in NAMES}
    for k in NAMES:
        i, j = int(rng.integers(0, n)), int(rng.integers(0, n))
        wild[k][i:i + 3, j:j + 3] = F32(rng.choice([np.inf, -np.inf]))
        i, j = int(rng.integers(0, n - 8)), int(rng.integers(0, n - 8))
        wild[k][i:i + 8, j:j + 8] = (rnd(rng, n)[:8, :8] * F32(2.0 ** 110)).astype(F32)
    zeros = {k: np.where(rng.random(shape) < 0.5, F32(-0.0), F32(0.0)).astype(F32) for k in NAMES}
    plain = make_fields("parameters", n, rng, oracle)
    for order in ((0, 1, 2, 3), (3, 2, 1, 0)):
        fields = [dict((k, v.copy()) for k, v in (nan, wild, zeros, plain)[q].items()) for q in order]
        models = [Model(oracle, f) for f in fields]
        with solver(n, 4) as s:
            upload_all(s, fields)
            run_sequence(s, models, iters, "order %r" % (order,), sequence=STEP_SEQUENCE[:3])


# ---- 8. shared lazy state against a member upload -------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 8, 20])
@pytest.mark.parametrize("fuse_add_source", [0, 1])
@pytest.mark.parametrize("field", ["u_prev", "dens_prev", "u", "dens"])
def test_member_upload_against_shared_marks_after_steps(oracle, field, fuse_add_source, iters):
    """The lazy marks (zero by definition, an increment owed, a source owed) are one record per field for all members.
    After a plain step and after a sourced one, ONE member's copy of a field is uploaded and the next call runs: the
    members that were not uploaded must have kept what the marks stood for."""
    from fluidsimulationcuda_amd import capi
    n, members = 61, 3
    fields = member_fields(oracle, n, members, seed=3, kinds=("uniform", "coarse", "parameters"))
    models = [Model(oracle, f) for f in fields]
    new = rnd(np.random.default_rng(2), n)
    with solver(n, members, params={capi.PARAM_FUSE_ADD_SOURCE: fuse_add_source}) as s:
        upload_all(s, fields)
        for k, (first, then) in enumerate(((False, True), (True, True), (True, False))):
            s.step(1, use_sources=first, iters=iters)
            for mod in models:
                mod.step(first, DT, DIFF, VISC, iters)
            who = k % members
            s.upload(member=who, **{field: new})
            models[who].f[field][...] = new
            s.step(1, use_sources=then, iters=iters)
            for mod in models:
                mod.step(then, DT, DIFF, VISC, iters)
            compare_all(s, models, "round %d: %s of member %d uploaded between steps" % (k, field, who))


def test_member_upload_against_operator_marks(oracle):
    """the operator API's marks: dens_prev zero by definition (divergence's p), dens owing dt * (+0); a member upload of
    either must leave the other members with zeros / the increment in memory"""
    n, members = 30, 3
    a, b = oracle.coefficients(n, DT, DIFF)
    for target in ("dens_prev", "dens"):
        fields = [{k: np.full((n + 2, n + 2), -0.0, F32) for k in NAMES} for _ in range(members)]
        for f in fields:
            f["dens_prev"][...] = 0.75              # stale memory behind the zero mark
        models = [Model(oracle, f) for f in fields]
        new = rnd(np.random.default_rng(8), n)
        with solver(n, members) as s:
            upload_all(s, fields)
            for op in (("divergence", "u", "v", "dens_prev", "v_prev"), ("add_source", "dens", "dens_prev", DT)):
                play_ensemble(s, models, op, target)
            s.upload(member=1, **{target: new})
            models[1].f[target][...] = new
            for op in (("diffuse", 0, "u_prev", "dens", a, b, 8), ("add_source", "u", "dens_prev", 0.5)):
                play_ensemble(s, models, op, target)
            compare_all(s, models, "upload of member 1's %s" % target)


def test_member_upload_against_scaled_fields_fp16():
    """fp16 storage: a step leaves u_prev / v_prev multiplied by a power of two (one factor for all members).  One member's
    u_prev is uploaded, then a sourced step reads all of them: each member equals a one-member fp16 context that was given
    the same calls (and, for that member alone, the same upload)"""
    from fluidsimulationcuda_amd import capi
    from oracle.oracle import Oracle
    n, members, iters = 113, 3, 20
    fields = member_fields(Oracle(), n, members, seed=1, kinds=("parameters", "uniform", "parameters"))
    new = rnd(np.random.default_rng(4), n)

    def calls(s, upload):
        s.step(1, use_sources=True, iters=iters)
        s.step(1, iters=iters)
        upload(s)
        s.step(1, use_sources=True, iters=iters)

    with solver(n, members, storage=capi.STORAGE_F16) as s:
        upload_all(s, fields)
        calls(s, lambda s: s.upload(member=1, u_prev=new))
        got = [{k: s.download(k, member=m) for k in NAMES} for m in range(members)]
    for m in range(members):
        with solver(n, 1, storage=capi.STORAGE_F16) as one:
            one.upload(**fields[m])
            calls(one, (lambda s: s.upload(u_prev=new)) if m == 1 else (lambda s: None))
            for k in NAMES:
                same_bits(got[m][k], one.download(k), "member %d, %s" % (m, k))


# ---- 9. refusals and bookkeeping on a live context ------------------------------------------------------------------------
def test_refusals_on_a_live_ensemble(oracle):
    import ctypes as C
    from fluidsimulationcuda_amd import capi
    n, members = 30, 3
    L = capi.lib()
    host = np.zeros((n + 2, n + 2), F32)
    with solver(n, members) as s:
        h = s._h
        m = C.c_int()
        assert L.fluid_members(h, C.byref(m)) == capi.OK and m.value == members
        assert L.fluid_members(h, None) == capi.E_INVALID
        it, res = C.c_int(), C.c_float()
        ll = C.c_longlong()
        ids = (C.c_int * 1)(0)
        refused = {
            "fluid_upload": lambda: L.fluid_upload(h, 0, host),
            "fluid_download": lambda: L.fluid_download(h, 0, host),
            "fluid_upload_rows": lambda: L.fluid_upload_rows(h, 0, host, 1, 3),
            "fluid_download_rows": lambda: L.fluid_download_rows(h, 0, host, 1, 3),
            "fluid_op_diffuse_tol": lambda: L.fluid_op_diffuse_tol(h, 0, 0, 1, 1.0, 4.0, 0.0, 8, 4, C.byref(it), C.byref(res)),
            "fluid_set_exchange": lambda: L.fluid_set_exchange(h, C.cast(None, capi.EXCHANGE_FN), None),
            "fluid_exchange_now": lambda: L.fluid_exchange_now(h, capi.XCHG_HALO, ids, 1, 1),
            "fluid_exchange_rccl_attach": lambda: L.fluid_exchange_rccl_attach(h, C.create_string_buffer(128), 128),
            "fluid_exchange_rccl_attach_comm": lambda: L.fluid_exchange_rccl_attach_comm(h, C.c_void_p(8)),
            "fluid_exchange_rccl_detach": lambda: L.fluid_exchange_rccl_detach(h),
            "fluid_exchange_rccl_calls": lambda: L.fluid_exchange_rccl_calls(h, C.byref(ll), C.byref(ll), C.byref(ll)),
        }
        for name, call in refused.items():
            assert call() == capi.E_INVALID, name
            msg = L.fluid_last_error()
            assert name.encode() in msg and (b"member" in msg or b"ensemble" in msg), (name, msg)
        for name in ("fluid_upload", "fluid_download", "fluid_upload_rows", "fluid_download_rows"):
            assert refused[name]() == capi.E_INVALID and b"fluid_upload_member" in L.fluid_last_error()
        for bad in (-1, members, members + 7):
            assert L.fluid_upload_member(h, bad, 0, host) == capi.E_INVALID and b"member" in L.fluid_last_error()
            assert L.fluid_download_member(h, bad, 0, host) == capi.E_INVALID
        assert L.fluid_upload_member(h, 0, 12, host) == capi.E_INVALID
        with pytest.raises(capi.FluidError):
            s.upload(u=host)
        with pytest.raises(capi.FluidError):
            s.download("u")
    # the one-member context keeps the whole-field calls, and the member calls work on it as member 0
    f = make_fields("uniform", n, np.random.default_rng(1), oracle)
    with solver(n, 1) as s:
        s.upload(**f)
        same_bits(s.download("u", member=0), f["u"], "member 0 of a one-member context")
        s.upload(member=0, v=f["dens"])
        same_bits(s.download("v"), f["dens"], "uploaded as member 0")
        assert s.member_count() == 1


@pytest.mark.parametrize("variant", [3, 0])
def test_timing_counts_per_member(oracle, variant):
    n, iters = 61, 20
    counts = {}
    for members in (1, 4):
        fields = member_fields(oracle, n, members, seed=2, kinds=("parameters", "uniform"))
        with solver(n, members, variant=variant) as s:
            upload_all(s, fields)
            s.timing_enable(True)
            s.timing_read(reset=True)
            s.step(1, use_sources=True, iters=iters)
            s.step(1, iters=iters)
            s.diffuse(0, "dens", "dens_prev", 1.0, 4.0, iters)
            counts[members] = s.timing_read(reset=True)
    one, four = counts[1], counts[4]
    assert one["jacobi_launches"] > 0 and four["jacobi_launches"] == one["jacobi_launches"], (one, four)
    for k in ("jacobi_field_launches", "sweeps", "pressure_sweeps"):
        assert four[k] == 4 * one[k] and one[k] > 0, (k, one, four)
    for k in ("solves", "source_calls", "advection_calls", "projection_calls", "divergence_calls"):
        assert four[k] == one[k], (k, one, four)


def test_reductions_are_the_maximum_over_members(oracle):
    n, members = 61, 5
    a, b = oracle.coefficients(n, DT, VISC)
    for top in range(members):
        fields = member_fields(oracle, n, members, seed=4, kinds=("uniform", "coarse"))
        for k in ("u", "v", "u_prev"):
            fields[top][k] = (fields[top][k] * F32(8 + top)).astype(F32)
        models = [Model(oracle, f) for f in fields]
        with solver(n, members) as s:
            upload_all(s, fields)
            got = play_ensemble(s, models, ("absmax", "u", "v"), "member %d largest" % top)
            assert F32(got) == absmax32(fields[top]["u"], fields[top]["v"])
            play_ensemble(s, models, ("residual", "u", "u_prev", a, b), "member %d largest" % top)


# ---- 10. against one-member contexts: fp16 storage, and fp32 at the sizes the oracle is too slow for ------------------------
def one_member_runs(n, fields, storage, iters, sequence):
    out = []
    for f in fields:
        with solver(n, 1, storage=storage) as one:
            one.upload(**f)
            snaps = []
            for call in sequence:
                if call[0] == "step":
                    one.step(1, use_sources=call[1], iters=iters)
                elif call[0] == "vel_step":
                    one.vel_step(VISC, DT, iters)
                else:
                    one.dens_step(DIFF, DT, iters)
                snaps.append({k: one.download(k) for k in NAMES})
            out.append(snaps)
    return out


@pytest.mark.parametrize("n", [33, 113, 254])
def test_fp16_ensemble_equals_one_member_contexts(oracle, n):
    from fluidsimulationcuda_amd import capi
    members, iters = 3, 20
    fields = member_fields(oracle, n, members, seed=n, kinds=("parameters", "uniform", "subnormal", "large", "coarse"))
    want = one_member_runs(n, fields, capi.STORAGE_F16, iters, STEP_SEQUENCE)
    with solver(n, members, storage=capi.STORAGE_F16) as s:
        upload_all(s, fields)
        for k, call in enumerate(STEP_SEQUENCE):
            if call[0] == "step":
                s.step(1, use_sources=call[1], iters=iters)
            elif call[0] == "vel_step":
                s.vel_step(VISC, DT, iters)
            else:
                s.dens_step(DIFF, DT, iters)
            for m in range(members):
                for name in NAMES:
                    same_bits(s.download(name, member=m), want[m][k][name], "fp16 n=%d member %d %s after call %d" % (n, m, name, k + 1))


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.float32).view(np.uint8).reshape(-1))


@pytest.mark.parametrize("n", [2046, 4094])
def test_large_ensemble_equals_one_member_contexts(oracle, n):
    """M = 2 at the sizes whose default schedule has the 12- and 16-sweep launches; at 4094 member 0 starts from the
    reference's own initial state and must also give the CRC-32 the compiled reference left (tests/golden/checksums.json)"""
    from fluidsimulationcuda_amd.harness import initialize_parameters
    dens, dens0, u, u0, v, v0 = oracle.initialize_glibc(n, seed=1)
    fields = [dict(u=u, v=v, dens=dens, u_prev=u0, v_prev=v0, dens_prev=dens0), initialize_parameters(n, seed=9)]
    sequence = STEP_SEQUENCE[:2]
    want = one_member_runs(n, fields, 0, 40, sequence)
    with solver(n, 2) as s:
        upload_all(s, fields)
        s.step(1, use_sources=True)
        first = [{k: s.download(k, member=m) for k in NAMES} for m in range(2)]
        s.step(1)
        second = [{k: s.download(k, member=m) for k in NAMES} for m in range(2)]
    for m in range(2):
        for k in NAMES:
            same_bits(first[m][k], want[m][0][k], "n=%d member %d %s after the sourced step" % (n, m, k))
            same_bits(second[m][k], want[m][1][k], "n=%d member %d %s after the plain step" % (n, m, k))
    rows = [r for r in json.load(open(os.path.join(GOLDEN, "checksums.json"))) if r["n"] == n]
    if n == 4094:
        assert rows, "tests/golden/checksums.json has no row for N = 4094"
    for row in rows:
        assert (crc(first[0]["u"]), crc(first[0]["v"]), crc(first[0]["dens"])) == (row["crc_u"], row["crc_v"], row["crc_dens"])


# ---- 11. seeded random configurations and operator sequences ---------------------------------------------------------------
@pytest.mark.parametrize("seed", range(N_RANDOM))
def test_random_ensemble_configuration_matches_oracle(oracle, seed):
    from fluidsimulationcuda_amd import capi
    rng = np.random.default_rng(9000 + seed)
    n = int(rng.choice([1, 2, 3, 5, 8, 13, 31, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 200, 255, 256, 257, 333]))
    iters = int(rng.choice([0, 2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 44]))
    members = int(rng.integers(1, 7))
    variant = int(rng.choice([3, 3, 3, 3, 0, 1, 2]))
    params = random_params(rng, capi)
    kinds = [KINDS[rng.integers(len(KINDS))] for _ in range(members)]
    fields = [make_fields(k, n, rng, oracle) for k in kinds]
    dt, diff, visc = float(rng.choice([0.016, 0.1])), float(rng.choice([0.1, 0.0, 1e-4])), float(rng.choice([0.0025, 0.0, 0.3]))
    what = "seed %d: n=%d iters=%d M=%d variant=%d %r %r" % (seed, n, iters, members, variant, kinds, params)
    models = [Model(oracle, f) for f in fields]
    with solver(n, members, params=params, variant=variant) as s:
        upload_all(s, fields)
        run_sequence(s, models, iters, what, dt=dt, diff=diff, visc=visc, sequence=STEP_SEQUENCE[:2])


def ensemble_ops(rng, ops, n, members):
    """test_gpu_lazy_state's sequences for an ensemble: the whole-field and row copies (refused there) become copies of
    one member, the residual-terminated solve (refused) a fixed one"""
    out = []
    for op in ops:
        if op[0] == "upload_rows":
            out.append(("upload_member", int(rng.integers(members)), op[1], op[4]))
        elif op[0] in ("download", "download_rows"):
            out.append(("download_member", int(rng.integers(members)), op[1]))
        elif op[0] == "diffuse_tol":
            out.append(("diffuse",) + tuple(op[1:6]) + (int(op[7]),))
        else:
            out.append(op)
        if rng.random() < 0.15:
            out.append(("upload_member", int(rng.integers(members)), NAMES[rng.integers(6)], float(rng.choice([-0.0, 0.25]))))
    return out


@pytest.mark.parametrize("seed", range(N_SEQ))
def test_random_operator_sequence_on_an_ensemble(oracle, seed):
    from fluidsimulationcuda_amd import capi
    rng = np.random.default_rng(12000 + seed)
    n = int(rng.choice([1, 2, 3, 5, 8, 13, 31, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 200, 255, 256, 257]))
    members = 3
    params = {capi.PARAM_TB_T16_MIN_CELLS: int(rng.choice([0, -1]))}
    fields = [draw_fields(rng, n) for _ in range(members)]
    ops = ensemble_ops(rng, draw_sequence(rng, oracle, n), n, members)
    what = "seed %d n=%d %r: %r" % (seed, n, params, ops)
    models = [Model(oracle, f) for f in fields]
    with solver(n, members, params=params) as s:
        upload_all(s, fields)
        for op in ops:
            if op[0] == "upload_member":
                _, m, name, value = op
                host = rng.choice(COARSE, size=(n + 2, n + 2)).astype(F32) if value else np.full((n + 2, n + 2), value, F32)
                s.upload(member=m, **{name: host})
                models[m].f[name][...] = host
            elif op[0] == "download_member":
                _, m, name = op
                same_bits(s.download(name, member=m), models[m].f[name], "%r -- %s" % (op, what))
            else:
                play_ensemble(s, models, op, what)
        compare_all(s, models, what)
