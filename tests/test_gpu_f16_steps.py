"""fp16 storage (FLUID_STORAGE_F16) pinned bit for bit above the operator level: whole steps against a model of the mode.

test_gpu_f16.py defines what the mode computes -- the oracle's fp32 arithmetic on fp16-widened inputs, one round to
nearest per store, once per fused launch -- and pins it for single operators and solves.  One rule was added since:
inside a step the divergence and the pressure of a projection are kept multiplied by S = 2^(floor(log2 N) - 2) (N >= 16,
FLUID_PARAM_F16_PRESSURE_SCALE on).  F16Model composes whole steps from those two statements and the oracle's operators,
as test_gpu_lazy_state.Model does for fp32:

- Every store is rounded once, h(x) = float32(float16(x)): add_source h(x + dt*s), each launch of a solve (each sweep
  of a single-sweep kernel), the divergence, the gradient subtraction, each advection.  The fused paths -- the add_source
  and the divergence inside a solve's first launch, the density advection inside the gradient subtraction -- hand on the
  rounded value, so the model has no fusion knob.
- A solve's launch depths are fluid_plan_sweeps' for fp16 storage (the greedy 8 / 4 / 2), or one sweep per launch
  (Jacobi variants 0-2, grids under FLUID_PARAM_TB_MIN_CELLS).  The library's jacobi_field_launches is asserted against
  the model's count, so that a schedule drift fails as one.
- The divergence is stored as h(S * div); the pressure solve runs and rounds on the scaled values; the gradient divides
  back exactly.  A download divides on the host (exact); any other reader of a scaled field -- the add_source of a sourced
  step after a step -- first multiplies it back in place, which rounds again: h(p_s / S).

The header calls every other knob "speed only in both storage types": each of them, at each of its values, must give the
model's bits.  Slabs are not repeated here: the fp16 slab tests require them to equal one context.
"""
import os

import numpy as np
import pytest

from conftest import assert_bit_equal, rnd
from test_gpu_f16 import emu_solve, h, launches
from test_gpu_lazy_state import COARSE, NAMES, Model, same_bits

gpu = pytest.mark.gpu
DT, VISC, DIFF = 0.016, 0.0025, 0.1
F32 = np.float32
# more seeds for a one-off soak: FLUID_FUZZ_F16=2000 python -m pytest tests/test_gpu_f16_steps.py -k random
N_FUZZ = int(os.environ.get("FLUID_FUZZ_F16", "48"))
# the scale's boundaries (16, 32), the fused kernel's window widths (owned columns per window: 2-column lanes 112 / 120 /
# 124 at depth 8 / 4 / 2, 4-column lanes 240 / 248; test_gpu_ops.TB_SIZES) and strip edges
SIZES = [1, 2, 3, 5, 14, 15, 16, 17, 31, 32, 33, 61, 96, 97, 112, 113, 127, 128, 129, 240, 241, 254, 257, 510, 1022]
ITERS = [0, 2, 6, 10, 14, 40]
INPUTS = ["parameters", "portable", "uniform", "coarse", "subnormal", "large", "nonfinite"]


def identity(a):
    return np.array(a, np.float32, copy=True)


def pressure_scale(n, knob=1):
    """the factor of a step's divergence and pressure: 2^(floor(log2 N) - 2) from N = 16 on, with the knob on; else 1"""
    return F32(2.0 ** (int(n).bit_length() - 3)) if knob and n >= 16 else F32(1.0)


def plan_sweeps(n, iters, max_t=16, pressure=False):
    """fluid_plan_sweeps for fp16 storage on the whole grid (host logic: no device)"""
    import ctypes as C
    from fluidsimulationcuda_amd import capi
    buf, cnt = (C.c_int * 64)(), C.c_int()
    capi.check(capi.lib().fluid_plan_sweeps(n, n, capi.STORAGE_F16, int(pressure), iters, max_t, -1, buf, 64, C.byref(cnt)))
    assert cnt.value <= 64
    return list(buf[:cnt.value])


def schedule(n, iters, pressure=False, variant=3, max_t=16, min_cells=0):
    """one solve's launch depths: the fused kernel's plan, or one sweep per launch (variants 0-2, grids under TB_MIN_CELLS)"""
    if variant != 3 or n * n < min_cells:
        return [1] * iters
    return plan_sweeps(n, iters, max_t, pressure)


class F16Model(Model):
    """The six fields as an fp16 context holds them: each store goes through `store` (h; the identity gives the fp32
    steps), and `scaled` names the fields kept multiplied by S.  plan(iters, pressure) -> a solve's launch depths;
    field_launches counts them as the library's timing does (once per field)."""

    def __init__(self, oracle, fields, scale, plan, store=h):
        super().__init__(oracle, {k: store(fields[k]) for k in NAMES})
        self.S, self.plan, self.store = F32(scale), plan, store
        self.scaled = set()
        self.field_launches = 0

    def wrote(self, k, value):
        self.f[k] = self.store(value)
        self.scaled.discard(k)

    def unscale(self, *ks):
        """a reader that does not know the scale: the field is multiplied back in place, and stored again"""
        for k in ks:
            if k in self.scaled:
                self.wrote(k, self.f[k] / self.S)

    def download(self, k):
        """what fluid_download returns: a scaled field divided on the host, exactly"""
        return self.f[k] / self.S if k in self.scaled else self.f[k].copy()

    def add_source(self, x, s, dt):
        self.unscale(x, s)
        out = self.f[x].copy()
        self.o.add_source(out, self.f[s], dt)
        self.wrote(x, out)

    def solve(self, b, x, x0, alpha, beta, it, pressure=False):
        chunks = self.plan(it, pressure)
        assert sum(chunks) == it, (it, chunks)
        self.field_launches += len(chunks)
        self.f[x] = emu_solve(self.o, b, self.f[x], self.f[x0], alpha, beta, chunks, store=self.store)

    def advect_into(self, b, d, d0, u, v, dt):
        self.unscale(d0, u, v)
        out = np.zeros_like(self.f[d])
        self.advect(b, out, self.f[d0], self.f[u], self.f[v], dt)
        self.wrote(d, out)

    def project(self, it, u, v, p, div):
        """divergence h(S * div), p = 0; the solve on the scaled values; the gradient of p_s / S (exact)"""
        f, S = self.f, self.S
        self.unscale(u, v)
        p0, d = np.empty_like(f[p]), np.empty_like(f[div])
        self.o.divergence(f[u], f[v], p0, d)
        self.wrote(div, d * S)
        self.wrote(p, p0)
        self.solve(0, p, div, 1.0, 4.0, it, pressure=True)
        uu, vv = f[u].copy(), f[v].copy()
        self.o.subtract_gradient(uu, vv, f[p] / S)
        self.wrote(u, uu)
        self.wrote(v, vv)
        self.scaled |= {p, div}

    # fluid_solver.hip: vel_step / dens_step (full_step runs the density's add_source and diffusion beside the velocity's:
    # the same arithmetic per field)
    def vel_step(self, visc, dt, it):
        self.add_source("u", "u_prev", dt)
        self.add_source("v", "v_prev", dt)
        a, b = self.o.coefficients(self.n, dt, visc)
        self.solve(1, "u_prev", "u", a, b, it)
        self.solve(2, "v_prev", "v", a, b, it)
        self.project(it, "u_prev", "v_prev", "u", "v")
        self.advect_into(1, "u", "u_prev", "u_prev", "v_prev", dt)
        self.advect_into(2, "v", "v_prev", "u_prev", "v_prev", dt)
        self.project(it, "u", "v", "u_prev", "v_prev")

    def dens_step(self, diff, dt, it):
        self.add_source("dens", "dens_prev", dt)
        a, b = self.o.coefficients(self.n, dt, diff)
        self.solve(0, "dens_prev", "dens", a, b, it)
        self.advect_into(0, "dens", "dens_prev", "u", "v", dt)

    def step(self, use_sources, dt, diff, visc, it):
        if not use_sources:
            for k in ("u_prev", "v_prev", "dens_prev"):
                self.wrote(k, np.zeros_like(self.f[k]))
        self.vel_step(visc, dt, it)
        self.dens_step(diff, dt, it)


def model_of(oracle, n, fields, params=None, variant=3):
    """the model of an fp16 context made with these parameters"""
    from fluidsimulationcuda_amd import capi
    p = params or {}
    max_t = p.get(capi.PARAM_TB_MAX_SWEEPS, 16)
    min_cells = p.get(capi.PARAM_TB_MIN_CELLS, 0)
    return F16Model(oracle, fields, pressure_scale(n, p.get(capi.PARAM_F16_PRESSURE_SCALE, 1)),
                    lambda it, pressure: schedule(n, it, pressure, variant, max_t, min_cells))


def make_fields(kind, n, rng, oracle):
    """the six fields of one input class"""
    shape = (n + 2, n + 2)

    def signed(mag):
        return (np.where(rng.random(shape) < 0.5, -1.0, 1.0) * mag).astype(np.float32)

    if kind == "parameters":
        from fluidsimulationcuda_amd.harness import initialize_parameters
        return initialize_parameters(n, seed=int(rng.integers(1 << 30)))
    if kind == "portable":
        dens, dens0, u, u0, v, v0 = oracle.initialize_portable(n, seed=int(rng.integers(1 << 30)))
        return dict(u=u, v=v, dens=dens, u_prev=u0, v_prev=v0, dens_prev=dens0)
    if kind == "uniform":
        return {k: rnd(rng, n) for k in NAMES}
    if kind == "coarse":
        return {k: rng.choice(COARSE, size=shape).astype(np.float32) for k in NAMES}
    if kind == "subnormal":
        # velocities and their sources in fp16's subnormal range (2^-24 ... 2^-14), zeros of both signs among them
        out = {k: signed(2.0 ** rng.uniform(-24, -14, shape)) for k in ("u", "v", "u_prev", "v_prev")}
        for a in out.values():
            a[rng.random(shape) < 0.1] = 0.0
            a[rng.random(shape) < 0.1] = -0.0
        out.update(dens=rnd(rng, n, 0, 1), dens_prev=rnd(rng, n, 0, 1))
        return out
    if kind == "large":
        # magnitudes from 1/4 up to 2^15: back-traces leave the grid, sums and scaled divergences reach fp16's overflow
        return {k: signed(2.0 ** rng.uniform(-2, 15, shape)) for k in NAMES}
    if kind == "nonfinite":
        # islands of +inf, -inf and NaN (a NaN velocity pins the back-trace: Model.advect_numpy)
        out = {k: rnd(rng, n) for k in NAMES}
        for _ in range(int(rng.integers(1, 4))):
            k = NAMES[rng.integers(len(NAMES))]
            w = int(rng.integers(1, 4))
            i, j = int(rng.integers(0, n + 2)), int(rng.integers(0, n + 2))
            out[k][i:i + w, j:j + w] = F32(rng.choice([np.inf, -np.inf, np.nan]))
        return out
    raise ValueError(kind)


def f16_solver(n, params=None, variant=3):
    import fluidsimulationcuda_amd as F
    from fluidsimulationcuda_amd import capi
    return F.FluidSolver(n, jacobi=variant, storage=capi.STORAGE_F16, params=params)


def compare(s, m, what):
    """the launches of the model's schedule, then all six fields as the API returns them (NaN where the model has NaN,
    the bits of everything else)"""
    t = s.timing_read(reset=True)
    assert t["jacobi_field_launches"] == m.field_launches, \
        "%s: %d field launches, the model's schedule %d" % (what, t["jacobi_field_launches"], m.field_launches)
    m.field_launches = 0
    for k in NAMES:
        same_bits(s.download(k), m.download(k), "%s -- %s" % (k, what))


def run_steps(oracle, n, fields, iters, params=None, variant=3, what="", separate=True, dt=DT, diff=DIFF, visc=VISC,
              sources=(True, False, False, True)):
    """a sourced step, two plain ones, a sourced step that consumes the scaled u_prev / v_prev the last one left in place
    (`sources`), then (`separate`) vel_step and dens_step on their own; the library and the model compared after each
    call"""
    m = model_of(oracle, n, fields, params, variant)
    with f16_solver(n, params, variant) as s:
        s.timing_enable(True)
        s.upload(**fields)
        s.timing_read(reset=True)
        for k, src in enumerate(sources):
            s.step(1, use_sources=src, dt=dt, diff=diff, visc=visc, iters=iters)
            m.step(src, dt, diff, visc, iters)
            compare(s, m, "%s: step %d (%s) n=%d iters=%d" % (what, k + 1, "sourced" if src else "plain", n, iters))
        if separate:
            s.vel_step(visc, dt, iters)
            m.vel_step(visc, dt, iters)
            compare(s, m, "%s: vel_step n=%d iters=%d" % (what, n, iters))
            s.dens_step(diff, dt, iters)
            m.dens_step(diff, dt, iters)
            compare(s, m, "%s: dens_step n=%d iters=%d" % (what, n, iters))
    return m


# ---- the model itself (no GPU) ----------------------------------------------------------------------------------------
def test_model_without_rounding_is_the_oracle(oracle):
    """store = identity: the composed steps are the oracle's step_src / step bit for bit -- with S = 1, and with S = 8 too
    (a power of two scales fp32 arithmetic exactly: what is left is the model's bookkeeping of the scale) -- under the
    fused schedule and one sweep per launch"""
    rng = np.random.default_rng(3)
    for n in (1, 5, 30, 61):
        for it in (0, 2, 6, 10, 40):
            fields = {k: rng.uniform(-1, 1, (n + 2, n + 2)).astype(np.float32) for k in NAMES}
            for scale in (1.0, 8.0):
                for name, plan in (("fused", lambda i, p: launches(i)), ("single", lambda i, p: [1] * i)):
                    m = F16Model(oracle, fields, scale, plan, store=identity)
                    w = {k: a.copy() for k, a in fields.items()}
                    m.step(True, DT, DIFF, VISC, it)
                    oracle.step_src(w["u"], w["v"], w["dens"], w["u_prev"], w["v_prev"], w["dens_prev"], iters=it)
                    for k in NAMES:
                        assert_bit_equal(m.download(k), w[k], "sourced step n=%d iters=%d S=%g %s: %s" % (n, it, scale, name, k))
                    m.step(False, DT, DIFF, VISC, it)
                    oracle.step(w["u"], w["v"], w["dens"], w["u_prev"], w["v_prev"], w["dens_prev"], iters=it)
                    m.step(True, DT, DIFF, VISC, it)
                    oracle.step_src(w["u"], w["v"], w["dens"], w["u_prev"], w["v_prev"], w["dens_prev"], iters=it)
                    for k in NAMES:
                        assert_bit_equal(m.download(k), w[k], "three steps n=%d iters=%d S=%g %s: %s" % (n, it, scale, name, k))


def test_model_stores_fp16_values_and_leaves_the_projection_scaled(oracle):
    from fluidsimulationcuda_amd.harness import initialize_parameters
    n = 33
    m = F16Model(oracle, initialize_parameters(n), pressure_scale(n), lambda i, p: launches(i))
    m.step(True, DT, DIFF, VISC, 10)
    assert m.scaled == {"u_prev", "v_prev"}
    for k in NAMES:
        assert_bit_equal(h(m.f[k]), m.f[k], "stored %s" % k)


def test_model_pressure_scale():
    want = {1: 1, 15: 1, 16: 4, 17: 4, 31: 4, 32: 8, 33: 8, 1023: 128, 1024: 256, 1025: 256, 16382: 2048, 16384: 4096}
    for n, s in want.items():
        assert pressure_scale(n) == s, (n, pressure_scale(n), s)
        assert pressure_scale(n, 0) == 1
    for n in range(1, 16):
        assert pressure_scale(n) == 1


def test_model_schedule_is_the_libraries():
    """the model's launch depths are fluid_plan_sweeps' for fp16 storage, and those are the mode's stated schedule: the
    greedy 8 / 4 / 2 for every cap, grid and form (the deeper launches are fp32 only); one sweep per launch for variants
    0-2 and below TB_MIN_CELLS"""
    for max_t in (16, 12, 8, 4, 2):
        for iters in range(0, 50, 2):
            want = launches(iters, max_t)
            for n in (1, 16, 1022, 4094, 16382):
                for pressure in (False, True):
                    assert schedule(n, iters, pressure, max_t=max_t) == want, (n, iters, max_t, pressure)
            for variant in (0, 1, 2):
                assert schedule(61, iters, variant=variant, max_t=max_t) == [1] * iters
            assert schedule(61, iters, max_t=max_t, min_cells=61 * 61 + 1) == [1] * iters
            assert schedule(61, iters, max_t=max_t, min_cells=61 * 61) == want


# ---- GPU: steps ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("n", SIZES)
def test_steps_match_model(oracle, n, iters):
    rng = np.random.default_rng(100 * n + iters)
    run_steps(oracle, n, make_fields("portable" if iters % 4 else "parameters", n, rng, oracle), iters, what="default knobs")


@gpu
def test_large_grid_steps_match_model(oracle):
    """2046^2, the size the scale is for: the plain pressure of ordinary velocities, of the order h |u|, nears fp16's
    subnormals there"""
    n = 2046
    rng = np.random.default_rng(2046)
    run_steps(oracle, n, make_fields("portable", n, rng, oracle), 40, what="large grid", separate=False,
              sources=(True, False, True))


@gpu
@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("n", [5, 17, 61, 129, 254])
def test_input_classes_match_model(oracle, n, kind):
    rng = np.random.default_rng(n)
    run_steps(oracle, n, make_fields(kind, n, rng, oracle), 14 if n % 2 else 40, what=kind)


# ---- GPU: the knobs, one at a time -----------------------------------------------------------------------------------
# "speed only": FUSE_DIVERGENCE, FUSE_ADD_SOURCE, TB_FAST_DIVISION, TB_LANE_COLUMNS, TB_ROWS, TB_EDGE_ROWS_PCT,
# TB_AUTOTUNE, TB_FILL, TB_T16_MIN_CELLS; through the model's schedule or scale: TB_MAX_SWEEPS, TB_MIN_CELLS, the Jacobi
# variant, F16_PRESSURE_SCALE
KNOBS = ([("FUSE_DIVERGENCE", v) for v in (0, 1)] + [("FUSE_ADD_SOURCE", v) for v in (0, 1)]
         + [("TB_FAST_DIVISION", v) for v in (0, 1, 2, 3)] + [("TB_LANE_COLUMNS", v) for v in (2, 4)]
         + [("TB_ROWS", v) for v in (0, 1, 5, 17, 1000)] + [("TB_EDGE_ROWS_PCT", v) for v in (0, 40, 100)]
         + [("TB_AUTOTUNE", v) for v in (0, 1)] + [("TB_FILL", v) for v in (0, 1)] + [("TB_T16_MIN_CELLS", v) for v in (0, -1)]
         + [("TB_MAX_SWEEPS", v) for v in (16, 12, 8, 4, 2)] + [("TB_MIN_CELLS", v) for v in (0, 1 << 30)]
         + [("F16_PRESSURE_SCALE", v) for v in (0, 1)] + [("jacobi", v) for v in (0, 1, 2, 3)])


@gpu
@pytest.mark.parametrize("knob,value", KNOBS)
def test_knob_gives_the_model_bits(oracle, knob, value):
    from fluidsimulationcuda_amd import capi
    params, variant = ({}, value) if knob == "jacobi" else ({getattr(capi, "PARAM_" + knob): value}, 3)
    for n, iters in ((113, 14), (241, 40), (33, 6)):
        rng = np.random.default_rng(n)
        run_steps(oracle, n, make_fields("portable", n, rng, oracle), iters, params, variant, "%s=%d" % (knob, value))


# ---- GPU: solves at the fused kernel's edges ---------------------------------------------------------------------------
# test_gpu_ops.TB_SIZES around every window width of 2- and 4-column lanes at depths 8 / 4 / 2, the smallest grids, and a
# few strips' worth of rows
EDGE_SIZES = [1, 2, 3, 5, 14, 61, 111, 112, 113, 119, 120, 121, 123, 124, 125, 239, 240, 241, 247, 248, 249, 257, 481]


@gpu
@pytest.mark.parametrize("fast_div", [0, 1, 2, 3])
@pytest.mark.parametrize("lane_cols", [2, 4])
@pytest.mark.parametrize("max_t", [8, 4, 2])
def test_fused_solves_at_the_kernels_edges(oracle, max_t, lane_cols, fast_div):
    """the fp16 twin of test_gpu_ops.test_temporal_blocking_matches_oracle: every depth, lane width and division mode
    (fast_div 0 true division, 1 the two-term reciprocal where |x0| allows it, 2 the scaled residual correction, 3 the
    double reciprocal; the pressure form's exact reciprocal), both forms, all three wall rules, tiny / ragged / huge
    strips; against emu_solve (one rounding per launch), with the launch count asserted"""
    import fluidsimulationcuda_amd as F
    from fluidsimulationcuda_amd import capi
    params = {capi.PARAM_TB_MIN_CELLS: 0, capi.PARAM_TB_LANE_COLUMNS: lane_cols, capi.PARAM_TB_MAX_SWEEPS: max_t,
              capi.PARAM_TB_FAST_DIVISION: fast_div}
    for n in EDGE_SIZES:
        rng = np.random.default_rng(600 + n)
        with f16_solver(n, params) as s:
            s.timing_enable(True)
            for rows in (0, 1, 3, 16, 5000):
                s.set_param(capi.PARAM_TB_ROWS, rows)
                for b, (alpha, beta), iters in ((0, (1.0, 4.0), 14), (1, F.coefficients(n, DT, VISC), 14),
                                                (2, F.coefficients(n, DT, DIFF), 14)):
                    x, x0 = rnd(rng, n), rnd(rng, n)
                    s.upload(u=x, v=x0)
                    s.timing_read(reset=True)
                    s.diffuse(b, "u", "v", alpha, beta, iters)
                    t = s.timing_read(reset=True)
                    plan = schedule(n, iters, (alpha, beta) == (1.0, 4.0), max_t=max_t)
                    what = "n=%d cols=%d maxT=%d div=%d rows=%d b=%d iters=%d" % (n, lane_cols, max_t, fast_div, rows, b, iters)
                    assert t["jacobi_launches"] == len(plan) and t["sweeps"] == iters, "%s: %r planned, %d launches" % (
                        what, plan, t["jacobi_launches"])
                    assert_bit_equal(s.download("u"), emu_solve(oracle, b, x, x0, alpha, beta, plan), what)
                    assert_bit_equal(s.download("v"), h(x0), "x0 untouched: " + what)


# ---- GPU: seeded random configurations ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("seed", range(N_FUZZ))
def test_random_f16_configuration_matches_model(oracle, seed):
    """the fp16 twin of test_gpu_random_configs.test_random_single_gpu_configuration_matches_oracle: the knobs above
    drawn together, with the input classes, against the model"""
    from test_gpu_random_configs import random_params
    from fluidsimulationcuda_amd import capi
    rng = np.random.default_rng(9000 + seed)
    n = int(rng.choice(SIZES[:-2]))               # (the largest two take seconds per seed with single-sweep kernels)
    iters = int(rng.choice([0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 28, 32, 36, 40, 44]))
    variant = int(rng.choice([3, 3, 3, 3, 0, 1, 2]))
    params = random_params(rng, capi)
    params[capi.PARAM_TB_FILL] = int(rng.choice([0, 1, 1]))
    params[capi.PARAM_F16_PRESSURE_SCALE] = int(rng.choice([0, 1, 1]))
    kind = str(rng.choice(INPUTS))
    fields = make_fields(kind, n, rng, oracle)
    dt, diff, visc = float(rng.choice([0.016, 0.1])), float(rng.choice([0.1, 0.0, 1e-4])), float(rng.choice([0.0025, 0.0, 0.3]))
    what = "seed %d: n=%d iters=%d variant=%d %s dt=%g diff=%g visc=%g %r" % (seed, n, iters, variant, kind, dt, diff, visc, params)
    run_steps(oracle, n, fields, iters, params, variant, what, separate=bool(rng.integers(2)), dt=dt, diff=diff, visc=visc)
