"""GPU: the deferred state of a field (FieldState, fluid_ctx.h) carried from one operator call into the next.

A field can be zero by definition without zeros in memory (`zero`), owe an increment in every cell (`pend`: add_source of a
zero source under the fused Jacobi kernel) or, with fp16 storage, be kept multiplied by a power of two (`fscale`).  Every
reader must settle such a state and every writer must drop it.  The other tests start each operator from a fresh upload,
and a download settles the field, so they never see a state that crosses a call boundary.  Here a producer leaves the
state, a consumer reads it in one operand position, and the six user fields are downloaded only at the end and compared,
bit for bit, with the oracle applied eagerly to a numpy copy of the fields (the Model below).

- test_transition: the table.  Fields of -0 (a lost +0 increment shows as a sign) and NaN increments (a lost NaN shows).
- test_random_sequence: seeded operator sequences on one context, with parameter changes between the calls.
- test_random_sequence_on_slabs: the same sequences on 2-4 fake ranks (test_gpu_slab.py): one context's bits.
- test_f16_scaled_fields: the scaled u_prev / v_prev an fp16 step leaves, read by every consumer.
"""
import os

import numpy as np
import pytest

from conftest import assert_bit_equal

gpu = pytest.mark.gpu
NAMES = ("u", "v", "dens", "u_prev", "v_prev", "dens_prev")
DT, VISC, DIFF = 0.016, 0.0025, 0.1
N = 30
# more seeds for a one-off soak: FLUID_FUZZ_SEQUENCES=2000 FLUID_FUZZ_SEQUENCE_SLABS=500
N_SEQ = int(os.environ.get("FLUID_FUZZ_SEQUENCES", "200"))
N_SEQ_SLABS = int(os.environ.get("FLUID_FUZZ_SEQUENCE_SLABS", "48"))
SIZES = [1, 2, 3, 5, 8, 13, 31, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 200, 255, 256, 257, 333, 511]
COARSE = np.array([-1, -0.5, -0.25, 0.0, -0.0, 0.25, 0.5, 1], np.float32)
F32 = np.float32


def canon(a):
    """NaN payloads and signs are not part of the contract (the host and the device make different default NaNs)"""
    a = np.array(a, np.float32, copy=True)
    a[np.isnan(a)] = np.float32(np.nan)
    return a


def same_bits(got, want, what):
    assert_bit_equal(canon(got), canon(want), what)


def residual32(x, x0, alpha, beta):
    """k_residual in float: max |beta*x - alpha*(L + R + U + D) - x0| over the interior, NaN cells skipped (fmaxf), from 0"""
    with np.errstate(all="ignore"):
        nb = ((x[1:-1, :-2] + x[1:-1, 2:]) + x[:-2, 1:-1]) + x[2:, 1:-1]
        r = np.abs((F32(beta) * x[1:-1, 1:-1] - F32(alpha) * nb) - x0[1:-1, 1:-1])
    return F32(np.fmax.reduce(r.ravel(), initial=F32(0)))


def check_residual(got, x, x0, alpha, beta, what):
    """float64 evaluation; NaN cells are skipped as the kernel's fmaxf skips them, so NaN-ness of the result must agree (it
    is never NaN) and a finite result must agree to 1e-5 of itself plus 1e-6 of the operands' magnitude"""
    x, x0 = x.astype(np.float64), x0.astype(np.float64)
    with np.errstate(all="ignore"):
        nb = x[1:-1, :-2] + x[1:-1, 2:] + x[:-2, 1:-1] + x[2:, 1:-1]
        r = np.abs(beta * x[1:-1, 1:-1] - alpha * nb - x0[1:-1, 1:-1])
        ops = np.abs(beta * x[1:-1, 1:-1]) + np.abs(alpha * nb) + np.abs(x0[1:-1, 1:-1])
    r, ops = r[~np.isnan(r)], ops[np.isfinite(ops)]
    want = float(r.max()) if r.size else 0.0
    scale = float(ops.max()) if ops.size else 0.0
    assert np.isnan(got) == np.isnan(want), "%s: residual %r, float64 %r" % (what, got, want)
    if np.isinf(want) or np.isinf(got):
        assert got == want, "%s: residual %r, float64 %r" % (what, got, want)
    else:
        assert abs(got - want) <= 1e-5 * want + 1e-6 * scale, "%s: residual %r, float64 %r" % (what, got, want)


def absmax32(u, v):
    return F32(np.fmax.reduce(np.concatenate([np.abs(u[1:-1, 1:-1]).ravel(), np.abs(v[1:-1, 1:-1]).ravel()]), initial=F32(0)))


class Model:
    """The six fields as numpy arrays; every operator applied at once with the oracle's arithmetic.  Advection is the one
    exception: a NaN back-trace coordinate sends the reference's (int) cast into undefined behaviour, and the kernels pin it
    to the lower bound (fluid_kernels.hip: advect_trace), so such an advection is restated in numpy with that rule (equal to
    the oracle wherever the oracle is defined: test_model_matches_oracle).  The steps are composed from these operators."""

    def __init__(self, oracle, fields):
        self.o = oracle
        self.f = {k: np.array(fields[k], np.float32, copy=True) for k in NAMES}
        self.n = self.f["u"].shape[0] - 2

    def advect(self, b, d, d0, u, v, dt):
        with np.errstate(all="ignore"):
            dt0 = F32(dt) * F32(self.n)
            nan_trace = np.isnan(dt0 * u[1:-1, 1:-1]).any() or np.isnan(dt0 * v[1:-1, 1:-1]).any()
        if nan_trace:
            self.advect_numpy(b, d, d0, u, v, dt)
        else:
            self.o.advect(b, d, d0, u, v, dt)

    def advect_numpy(self, b, d, d0, u, v, dt):
        """FluidSequential.c:107-141 in float, a NaN coordinate clamped to 0.5 (fmax / fmin)"""
        n = self.n
        i, j = np.meshgrid(np.arange(1, n + 1, dtype=np.float32), np.arange(1, n + 1, dtype=np.float32), indexing="ij")
        with np.errstate(all="ignore"):
            dt0 = F32(dt) * F32(n)
            px = np.fmin(np.fmax(j - dt0 * u[1:-1, 1:-1], F32(0.5)), F32(n) + F32(0.5))
            py = np.fmin(np.fmax(i - dt0 * v[1:-1, 1:-1], F32(0.5)), F32(n) + F32(0.5))
            j0, i0 = px.astype(np.int64), py.astype(np.int64)
            s1 = px - j0.astype(np.float32)
            s0 = F32(1) - s1
            t1 = py - i0.astype(np.float32)
            t0 = F32(1) - t1
            a = t0 * d0[i0, j0] + t1 * d0[i0 + 1, j0]
            c = t0 * d0[i0, j0 + 1] + t1 * d0[i0 + 1, j0 + 1]
            d[1:-1, 1:-1] = s0 * a + s1 * c
        self.o.set_bnd(b, d)

    def project(self, it, u, v, p, div):
        self.o.divergence(u, v, p, div)
        self.o.diffuse(0, p, div, 1.0, 4.0, it)
        self.o.subtract_gradient(u, v, p)

    def vel_step(self, visc, dt, it):
        o, f = self.o, self.f
        u, v, u0, v0 = f["u"], f["v"], f["u_prev"], f["v_prev"]
        o.add_source(u, u0, dt)
        o.add_source(v, v0, dt)
        a, b = o.coefficients(self.n, dt, visc)
        o.diffuse(1, u0, u, a, b, it)
        o.diffuse(2, v0, v, a, b, it)
        self.project(it, u0, v0, u, v)
        self.advect(1, u, u0, u0, v0, dt)
        self.advect(2, v, v0, u0, v0, dt)
        self.project(it, u, v, u0, v0)

    def dens_step(self, diff, dt, it):
        o, f = self.o, self.f
        x, x0 = f["dens"], f["dens_prev"]
        o.add_source(x, x0, dt)
        a, b = o.coefficients(self.n, dt, diff)
        o.diffuse(0, x0, x, a, b, it)
        self.advect(0, x, x0, f["u"], f["v"], dt)

    def step(self, use_sources, dt, diff, visc, it):
        if not use_sources:
            for k in ("u_prev", "v_prev", "dens_prev"):
                self.f[k][...] = 0.0
        self.vel_step(visc, dt, it)
        self.dens_step(diff, dt, it)


def read_ptr(s, name):
    """the field through its device address: a view of the torch-owned arena (test_gpu_slab._init_fake)"""
    p = s.field_ptr(name)
    s.synchronize()
    off = p - s.arena.data_ptr()
    assert off >= 0 and off % s._fb == 0, "field_ptr(%s) is not a field slot of the arena" % name
    return s._views[off // s._fb][:, s.xoff:s.xoff + s.n + 2].float().cpu().numpy()


def play(s, m, op, what):
    """one operator call on the library (s) and, if m is given, on the model -- with what it returns checked"""
    kind, a = op[0], op[1:]
    f = m.f if m is not None else None
    o = m.o if m is not None else None
    w = "%s: %r" % (what, op)
    if kind == "set_bnd":
        s.set_bnd(*a)
        if m: o.set_bnd(a[0], f[a[1]])
    elif kind == "add_source":
        s.add_source(*a)
        if m: o.add_source(f[a[0]], f[a[1]], a[2])
    elif kind == "jacobi":
        s.jacobi_sweep(*a)
        if m: o.jacobi_sweep(a[0], f[a[1]], f[a[2]], f[a[3]], a[4], a[5])
    elif kind == "diffuse":
        s.diffuse(*a)
        if m: o.diffuse(a[0], f[a[1]], f[a[2]], a[3], a[4], a[5])
    elif kind == "diffuse_tol":
        b, x, x0, alpha, beta, tol, max_iters, every = a
        it, res = s.diffuse_tol(*a)
        if m:
            done, r = 0, residual32(f[x], f[x0], alpha, beta)
            while r > tol and done < max_iters:
                blk = min(every, (max_iters - done) & ~1)
                if blk <= 0:
                    break
                o.diffuse(b, f[x], f[x0], alpha, beta, blk)
                done += blk
                r = residual32(f[x], f[x0], alpha, beta)
            assert it == done, "%s: %d sweeps, the model %d" % (w, it, done)
            check_residual(res, f[x], f[x0], alpha, beta, w)
    elif kind == "advect":
        s.advect(*a)
        if m: m.advect(a[0], f[a[1]], f[a[2]], f[a[3]], f[a[4]], a[5])
    elif kind == "divergence":
        s.computeDivergenceAndPressure(*a)
        if m: o.divergence(*(f[k] for k in a))
    elif kind == "gradient":
        s.lastProject(*a)
        if m: o.subtract_gradient(*(f[k] for k in a))
    elif kind == "residual":
        got = s.residual(*a)
        if m: check_residual(got, f[a[0]], f[a[1]], a[2], a[3], w)
        return got
    elif kind == "absmax":
        got = s.absmax_velocity(*a)
        if m: assert F32(got) == absmax32(f[a[0]], f[a[1]]), "%s: %r, want %r" % (w, got, absmax32(f[a[0]], f[a[1]]))
        return got
    elif kind == "fill":
        s.fill(*a)
        if m: f[a[0]][...] = a[1]
    elif kind == "upload_rows":
        name, lo, hi, value = a
        host = np.full((s.n + 2, s.n + 2), value, np.float32)
        s.upload_rows(name, host, lo, hi)
        if m: f[name][lo:hi] = host[lo:hi]
    elif kind == "download":
        got = s.download(a[0])
        if m: same_bits(got, f[a[0]], w)
    elif kind == "download_rows":
        name, lo, hi = a
        got = np.full((s.n + 2, s.n + 2), 7.0, np.float32)
        s.download_rows(name, got, lo, hi)
        if m: same_bits(got[lo:hi], f[name][lo:hi], w)
    elif kind == "field_ptr":
        if hasattr(s, "_views"):
            got = read_ptr(s, a[0])
            if m: same_bits(got, f[a[0]], w)
        else:
            s.field_ptr(a[0])
    elif kind == "variant":
        s.set_jacobi_variant(a[0])
    elif kind == "param":
        s.set_param(*a)
    elif kind == "vel_step":
        s.vel_step(*a)
        if m: m.vel_step(*a)
    elif kind == "dens_step":
        s.dens_step(*a)
        if m: m.dens_step(*a)
    elif kind == "step":
        use_sources, dt, diff, visc, it = a
        s.step(1, use_sources=use_sources, dt=dt, diff=diff, visc=visc, iters=it)
        if m: m.step(*a)
    else:
        raise ValueError(kind)
    return None


def arena_solver(n, params=None, jacobi=3, storage=0):
    """a one-rank context in a torch-owned arena, so that field_ptr can be read through a torch view"""
    from test_gpu_slab import _init_fake
    from fluidsimulationcuda_amd.solver import FluidSolver
    s = FluidSolver.__new__(FluidSolver)
    _init_fake(s, n, 0, 1, 0, jacobi, storage, params)
    return s


def run(oracle, fields, ops, what, params=None, jacobi=3):
    """the ops on a fresh context and on the model; the six fields compared at the end"""
    m = Model(oracle, fields)
    s = arena_solver(fields["u"].shape[0] - 2, params, jacobi)
    try:
        s.upload(**fields)
        for op in ops:
            play(s, m, op, what)
        got = {k: s.download(k) for k in NAMES}
    finally:
        s.close()
    for k in NAMES:
        same_bits(got[k], m.f[k], "%s -- %s after %r" % (k, what, ops))
    return m


# ---- 1. the transition table ---------------------------------------------------------------------------------------
def _coef():
    from oracle.oracle import Oracle
    return Oracle().coefficients(N, DT, VISC)


PRODUCERS = ["zero", "pend+0.016", "pend-0.016", "pend0", "pend+inf", "pend-inf", "pendnan", "zero_source"]
PEND_DT = {"pend+0.016": 0.016, "pend-0.016": -0.016, "pend0": 0.0, "pend+inf": np.inf, "pend-inf": -np.inf,
           "pendnan": np.nan}


def producer(kind, x):
    """ops that leave field x in state `kind`, and the fields' contents before them.  Everything is -0; the memory of a
    field about to be marked zero holds 0.75, so a reader that skips the zeros shows it."""
    others = [k for k in NAMES if k != x]
    a, b, d, s = others[:4]
    fields = {k: np.full((N + 2, N + 2), -0.0, np.float32) for k in NAMES}
    if kind == "zero":
        fields[x][...] = 0.75
        return fields, [("divergence", a, b, x, d)]
    if kind == "zero_source":       # x: a zero-marked field that has just been the source of a pending one
        fields[x][...] = 0.75
        return fields, [("divergence", a, b, x, d), ("add_source", s, x, 0.016)]
    fields[s][...] = 0.75
    return fields, [("divergence", a, b, s, d), ("add_source", x, s, PEND_DT[kind])]


def consumers():
    """name -> (the field x in the state, pre-producer ops, ops between producer and consumer, consumer ops(x, others))"""
    from fluidsimulationcuda_amd import capi
    A1, B1 = _coef()
    X = "dens"
    out = {}

    def add(name, fn, x=X, pre=(), mid=()):
        out[name] = (x, list(pre), list(mid), fn)

    add("set_bnd.x", lambda x, o: [("set_bnd", 1, x)])
    add("add_source.x", lambda x, o: [("add_source", x, o[0], 0.5)])
    add("add_source.s", lambda x, o: [("add_source", o[0], x, 0.5)])
    add("jacobi.x", lambda x, o: [("jacobi", 1, x, o[0], o[2], A1, B1)])
    add("jacobi.x0", lambda x, o: [("jacobi", 1, o[0], x, o[2], A1, B1)])
    configs = {"tb16": ([("param", capi.PARAM_TB_T16_MIN_CELLS, 0)], []),
               "tb2": ([("param", capi.PARAM_TB_MAX_SWEEPS, 2)], []),
               "tb_min_cells": ([("param", capi.PARAM_TB_MIN_CELLS, 1 << 30)], []),
               # the producer runs under the fused kernel (only it defers), the consumer after a switch
               "switch_stream": ([], [("variant", capi.JACOBI_STREAM)]),
               "switch_lds": ([], [("variant", capi.JACOBI_LDS)]),
               "switch_naive": ([], [("variant", capi.JACOBI_NAIVE)])}
    for cname, (pre, mid) in configs.items():
        for it in (0, 2, 16, 40):
            add("diffuse.x.%s.%d" % (cname, it), lambda x, o, it=it: [("diffuse", 1, x, o[0], A1, B1, it)], pre=pre, mid=mid)
            add("diffuse.x0.%s.%d" % (cname, it), lambda x, o, it=it: [("diffuse", 1, o[0], x, A1, B1, it)], pre=pre, mid=mid)
    add("diffuse_tol.x", lambda x, o: [("diffuse_tol", 1, x, o[0], A1, B1, 0.0, 8, 4)])
    add("diffuse_tol.x0", lambda x, o: [("diffuse_tol", 1, o[0], x, A1, B1, 0.0, 8, 4)])
    add("advect.d0", lambda x, o: [("advect", 0, o[0], x, o[2], o[3], DT)])
    add("advect.u", lambda x, o: [("advect", 0, o[0], o[1], x, o[3], DT)])
    add("advect.v", lambda x, o: [("advect", 0, o[0], o[1], o[2], x, DT)])
    add("divergence.u", lambda x, o: [("divergence", x, o[0], o[1], o[2])])
    add("divergence.v", lambda x, o: [("divergence", o[0], x, o[1], o[2])])
    add("gradient.u", lambda x, o: [("gradient", x, o[0], o[1])])
    add("gradient.v", lambda x, o: [("gradient", o[0], x, o[1])])
    add("gradient.p", lambda x, o: [("gradient", o[0], o[1], x)])
    add("residual.x", lambda x, o: [("residual", x, o[0], A1, B1)])
    add("residual.x0", lambda x, o: [("residual", o[0], x, A1, B1)])
    add("absmax.u", lambda x, o: [("absmax", x, o[0])])
    add("absmax.v", lambda x, o: [("absmax", o[0], x)])
    add("download", lambda x, o: [])
    add("download_rows", lambda x, o: [("download_rows", x, 3, 11)])
    add("upload_rows", lambda x, o: [("upload_rows", x, 5, 9, 0.25)])
    add("field_ptr", lambda x, o: [("field_ptr", x)])
    for x in ("u", "v", "u_prev", "v_prev"):
        add("vel_step.%s" % x, lambda x, o: [("vel_step", VISC, DT, 8)], x=x)
    for x in ("dens", "dens_prev", "u", "v"):
        add("dens_step.%s" % x, lambda x, o: [("dens_step", DIFF, DT, 8)], x=x)
    for x in NAMES:
        add("step_sources.%s" % x, lambda x, o: [("step", True, DT, DIFF, VISC, 8)], x=x)
    # writers: the state must go with the old contents (the end download reads x)
    add("writer.fill", lambda x, o: [("fill", x, -0.0)])
    add("writer.advect_d", lambda x, o: [("advect", 0, x, o[0], o[2], o[3], DT)])
    add("writer.divergence_p", lambda x, o: [("divergence", o[0], o[2], x, o[3])])
    add("writer.divergence_div", lambda x, o: [("divergence", o[0], o[2], o[3], x)])
    add("writer.jacobi_out", lambda x, o: [("jacobi", 1, o[0], o[2], x, A1, B1)])
    return out


CONSUMER_NAMES = ["set_bnd.x", "add_source.x", "add_source.s", "jacobi.x", "jacobi.x0"] + [
    "diffuse.%s.%s.%d" % (p, c, it) for c in ("tb16", "tb2", "tb_min_cells", "switch_stream", "switch_lds", "switch_naive")
    for it in (0, 2, 16, 40) for p in ("x", "x0")] + [
    "diffuse_tol.x", "diffuse_tol.x0", "advect.d0", "advect.u", "advect.v", "divergence.u", "divergence.v", "gradient.u",
    "gradient.v", "gradient.p", "residual.x", "residual.x0", "absmax.u", "absmax.v", "download", "download_rows",
    "upload_rows", "field_ptr"] + ["vel_step.%s" % x for x in ("u", "v", "u_prev", "v_prev")] + [
    "dens_step.%s" % x for x in ("dens", "dens_prev", "u", "v")] + ["step_sources.%s" % x for x in NAMES] + [
    "writer.fill", "writer.advect_d", "writer.divergence_p", "writer.divergence_div", "writer.jacobi_out"]


@pytest.fixture(scope="module")
def table():
    return consumers()


@gpu
@pytest.mark.parametrize("consumer", CONSUMER_NAMES)
@pytest.mark.parametrize("state", PRODUCERS)
def test_transition(oracle, table, state, consumer):
    x, pre, mid, fn = table[consumer]
    fields, prod = producer(state, x)
    others = [k for k in NAMES if k != x][::-1]
    run(oracle, fields, pre + prod + mid + fn(x, others), "%s -> %s" % (state, consumer))


@gpu
def test_issue_case_pending_first_guess_of_a_fused_solve(oracle):
    """fluid_op_add_source(X, P) with P zero-marked leaves X pending; the fused launches of a following diffusion must start
    from X + dt*(+0), not from X as it is in memory (n = 30, the default fused kernel)"""
    A1, B1 = _coef()
    z = np.full((N + 2, N + 2), -0.0, np.float32)
    for dt in (0.016, np.inf):
        fields = {k: z.copy() for k in NAMES}
        ops = [("divergence", "u", "v", "dens_prev", "u_prev"), ("add_source", "dens", "dens_prev", dt),
               ("diffuse", 0, "dens", "v_prev", A1, B1, 8)]
        m = run(oracle, fields, ops, "dt=%r" % dt)
        assert (np.isnan(m.f["dens"]).all() if np.isinf(dt) else (m.f["dens"].view(np.uint32) == 0).all())


@gpu
def test_zero_sources_stay_free_in_steps():
    """fluid_step(use_sources=0) adds its zero sources inside the diffusion's loads: no add_source kernel, over several
    steps.  The operator API's pending first guess does cost one."""
    import fluidsimulationcuda_amd as F
    from fluidsimulationcuda_amd.harness import initialize_parameters
    for n in (N, 126):
        with F.FluidSolver(n) as s:
            s.upload(**initialize_parameters(n, seed=3))
            s.step(1, use_sources=True)
            s.timing_enable(True)
            s.timing_read()
            s.step(3)
            t = s.timing_read()
            assert t["source_calls"] == 0 and t["solves"] > 0, t
            s.computeDivergenceAndPressure("u", "v", "dens_prev", "u_prev")
            s.add_source("dens", "dens_prev", DT)
            assert s.timing_read()["source_calls"] == 0
            s.diffuse(0, "dens", "v_prev", 1.0, 4.0, 8)
            assert s.timing_read()["source_calls"] == 1


# ---- 2. seeded sequences ---------------------------------------------------------------------------------------------
def draw_sequence(rng, oracle, n, slabs=False):
    """6-20 operator calls on the six user fields with the state-makers (divergence's p, add_source of a zero-marked
    source) and their readers common, steps with iters down to 0, parameter changes, now and then a non-finite dt.
    Slabs: finite dt only.  A NaN velocity pins the back-trace to the grid's lower bound, rows a slab does not hold, while
    the slabs' advect bound skips NaN (fmaxf): there the slabs differ from one context, in a case the reference leaves
    undefined (its (int) cast of NaN)."""
    from fluidsimulationcuda_amd import capi
    coefs = [(1.0, 4.0), oracle.coefficients(n, DT, VISC), oracle.coefficients(n, DT, DIFF), (0.5, 3.0)]
    zero, pend = set(), set()

    def pick(excl=(), hot=0.7):
        cand = [k for k in (zero | pend) if k not in excl]
        if cand and rng.random() < hot:
            return cand[rng.integers(len(cand))]
        rest = [k for k in NAMES if k not in excl]
        return rest[rng.integers(len(rest))]

    def read(*ks):
        for k in ks:
            zero.discard(k)
            pend.discard(k)

    def dt_src():
        if rng.random() < 0.12 and not slabs:
            return float(rng.choice([np.inf, -np.inf, np.nan]))
        return float(rng.choice([0.016, -0.016, 0.0, 0.5, -0.25]))

    kinds = ["divergence"] * 4 + ["add_source"] * 5 + ["diffuse"] * 4 + ["jacobi", "diffuse_tol", "advect", "advect",
             "gradient", "gradient", "residual", "absmax", "fill", "upload_rows", "download_rows", "vel_step",
             "dens_step", "step", "variant", "param", "param"]
    if not slabs:
        kinds += ["set_bnd", "field_ptr"]
    ops = []
    for _ in range(int(rng.integers(6, 21))):
        kind = kinds[rng.integers(len(kinds))]
        if kind == "divergence":
            u = pick(hot=0.3)
            v = pick((), 0.3)
            p = pick((u, v), 0.2)
            d = pick((u, v, p), 0.2)
            ops.append(("divergence", u, v, p, d))
            read(u, v, d)
            pend.discard(p)
            zero.add(p)
        elif kind == "add_source":
            s = pick(hot=0.85) if zero else pick()
            x = pick((s,))
            ops.append(("add_source", x, s, dt_src()))
            was_zero = s in zero
            read(x, s)
            if was_zero:
                zero.add(s)
                pend.add(x)
        elif kind == "diffuse":
            x = pick()
            x0 = pick((x,))
            a, b = coefs[rng.integers(len(coefs))]
            it = int(rng.choice([0, 2, 4, 6, 8, 10, 12, 16, 20, 24, 40]))
            ops.append(("diffuse", int(rng.integers(3)), x, x0, a, b, it))
            read(x)
            if it:
                zero.discard(x0)
        elif kind == "jacobi":
            x = pick()
            x0 = pick()
            out = pick((x, x0), 0.3)
            a, b = coefs[rng.integers(len(coefs))]
            ops.append(("jacobi", int(rng.integers(3)), x, x0, out, a, b))
            read(x, x0, out)
        elif kind == "diffuse_tol":
            x = pick()
            x0 = pick((x,))
            a, b = coefs[rng.integers(len(coefs))]
            ops.append(("diffuse_tol", int(rng.integers(3)), x, x0, a, b, float(rng.choice([0.0, 1e-3])),
                        int(rng.choice([0, 4, 8, 12])), int(rng.choice([2, 4]))))
            read(x, x0)
        elif kind == "advect":
            d0, u, v = pick(), pick(), pick()
            d = pick((d0, u, v), 0.3)
            dt = float(rng.choice([np.inf, np.nan])) if rng.random() < 0.05 and not slabs else DT
            ops.append(("advect", int(rng.integers(3)), d, d0, u, v, dt))
            read(d, d0, u, v)
        elif kind == "gradient":
            p = pick()
            u = pick((p,))
            v = pick((p, u))
            ops.append(("gradient", u, v, p))
            read(u, v, p)
        elif kind == "residual":
            x, x0 = pick(), pick()
            a, b = coefs[rng.integers(len(coefs))]
            ops.append(("residual", x, x0, a, b))
            read(x, x0)
        elif kind == "absmax":
            u, v = pick(), pick()
            ops.append(("absmax", u, v))
            read(u, v)
        elif kind == "fill":
            x = pick()
            ops.append(("fill", x, float(rng.choice([0.0, -0.0, 0.5]))))
            read(x)
        elif kind == "upload_rows":
            x = pick()
            lo = int(rng.integers(0, n + 2))
            hi = int(rng.integers(lo, n + 3))
            ops.append(("upload_rows", x, lo, hi, float(rng.choice([-0.0, 0.25]))))
            read(x)
        elif kind == "download_rows":
            x = pick()
            lo = int(rng.integers(0, n + 2))
            ops.append(("download_rows", x, lo, int(rng.integers(lo, n + 3))))
            read(x)
        elif kind == "set_bnd":
            x = pick()
            ops.append(("set_bnd", int(rng.integers(3)), x))
            read(x)
        elif kind == "field_ptr":
            x = pick()
            ops.append(("field_ptr", x))
            read(x)
        elif kind in ("vel_step", "dens_step", "step"):
            it = int(rng.choice([0, 2, 4, 8, 12, 20]))
            if kind == "vel_step":
                ops.append(("vel_step", VISC, DT, it))
            elif kind == "dens_step":
                ops.append(("dens_step", DIFF, DT, it))
            else:
                ops.append(("step", bool(rng.integers(2)), DT, DIFF, VISC, it))
            zero.clear()
            pend.clear()
        elif kind == "variant":
            ops.append(("variant", int(rng.choice([3, 3, 0, 1, 2]))))
        else:
            key, vals = [(capi.PARAM_TB_MAX_SWEEPS, [16, 12, 8, 4, 2]), (capi.PARAM_FUSE_ADD_SOURCE, [0, 1]),
                         (capi.PARAM_TB_FAST_DIVISION, [0, 1, 2, 3]), (capi.PARAM_TB_FILL, [0, 1])][rng.integers(4)]
            ops.append(("param", key, int(rng.choice(vals))))
    return ops


def draw_fields(rng, n):
    """coarse dyadic values with both zeros; now and then a field of -0 alone"""
    out = {}
    for k in NAMES:
        if rng.random() < 0.25:
            out[k] = np.full((n + 2, n + 2), -0.0, np.float32)
        else:
            out[k] = rng.choice(COARSE, size=(n + 2, n + 2)).astype(np.float32)
    return out


def with_downloads(rng, ops):
    """about a quarter of the seeds also download fields between the calls: a download must not change what follows"""
    if rng.random() >= 0.25:
        return ops
    ops = list(ops)
    for _ in range(int(rng.integers(1, 4))):
        ops.insert(int(rng.integers(0, len(ops) + 1)), ("download", NAMES[rng.integers(6)]))
    return ops


@gpu
@pytest.mark.parametrize("seed", range(N_SEQ))
def test_random_sequence(oracle, seed):
    from fluidsimulationcuda_amd import capi
    rng = np.random.default_rng(5000 + seed)
    n = int(rng.choice(SIZES))
    params = {capi.PARAM_TB_T16_MIN_CELLS: int(rng.choice([0, -1]))}
    fields = draw_fields(rng, n)
    ops = with_downloads(rng, draw_sequence(rng, oracle, n))
    run(oracle, fields, ops, "seed %d n=%d %r" % (seed, n, params), params=params)


@gpu
@pytest.mark.parametrize("seed", range(N_SEQ_SLABS))
def test_random_sequence_on_slabs(oracle, seed):
    """the same generator on 2-4 fake ranks, without set_bnd (whole-grid only): the ranks' fields are one context's bits,
    what the reductions return is the same, and that context is the model's"""
    from test_gpu_slab import run_ranks, single
    from fluidsimulationcuda_amd import capi
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.choice([61, 100, 126, 200, 254, 257]))
    nranks = int(rng.choice([2, 3, 4]))
    while n // nranks < 10:
        nranks -= 1
    halo = int(rng.choice([0, 1, 3, 8, 16, 40]))
    params = {capi.PARAM_TB_T16_MIN_CELLS: int(rng.choice([0, -1]))}
    fields = draw_fields(rng, n)
    ops = with_downloads(rng, draw_sequence(rng, oracle, n, slabs=True))
    what = "seed %d n=%d ranks=%d halo=%d %r: %r" % (seed, n, nranks, halo, params, ops)
    m = Model(oracle, fields)
    scalars = {}

    def body_single(s):
        for k, v in params.items():
            s.set_param(k, v)
        scalars["single"] = [r for r in (play(s, m, op, what) for op in ops) if r is not None]

    def body_rank(s):
        scalars[s.rank] = [r for r in (play(s, None, op, what) for op in ops) if r is not None]

    want = single(n, fields, body_single)
    got, fab = run_ranks(n, nranks, halo, fields, body_rank, jacobi=3, params=params)
    for r in range(1, nranks):
        assert fab.log[r] == fab.log[0], "rank %d issued a different exchange sequence -- %s" % (r, what)
    for r in range(nranks):
        assert canon(scalars[r]).tobytes() == canon(scalars["single"]).tobytes(), \
            "rank %d returned %r, one context %r -- %s" % (r, scalars[r], scalars["single"], what)
    for k in NAMES:
        same_bits(want[k], m.f[k], "one context vs model: %s -- %s" % (k, what))
        same_bits(got[k], want[k], "slabs vs one context: %s -- %s" % (k, what))


# ---- 4. fp16: the scaled fields a step leaves ------------------------------------------------------------------------
F16_CONSUMERS = ["set_bnd.x", "add_source.x", "add_source.s", "jacobi.x", "jacobi.x0", "diffuse.x", "diffuse.x0",
                 "diffuse.both_scaled", "diffuse.x.stream", "diffuse.x0.stream", "diffuse_tol.x", "advect.d0", "advect.u",
                 "advect.v", "divergence.u", "divergence.v", "gradient.u", "gradient.v", "gradient.p", "residual.x",
                 "residual.x0", "absmax.u", "download", "download_rows", "upload_rows", "field_ptr", "vel_step",
                 "step_sources"]


def h(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


@gpu
@pytest.mark.parametrize("x", ["u_prev", "v_prev"])
@pytest.mark.parametrize("consumer", F16_CONSUMERS)
def test_f16_scaled_fields(oracle, consumer, x):
    """After an fp16 step u_prev (the pressure) and v_prev (the divergence) are kept multiplied by 2^k.  Each consumer must
    see the plain values: h(download) -- the host divides exactly, the device's unscale rounds to fp16 the same way --
    except the gradient's pressure, divided inside the kernel (the download itself), and a diffusion whose x and x0 carry
    the same scale, which solves on the scaled values and keeps the result scaled.  Expected values follow the
    rounded-oracle recipe of test_gpu_f16.py; the steps and diffuse_tol compare with a fresh context given the plain
    values."""
    from test_gpu_f16 import emu_solve, launches
    from fluidsimulationcuda_amd import capi
    from fluidsimulationcuda_amd.harness import initialize_parameters
    n = 61
    k = int(np.frexp(np.float32(n))[1]) - 3
    scale = np.float32(2.0 ** k)
    init = initialize_parameters(n, seed=4)
    A1, B1 = oracle.coefficients(n, DT, VISC)
    other = "v_prev" if x == "u_prev" else "u_prev"
    o = ["dens", "dens_prev", "u", "v"]

    def stepped():
        s = arena_solver(n, jacobi=3, storage=capi.STORAGE_F16)
        s.upload(**init)
        s.step(1, use_sources=True)
        return s

    s = stepped()
    try:
        dl = {k_: s.download(k_) for k_ in NAMES}
    finally:
        s.close()
    m = {k_: dl[k_].copy() for k_ in NAMES}

    touched = set()

    def plain(*ks):                       # a reader that unscales: the field now holds h(download)
        for k_ in ks:
            m[k_] = h(m[k_])
            touched.add(k_)

    ops, post, twin = [], None, None
    c = consumer
    if c == "set_bnd.x":
        ops = [("set_bnd", 1, x)]
        plain(x)
        oracle.set_bnd(1, m[x])
    elif c == "add_source.x":
        ops = [("add_source", x, o[0], 0.5)]
        plain(x)
        oracle.add_source(m[x], m[o[0]], 0.5)
        m[x] = h(m[x])
    elif c == "add_source.s":
        ops = [("add_source", o[0], x, 0.5)]
        plain(x)
        oracle.add_source(m[o[0]], m[x], 0.5)
        m[o[0]] = h(m[o[0]])
    elif c in ("jacobi.x", "jacobi.x0"):
        xx, x0 = (x, o[0]) if c == "jacobi.x" else (o[0], x)
        ops = [("jacobi", 1, xx, x0, o[1], A1, B1)]
        plain(x)
        oracle.jacobi_sweep(1, m[xx], m[x0], m[o[1]], A1, B1)
        m[o[1]] = h(m[o[1]])
    elif c.startswith("diffuse.x") and c != "diffuse_tol.x":
        stream = c.endswith(".stream")
        xx, x0 = (x, o[0]) if c.startswith("diffuse.x.") or c == "diffuse.x" else (o[0], x)
        ops = ([("variant", capi.JACOBI_STREAM)] if stream else []) + [("diffuse", 1, xx, x0, A1, B1, 16)]
        plain(x)
        m[xx] = emu_solve(oracle, 1, m[xx], m[x0], A1, B1, [1] * 16 if stream else launches(16))
    elif c == "diffuse.both_scaled":
        ops = [("diffuse", 0, x, other, 1.0, 4.0, 16)]
        m[x] = emu_solve(oracle, 0, m[x] * scale, m[other] * scale, 1.0, 4.0, launches(16)) / scale
    elif c == "diffuse_tol.x":
        ops = [("diffuse_tol", 1, x, o[0], A1, B1, 0.0, 8, 4)]
        plain(x)
        twin = True
    elif c.startswith("advect."):
        pos = {"advect.d0": 2, "advect.u": 3, "advect.v": 4}[c]
        args = [0, "dens", "dens_prev", "u", "v", DT]
        args[pos] = x
        ops = [("advect",) + tuple(args)]
        plain(x)
        oracle.advect(0, m[args[1]], m[args[2]], m[args[3]], m[args[4]], DT)
        m[args[1]] = h(m[args[1]])
    elif c in ("divergence.u", "divergence.v"):
        u, v = (x, "v") if c == "divergence.u" else ("u", x)
        ops = [("divergence", u, v, "dens", "dens_prev")]
        plain(x)
        oracle.divergence(m[u], m[v], m["dens"], m["dens_prev"])
        m["dens_prev"] = h(m["dens_prev"])
    elif c in ("gradient.u", "gradient.v"):
        u, v = (x, "v") if c == "gradient.u" else ("u", x)
        ops = [("gradient", u, v, "dens")]
        plain(x)
        oracle.subtract_gradient(m[u], m[v], m["dens"])
        m[u], m[v] = h(m[u]), h(m[v])
    elif c == "gradient.p":
        ops = [("gradient", "u", "v", x)]
        oracle.subtract_gradient(m["u"], m["v"], m[x])
        m["u"], m["v"] = h(m["u"]), h(m["v"])
    elif c in ("residual.x", "residual.x0"):
        xx, x0 = (x, o[0]) if c == "residual.x" else (o[0], x)
        ops = [("residual", xx, x0, A1, B1)]
        plain(x)
        post = lambda got: check_residual(got, m[xx], m[x0], A1, B1, c)
    elif c == "absmax.u":
        ops = [("absmax", x, "v")]
        plain(x)
        post = lambda got: (np.float32(got) == absmax32(m[x], m["v"])) or pytest.fail("absmax %r" % got)
    elif c == "download":
        ops = []
    elif c == "download_rows":
        ops = [("download_rows", x, 3, 11)]
    elif c == "upload_rows":
        ops = [("upload_rows", x, 5, 9, 0.25)]
        plain(x)
        m[x][5:9] = 0.25
    elif c == "field_ptr":
        ops = [("field_ptr", x)]
        plain(x)
    elif c in ("vel_step", "step_sources"):
        ops = [("vel_step", VISC, DT, 40)] if c == "vel_step" else [("step", True, DT, DIFF, VISC, 40)]
        plain("u_prev", "v_prev")
        twin = True
    else:
        raise ValueError(c)

    s = stepped()
    try:
        rets = []
        for op in ops:
            if op[0] == "field_ptr":
                same_bits(read_ptr(s, x), m[x], "field_ptr")
            elif op[0] == "download_rows":
                got = np.full((n + 2, n + 2), 7.0, np.float32)
                s.download_rows(x, got, 3, 11)
                same_bits(got[3:11], m[x][3:11], "download_rows")
            else:
                rets.append(play(s, None, op, c))
        if post is not None and rets:
            post(rets[-1])
        got = {k_: s.download(k_) for k_ in NAMES}
    finally:
        s.close()
    if twin:
        # the same calls on a context that was given the plain values
        t = arena_solver(n, jacobi=3, storage=capi.STORAGE_F16)
        try:
            t.upload(**m)
            for op in ops:
                play(t, None, op, c)
            # (a field the calls did not read is still scaled there: its download is exact, not the twin's rounding)
            m = {k_: t.download(k_) if k_ in touched or k_ not in ("u_prev", "v_prev") else m[k_] for k_ in NAMES}
        finally:
            t.close()
    for k_ in NAMES:
        same_bits(got[k_], m[k_], "%s after %s (x = %s)" % (k_, c, x))


# ---- the model itself (no GPU) ----------------------------------------------------------------------------------------
def test_model_matches_oracle(oracle):
    """the numpy advection equals the oracle's where the oracle is defined, and the composed steps equal the oracle's"""
    rng = np.random.default_rng(1)
    for n in (1, 5, 30, 61):
        fields = {k: rng.uniform(-1, 1, (n + 2, n + 2)).astype(np.float32) for k in NAMES}
        m = Model(oracle, fields)
        for amp in (0.0, 1.0, 300.0):
            u, v = fields["u"] * F32(amp), fields["v"] * F32(amp)
            for b in (0, 1, 2):
                want, got = np.zeros_like(u), np.zeros_like(u)
                oracle.advect(b, want, fields["dens"], u, v, DT)
                m.advect_numpy(b, got, fields["dens"], u, v, DT)
                assert_bit_equal(got, want, "numpy advect n=%d amp=%g b=%d" % (n, amp, b))
        for it in (0, 4, 10):
            m = Model(oracle, fields)
            w = {k: a.copy() for k, a in fields.items()}
            m.step(True, DT, DIFF, VISC, it)
            oracle.step_src(w["u"], w["v"], w["dens"], w["u_prev"], w["v_prev"], w["dens_prev"], iters=it)
            m.step(False, DT, DIFF, VISC, it)
            oracle.step(w["u"], w["v"], w["dens"], w["u_prev"], w["v_prev"], w["dens_prev"], iters=it)
            for k in NAMES:
                assert_bit_equal(m.f[k], w[k], "composed steps n=%d iters=%d: %s" % (n, it, k))


def test_model_advection_pins_a_nan_trace_to_the_lower_bound(oracle):
    """a NaN velocity reads the cell at 0.5 (the kernels' fmax / fmin), whatever the other cells do"""
    n = 5
    d0 = np.arange((n + 2) ** 2, dtype=np.float32).reshape(n + 2, n + 2)
    u, v = np.zeros_like(d0), np.zeros_like(d0)
    u[2, 3] = np.nan
    d = np.zeros_like(d0)
    Model(oracle, {k: d0 for k in NAMES}).advect(0, d, d0, u, v, DT)
    # x pinned to 0.5: 0.5 * (d0[i, 0] + d0[i, 1]); y on the row itself
    assert d[2, 3] == np.float32(0.5) * d0[2, 0] + np.float32(0.5) * d0[2, 1]
    assert d[3, 3] == d0[3, 3]
