"""GPU: looking at an ensemble on the device -- fluid_residual_members / fluid_absmax_velocity_members (one maximum per
member), fluid_member_moments (sum and sum of squares per member, in double), fluid_ensemble_stats (mean and variance per
cell across the members) and fluid_ensemble_stats_ptr.

What each is held to (include/fluid_amd.h, "ensemble diagnostics"):
- the maxima: bit for bit what the scalar call returns on a one-member context that went through the same uploads and
  calls with member m's arrays and coefficients (the existing suites hold the scalar call to the float64 evaluation), the
  project's check_residual / absmax32 against member m's model fields on top;
- the moments: `==` math.fsum on dyadic data (every partial sum is representable, so any order is exact); on general data
  the textbook bound of a recursive double sum in any order, gamma = (n-1)u / (1 - (n-1)u) with n = N^2, u = 2^-53,
  times the sum of magnitudes -- derived, not measured; the same bits call after call and context after context;
- the statistics: the header's definition written as a numpy loop over the members in float64, every one of the (N+2)^2
  cells, bit for bit (NaN where the model has NaN);
- nothing is disturbed: call sequences with the new calls inserted leave every field of every member as the model has it
  and as the same sequence without them leaves it, with the same sweep and launch counts.
No tolerance here that is not derived above."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_ensemble import KINDS, compare_all, ensemble_ops, member_fields, play_ensemble, solver, upload_all
from test_gpu_f16 import h
from test_gpu_f16_steps import model_of
from test_gpu_lazy_state import COARSE, NAMES, Model, absmax32, check_residual, draw_fields, draw_sequence, play, same_bits

pytestmark = pytest.mark.gpu
F32 = np.float32
DT, VISC, DIFF = 0.016, 0.0025, 0.1
SIZES = [1, 14, 61, 129, 254, 1022]
MEMBERS = [1, 2, 3, 5, 16]
ITERS = 4
# distinct coefficients per member (member 0: the pressure form)
ALPHA = np.array([1.0] + [0.3 + 0.17 * m for m in range(1, 64)], F32)
BETA = (F32(1) + F32(4) * ALPHA).astype(F32)
BETA[0] = F32(4)


def stored(a, storage):
    """a host array as a context of this storage type holds it"""
    return h(a) if storage else np.array(a, F32, copy=True)


def model_for(oracle, n, fields, storage):
    return model_of(oracle, n, fields) if storage else Model(oracle, fields)


def settled(mod, *ks):
    """the model's fields as a reader that does not know a scale sees them (fp16: divided back and stored again)"""
    if hasattr(mod, "unscale"):
        mod.unscale(*ks)
    return [mod.f[k] for k in ks]


# ---- 1. maxima per member ------------------------------------------------------------------------------------------------
def stages(s, oracle, res, amax, mod=None):
    """The calls every context goes through, ensemble or one member, and what its reductions return at each stage:
    after the uploads; after a sourced step; after a plain step (fp16: u_prev / v_prev are kept scaled there); and with a
    field that is zero by definition and one that owes an increment.  res(x, x0, k) / amax(u, v) make the calls (k: which
    coefficients); with a model, each value is also checked against the model's fields."""
    out = []

    def both(x, x0, k):
        got = res(x, x0, k)
        if mod is not None:
            fx, fx0 = settled(mod, x, x0)
            a, b = coefficients_of(mod, k)
            check_residual(float(got), fx, fx0, float(a), float(b), "residual(%s, %s) stage %d" % (x, x0, len(out)))
        return got

    def vel(u, v):
        got = amax(u, v)
        if mod is not None:
            fu, fv = settled(mod, u, v)
            assert F32(got) == absmax32(fu, fv), "absmax(%s, %s) stage %d: %r, the model %r" % (u, v, len(out), got, absmax32(fu, fv))
        return got

    out.append([both("u", "u_prev", 0), both("dens", "dens", 0), vel("u", "v")])
    s.step(1, use_sources=True, iters=ITERS)
    if mod is not None:
        mod.step(True, DT, DIFF, VISC, ITERS)
    out.append([both("u_prev", "v_prev", 1), both("dens", "dens_prev", 0), vel("u", "v")])
    s.step(1, iters=ITERS)
    if mod is not None:
        mod.step(False, DT, DIFF, VISC, ITERS)
    out.append([both("u_prev", "v_prev", 0), both("dens", "u", 0), vel("u_prev", "v")])
    # dens_prev: zero by definition; u_prev: owes the increment dt * 0 (the fused kernel's deferred add_source)
    s.computeDivergenceAndPressure("u", "v", "dens_prev", "dens")
    s.add_source("u_prev", "dens_prev", DT)
    if mod is not None and not hasattr(mod, "unscale"):
        mod.o.divergence(mod.f["u"], mod.f["v"], mod.f["dens_prev"], mod.f["dens"])
        mod.o.add_source(mod.f["u_prev"], mod.f["dens_prev"], DT)
    else:
        mod = None              # (the fp16 model has no divergence operator: the one-member context is the yardstick here)
    out.append([both("u_prev", "dens_prev", 0), both("dens_prev", "u_prev", 0), vel("u_prev", "dens_prev"), vel("dens_prev", "dens_prev")])
    return out


def coefficients_of(mod, k):
    return mod.coef[k]


def one_member_yardstick(oracle, n, storage, m, fields):
    """member m alone: the scalar calls on a one-member context, checked against the model on the way"""
    mod = model_for(oracle, n, fields, storage)
    mod.coef = [(ALPHA[m], BETA[m]), (F32(1), F32(4))]
    with solver(n, 1, storage=storage) as one:
        one.upload(**fields)
        return stages(one, oracle, lambda x, x0, k: F32(one.residual(x, x0, float(mod.coef[k][0]), float(mod.coef[k][1]))),
                      lambda u, v: F32(one.absmax_velocity(u, v)), mod)


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n", SIZES)
def test_maxima_per_member(oracle, n, storage):
    fields = member_fields(oracle, n, max(MEMBERS), seed=n)       # member m's arrays do not depend on M
    want = [one_member_yardstick(oracle, n, storage, m, fields[m]) for m in range(max(MEMBERS))]
    for members in MEMBERS:
        coef = [(ALPHA[:members].copy(), BETA[:members].copy()), (np.full(members, 1, F32), np.full(members, 4, F32))]
        with solver(n, members, storage=storage) as s:
            upload_all(s, fields[:members])
            got = stages(s, oracle, lambda x, x0, k: s.residual_members(x, x0, coef[k][0], coef[k][1]),
                         lambda u, v: s.absmax_velocity_members(u, v))
            # equal coefficients: the classic call is the maximum of the per-member values, exactly
            per = s.residual_members("u", "v", 0.5, 3.0)
            assert per.dtype == F32 and per.shape == (members,)
            assert F32(per.max()) == F32(s.residual("u", "v", 0.5, 3.0)), "n=%d M=%d" % (n, members)
            assert F32(s.absmax_velocity_members().max()) == F32(s.absmax_velocity())
        for k, stage in enumerate(got):
            for c, values in enumerate(stage):
                assert values.dtype == F32 and values.shape == (members,)
                for m in range(members):
                    w = want[m][k][c]
                    assert not np.isnan(values[m])
                    assert values[m].view(np.uint32) == w.view(np.uint32), \
                        "n=%d M=%d storage=%d stage %d call %d member %d: %r, a one-member context %r" % (n, members, storage, k, c, m, values[m], w)


# ---- 2. moments, exact ---------------------------------------------------------------------------------------------------
def fsums(a):
    inner = a[1:-1, 1:-1].astype(np.float64).ravel()
    return math.fsum(inner.tolist()), math.fsum((inner * inner).tolist())


def check_exact(s, fields, what):
    sums, squares = s.member_moments("u")
    assert sums.dtype == np.float64 and squares.dtype == np.float64 and sums.shape == squares.shape == (len(fields),)
    for m, f in enumerate(fields):
        ws, wq = fsums(f)
        assert sums[m] == ws and squares[m] == wq, "%s member %d: (%r, %r), fsum (%r, %r)" % (what, m, sums[m], squares[m], ws, wq)


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n", SIZES)
def test_moments_are_exact_on_dyadic_data(n, storage):
    rng = np.random.default_rng(31 * n + storage)
    for members in MEMBERS:
        fields = [rng.choice(COARSE, size=(n + 2, n + 2)).astype(F32) for _ in range(members)]
        with solver(n, members, storage=storage) as s:
            for m, f in enumerate(fields):
                s.upload(member=m, u=f)
            check_exact(s, fields, "n=%d M=%d storage=%d" % (n, members, storage))
            # a field that is zero by definition: +0; a field of -0: a sum whose value is 0
            s.computeDivergenceAndPressure("u", "v", "dens_prev", "dens")
            sums, squares = s.member_moments("dens_prev")
            assert not sums.any() and not squares.any() and not np.signbit(sums).any() and not np.signbit(squares).any()
            s.fill("v", -0.0)
            sums, squares = s.member_moments("v")
            assert (sums == 0).all() and (squares == 0).all() and not np.signbit(squares).any()
            # either output alone
            L, dp = s_lib(), C.POINTER(C.c_double)
            only = np.empty(members, np.float64)
            assert L.fluid_member_moments(s._h, 0, only.ctypes.data_as(dp), None) == 0
            assert only.tolist() == [fsums(f)[0] for f in fields]
            assert L.fluid_member_moments(s._h, 0, None, only.ctypes.data_as(dp)) == 0
            assert only.tolist() == [fsums(f)[1] for f in fields]


def s_lib():
    from fluidsimulationcuda_amd import capi
    return capi.lib()


def test_moments_are_exact_on_a_large_grid():
    n, members = 4094, 4
    rng = np.random.default_rng(4094)
    fields = [rng.choice(COARSE, size=(n + 2, n + 2)).astype(F32) for _ in range(members)]
    with solver(n, members) as s:
        for m, f in enumerate(fields):
            s.upload(member=m, u=f)
        check_exact(s, fields, "n=4094 M=4")


# ---- 3. moments, general data --------------------------------------------------------------------------------------------
def general_field(rng, n, scale):
    mag = rng.uniform(0.25, 1.0, size=(n + 2, n + 2))
    sign = np.where(rng.random((n + 2, n + 2)) < 0.5, -1.0, 1.0)
    return (sign * mag * scale).astype(F32)


@pytest.mark.parametrize("n, members", [(14, 5), (61, 16), (254, 3), (1022, 2), (4094, 2)])
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -120, 2.0 ** 60], ids=["1", "2^-120", "2^60"])
def test_moments_of_general_data_within_the_summation_bound(n, members, scale):
    rng = np.random.default_rng(n + members)
    fields = [general_field(rng, n, scale) for _ in range(members)]
    count, u = n * n, 2.0 ** -53
    gamma = (count - 1) * u / (1 - (count - 1) * u)

    def moments():
        with solver(n, members) as s:
            for m, f in enumerate(fields):
                s.upload(member=m, dens=f)
            first = s.member_moments("dens")
            again = s.member_moments("dens")
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes(), "two calls in a row differ"
        return first

    sums, squares = moments()
    for m, f in enumerate(fields):
        x = f[1:-1, 1:-1].astype(np.float64).ravel()
        ws, wa, wq = math.fsum(x.tolist()), math.fsum(np.abs(x).tolist()), math.fsum((x * x).tolist())
        es, eq = abs(sums[m] - ws), abs(squares[m] - wq)
        print("n=%d M=%d scale=%g member %d: |sum err| %.3g (bound %.3g), |sumsq err| %.3g (bound %.3g)" % (n, members, scale, m, es, gamma * wa, eq, gamma * wq))
        assert es <= gamma * wa, "n=%d member %d: sum %r, fsum %r, bound %r" % (n, m, sums[m], ws, gamma * wa)
        assert eq <= gamma * wq, "n=%d member %d: sum of squares %r, fsum %r, bound %r" % (n, m, squares[m], wq, gamma * wq)
    other = moments()                                   # a second context in the same process: the same bits
    assert sums.tobytes() == other[0].tobytes() and squares.tobytes() == other[1].tobytes()


def test_moments_nan_stays_in_its_member():
    n, members = 61, 5
    rng = np.random.default_rng(5)
    fields = [general_field(rng, n, 1.0) for _ in range(members)]
    with solver(n, members) as s:
        for m, f in enumerate(fields):
            s.upload(member=m, u=f)
        clean = s.member_moments("u")
        bad = fields[2].copy()
        bad[17, 40] = np.nan
        s.upload(member=2, u=bad)
        sums, squares = s.member_moments("u")
    assert np.isnan(sums[2]) and np.isnan(squares[2])
    keep = [0, 1, 3, 4]
    assert sums[keep].tobytes() == clean[0][keep].tobytes() and squares[keep].tobytes() == clean[1][keep].tobytes()


# ---- 4. statistics across members ----------------------------------------------------------------------------------------
def stats_model(x):
    """include/fluid_amd.h, fluid_ensemble_stats: per cell, in float64, the members in order"""
    members = x.shape[0]
    with np.errstate(all="ignore"):
        xd = x.astype(np.float64)
        s = xd[0].copy()
        for m in range(1, members):
            s = s + xd[m]
        mean_d = s / np.float64(members)
        d = xd[0] - mean_d
        q = d * d
        for m in range(1, members):
            d = xd[m] - mean_d
            q = q + d * d
        return mean_d.astype(F32), (q / np.float64(members)).astype(F32)


def test_stats_model_on_the_definitions_corner_cases():
    """(the model itself: no device)"""
    z = np.full((3, 4, 4), -0.0, F32)
    mean, var = stats_model(z)
    assert np.signbit(mean).all() and (var == 0).all() and not np.signbit(var).any()
    one = np.array([[[1.5, np.inf], [np.nan, -0.0]]], F32)
    mean, var = stats_model(one)
    assert mean[0, 0] == 1.5 and mean[0, 1] == np.inf and np.isnan(mean[1, 0]) and np.signbit(mean[1, 1])
    assert var[0, 0] == 0 and np.isnan(var[0, 1]) and np.isnan(var[1, 0]) and var[1, 1] == 0


def hip_runtime():
    """the HIP runtime this process already holds (the one libfluid_amd.so runs on)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            lib = C.CDLL(line.split()[-1])
            lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            lib.hipMemcpy.restype = C.c_int
            return lib
    raise RuntimeError("no HIP runtime is loaded")


def read_stats_fields(s):
    """the two device fields behind ensemble_stats_ptr, whole: (N+2, pitch) arrays"""
    L = s_lib()
    pitch, xoff, ff = C.c_int(), C.c_int(), C.c_size_t()
    assert L.fluid_layout(s.n, C.byref(pitch), C.byref(xoff), C.byref(ff)) == 0
    s.synchronize()
    out = []
    for p in s.ensemble_stats_ptr():
        a = np.empty(ff.value, F32)
        assert hip_runtime().hipMemcpy(a.ctypes.data, p, a.nbytes, 2) == 0        # hipMemcpyDeviceToHost
        out.append(a.reshape(s.n + 2, pitch.value))
    return out, xoff.value


def check_stats(s, x, what):
    want_mean, want_var = stats_model(x)
    mean, var = s.ensemble_stats("u")
    same_bits(mean, want_mean, "mean -- " + what)
    same_bits(var, want_var, "variance -- " + what)
    # one at a time, and computed only: the device copies hold the same bits, pads untouched zeros
    only_mean, none = s.ensemble_stats("u", variance=False)
    assert none is None
    same_bits(only_mean, want_mean, "mean alone -- " + what)
    assert s.ensemble_stats("u", mean=False, variance=False) == (None, None)
    (dmean, dvar), xoff = read_stats_fields(s)
    w = x.shape[1]
    for name, dev, want in (("mean", dmean, want_mean), ("variance", dvar, want_var)):
        same_bits(dev[:, xoff:xoff + w], want, "%s on the device -- %s" % (name, what))
        pads = np.concatenate([dev[:, :xoff].ravel(), dev[:, xoff + w:].ravel()])
        assert not pads.view(np.uint32).any(), "%s: pad columns written -- %s" % (name, what)


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("n", SIZES)
def test_statistics_across_members(oracle, n, storage):
    for members in MEMBERS:
        # every input class in every member position on the smaller grids; from 16 members on one rotation holds them all
        for seed in (range(len(KINDS)) if members < len(KINDS) and n <= 129 else (0, 3) if members < len(KINDS) else (0,)):
            fields = member_fields(oracle, n, members, seed=seed)
            with solver(n, members, storage=storage) as s:
                for m, f in enumerate(fields):
                    s.upload(member=m, u=f["u"])
                x = np.stack([stored(f["u"], storage) for f in fields])
                check_stats(s, x, "n=%d M=%d storage=%d seed=%d" % (n, members, storage, seed))
    # cells that are -0 in every member, and cells that are equal in every member
    members = 3
    with solver(n, members, storage=storage) as s:
        x = np.stack([np.full((n + 2, n + 2), -0.0, F32)] * members)
        x[:, n // 2:, :] = F32(0.75)
        for m in range(members):
            s.upload(member=m, u=x[m])
        check_stats(s, x, "n=%d: -0 and constant cells" % n)
        mean, var = s.ensemble_stats("u")
        assert np.signbit(mean[:n // 2]).all() and not var.any()


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_statistics_of_many_members(oracle, storage):
    n, members = 61, 64
    fields = member_fields(oracle, n, members, seed=3)
    with solver(n, members, storage=storage) as s:
        for m, f in enumerate(fields):
            s.upload(member=m, u=f["u"])
        check_stats(s, np.stack([stored(f["u"], storage) for f in fields]), "n=61 M=64 storage=%d" % storage)


def test_statistics_of_a_large_grid():
    n, members = 4094, 4
    rng = np.random.default_rng(7)
    x = np.stack([rng.uniform(-1, 1, size=(n + 2, n + 2)).astype(F32) + F32(100 * (m % 2)) for m in range(members)])
    with solver(n, members) as s:
        for m in range(members):
            s.upload(member=m, u=x[m])
        check_stats(s, x, "n=4094 M=4")


def test_statistics_see_a_lazy_field_settled(oracle):
    """zero by definition, an increment owed: the statistics are those of the field a download would show"""
    n, members = 61, 3
    fields = member_fields(oracle, n, members, seed=1, kinds=("uniform", "coarse"))
    with solver(n, members) as s:
        upload_all(s, fields)
        s.computeDivergenceAndPressure("u", "v", "u_prev", "dens")        # u_prev: zero by definition
        s.add_source("dens_prev", "u_prev", [0.5, -0.25, 0.0])           # dens_prev owes +0 / -0 / +0 per member
        for name in ("u_prev", "dens_prev"):
            mean, var = s.ensemble_stats(name)
            want = stats_model(np.stack([s.download(name, member=m) for m in range(members)]))
            same_bits(mean, want[0], name)
            same_bits(var, want[1], name)


# ---- 5. nothing is disturbed ---------------------------------------------------------------------------------------------
COUNTERS = ("sweeps", "jacobi_launches", "jacobi_field_launches", "pressure_sweeps", "solves")


def insert_new_calls(rng, ops):
    ops = list(ops)
    for _ in range(int(rng.integers(3, 9))):
        kind = ("x_residual", "x_absmax", "x_moments", "x_stats", "x_stats_ptr")[rng.integers(5)]
        a, b = NAMES[rng.integers(6)], NAMES[rng.integers(6)]
        ops.insert(int(rng.integers(0, len(ops) + 1)), (kind, a, b, int(rng.integers(4))))
    return ops


def play_new(s, op, state):
    from fluidsimulationcuda_amd import capi
    kind, a, b, mode = op
    if kind == "x_residual":
        s.residual_members(a, b, ALPHA[:s.members], BETA[:s.members])
    elif kind == "x_absmax":
        s.absmax_velocity_members(a, b)
    elif kind == "x_moments":
        s.member_moments(a)
    elif kind == "x_stats":
        s.ensemble_stats(a, mean=bool(mode & 1), variance=bool(mode & 2))
        state["stats"] = True
    elif state.get("stats"):
        assert all(s.ensemble_stats_ptr())
    else:
        with pytest.raises(capi.FluidError):
            s.ensemble_stats_ptr()


def run_sequence(oracle, n, members, params, fields, ops, what, models):
    with solver(n, members, params=params) as s:
        s.timing_enable(True)
        upload_all(s, fields)
        s.timing_read(reset=True)
        state = {}
        for op in ops:
            if op[0].startswith("x_"):
                play_new(s, op, state)
            elif op[0] == "upload_member":
                s.upload(member=op[1], **{op[2]: op[3]})
                if models:
                    models[op[1]].f[op[2]][...] = op[3]
            elif op[0] == "download_member":
                got = s.download(op[2], member=op[1])
                if models:
                    same_bits(got, models[op[1]].f[op[2]], "%r -- %s" % (op[:3], what))
            elif models:
                play_ensemble(s, models, op, what)
            else:
                play(s, None, op, what)
        if models:
            compare_all(s, models, what)
        t = s.timing_read(reset=True)
        return [[s.download(k, member=m) for k in NAMES] for m in range(members)], {k: t[k] for k in COUNTERS}


@pytest.mark.parametrize("seed", range(24))
def test_new_calls_disturb_nothing(oracle, seed):
    from fluidsimulationcuda_amd import capi
    rng = np.random.default_rng(15000 + seed)
    n = int(rng.choice([1, 2, 3, 5, 8, 13, 31, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 200, 255, 256, 257]))
    members = int(rng.choice([1, 2, 3, 5]))
    params = {capi.PARAM_TB_T16_MIN_CELLS: int(rng.choice([0, -1]))}
    fields = [draw_fields(rng, n) for _ in range(members)]
    plain = []
    for op in ensemble_ops(rng, draw_sequence(rng, oracle, n), n, members):
        if op[0] == "upload_member":        # the array goes into the op, so that both runs upload the same one
            host = rng.choice(COARSE, size=(n + 2, n + 2)).astype(F32) if op[3] else np.full((n + 2, n + 2), op[3], F32)
            op = op[:3] + (host,)
        plain.append(op)
    ops = insert_new_calls(rng, plain)
    what = "seed %d n=%d M=%d %r: %r" % (seed, n, members, params, [op[:3] for op in ops])
    got, counts = run_sequence(oracle, n, members, params, fields, ops, what, [Model(oracle, f) for f in fields])
    ref, ref_counts = run_sequence(oracle, n, members, params, fields, plain, what, None)
    for m in range(members):
        for k, name in enumerate(NAMES):
            same_bits(got[m][k], ref[m][k], "member %d %s against the sequence without the new calls -- %s" % (m, name, what))
    assert counts == ref_counts, what


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(oracle):
    from fluidsimulationcuda_amd import capi
    import fluidsimulationcuda_amd as F
    n, members = 30, 5
    L = capi.lib()
    dp = C.POINTER(C.c_double)
    fields = member_fields(oracle, n, members, seed=2, kinds=("uniform", "coarse"))
    good = np.linspace(0.5, 1.5, members).astype(F32)
    out = np.empty(members, F32)
    dout = np.empty(members, np.float64)
    host = np.empty((n + 2, n + 2), F32)
    p, q = C.c_void_p(), C.c_void_p()

    def mf(a):
        return a.ctypes.data_as(capi._MF)

    with solver(n, members) as s:
        upload_all(s, fields)
        s.computeDivergenceAndPressure("u", "v", "u_prev", "v_prev")        # a lazy state that must survive the refusals
        s.add_source("dens", "u_prev", DT)
        hnd = s._h
        nan_beta = good.copy()
        nan_beta[3] = np.nan
        inf_alpha = good.copy()
        inf_alpha[1] = np.inf
        refused = [
            ("fluid_residual_members", lambda: L.fluid_residual_members(hnd, 0, 3, None, mf(good), mf(out)), b"alpha"),
            ("fluid_residual_members", lambda: L.fluid_residual_members(hnd, 0, 3, mf(good), None, mf(out)), b"beta"),
            ("fluid_residual_members", lambda: L.fluid_residual_members(hnd, 0, 3, mf(good), mf(good), None), b"out"),
            ("fluid_residual_members", lambda: L.fluid_residual_members(hnd, 12, 3, mf(good), mf(good), mf(out)), b"12"),
            ("fluid_residual_members", lambda: L.fluid_residual_members(hnd, 0, -1, mf(good), mf(good), mf(out)), b"-1"),
            ("fluid_residual_members", lambda: L.fluid_residual_members(hnd, 0, 3, mf(good), mf(nan_beta), mf(out)), b"member 3"),
            ("fluid_residual_members", lambda: L.fluid_residual_members(hnd, 0, 3, mf(inf_alpha), mf(good), mf(out)), b"member 1"),
            ("fluid_absmax_velocity_members", lambda: L.fluid_absmax_velocity_members(hnd, 0, 1, None), b"out"),
            ("fluid_absmax_velocity_members", lambda: L.fluid_absmax_velocity_members(hnd, 0, 12, mf(out)), b"12"),
            ("fluid_member_moments", lambda: L.fluid_member_moments(hnd, 0, None, None), b"null"),
            ("fluid_member_moments", lambda: L.fluid_member_moments(hnd, 99, dout.ctypes.data_as(dp), None), b"99"),
            ("fluid_ensemble_stats", lambda: L.fluid_ensemble_stats(hnd, -2, mf(host), None), b"-2"),
            ("fluid_ensemble_stats_ptr", lambda: L.fluid_ensemble_stats_ptr(hnd, C.byref(p), C.byref(q)), b"fluid_ensemble_stats"),
        ]
        for name, call, word in refused:
            L.fluid_synchronize(None)
            assert call() == capi.E_INVALID, name
            msg = L.fluid_last_error()
            assert name.encode() in msg and word in msg, (name, msg)
        # x == x0 is no error
        assert L.fluid_residual_members(hnd, 0, 0, mf(good), mf(good), mf(out)) == capi.OK
        models = [Model(oracle, f) for f in fields]
        for mod in models:
            mod.o.divergence(mod.f["u"], mod.f["v"], mod.f["u_prev"], mod.f["v_prev"])
            mod.o.add_source(mod.f["dens"], mod.f["u_prev"], DT)
        compare_all(s, models, "after the refusals")
    # row slabs: the maxima are the scalar calls with element 0 (test_gpu_member_params' rule); sums and statistics refused
    with F.FluidSolver(n, rank=0, nranks=2) as s:
        hnd = s._h
        for name, call in (("fluid_member_moments", lambda: L.fluid_member_moments(hnd, 0, dout.ctypes.data_as(dp), None)),
                           ("fluid_ensemble_stats", lambda: L.fluid_ensemble_stats(hnd, 0, mf(host), None)),
                           ("fluid_ensemble_stats_ptr", lambda: L.fluid_ensemble_stats_ptr(hnd, C.byref(p), C.byref(q)))):
            assert call() == capi.E_INVALID, name
            msg = L.fluid_last_error()
            assert name.encode() in msg and b"slab" in msg, (name, msg)
        s.upload(u=fields[0]["u"], u_prev=fields[0]["u_prev"])
        s.set_exchange(lambda kind, ids, depth, scalar: scalar)       # a fabric of one: nothing arrives, the maximum is its own
        got = s.residual_members("u", "u_prev", [0.5], [3.0])
        assert got.shape == (1,) and F32(got[0]) == F32(s.residual("u", "u_prev", 0.5, 3.0))
        assert F32(s.absmax_velocity_members("u", "u_prev")[0]) == F32(s.absmax_velocity("u", "u_prev"))
