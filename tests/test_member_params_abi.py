"""CPU: the per-member entry points (fluid_step_members and its kin) -- what can be checked without a device: the argument
errors that are found before the device is touched, the Python broadcast of scalars and sequences to one value per member,
and FluidSolver's signatures, whose defaults a call written before these entry points existed relies on."""
import ctypes as C
import inspect

import numpy as np
import pytest

MEMBERS_CALLS = {
    # name: (arguments after the context with `A` where a per-member array goes, the arrays' names)
    "fluid_step_members": (("A", "A", "A", 20, 1, 0), ("dt", "diff", "visc")),
    "fluid_vel_step_members": (("A", "A", 20), ("dt", "visc")),
    "fluid_dens_step_members": (("A", "A", 20), ("dt", "diff")),
    "fluid_op_add_source_members": ((0, 3, "A"), ("dt",)),
    "fluid_op_jacobi_sweep_members": ((0, 0, 3, 2, "A", "A"), ("alpha", "beta")),
    "fluid_op_diffuse_members": ((0, 0, 3, "A", "A", 20), ("alpha", "beta")),
    "fluid_op_advect_members": ((0, 2, 5, 0, 1, "A"), ("dt",)),
}


def _args(template, arrays):
    it = iter(arrays)
    return [next(it) if a == "A" else a for a in template]


@pytest.mark.parametrize("name", sorted(MEMBERS_CALLS))
def test_null_context_and_null_arrays(name):
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    template, names = MEMBERS_CALLS[name]
    fn = getattr(L, name)
    good = np.full(4, 0.5, np.float32)
    ptr = good.ctypes.data_as(capi._MF)
    # a null context with every array in place
    assert fn(None, *_args(template, [ptr] * len(names))) == capi.E_INVALID
    msg = L.fluid_last_error()
    assert name.encode() in msg and b"null context" in msg, msg
    # each array null in turn (found before the context is looked at, so a null context does not hide it)
    for k, arg in enumerate(names):
        arrays = [ptr] * len(names)
        arrays[k] = None
        assert fn(None, *_args(template, arrays)) == capi.E_INVALID, (name, arg)
        msg = L.fluid_last_error()
        assert name.encode() in msg and b"null array" in msg and arg.encode() in msg, msg


def test_every_members_call_is_bound_and_declared():
    from fluidsimulationcuda_amd import capi
    from test_abi import header_functions
    declared = set(header_functions())
    for name in MEMBERS_CALLS:
        assert name in capi.SIGNATURES and name in declared, name
        assert capi.SIGNATURES[name][0] is capi._ctx
        assert capi.SIGNATURES[name].count(capi._MF) == len(MEMBERS_CALLS[name][1])


def test_broadcast_scalars_mean_the_scalar_entry_point():
    from fluidsimulationcuda_amd.solver import member_values
    assert member_values(5, dt=0.016, diff=0.1, visc=0.0025) is None
    assert member_values(5, dt=np.float32(0.016)) is None
    assert member_values(5, dt=1, visc=np.float64(2.0), diff=np.array(3.0)) is None     # 0-d arrays are scalars
    assert member_values(1, dt=0.5) is None


def test_broadcast_sequences_and_mixed():
    from fluidsimulationcuda_amd.solver import member_values
    out = member_values(3, dt=0.016, diff=[0.1, 0.0, 1e-4], visc=(1, 2, 3))
    assert list(out) == ["dt", "diff", "visc"]
    for a in out.values():
        assert a.dtype == np.float32 and a.shape == (3,) and a.flags.c_contiguous
    assert np.array_equal(out["dt"], np.full(3, np.float32(0.016)))
    assert np.array_equal(out["diff"], np.array([0.1, 0.0, 1e-4], np.float32))
    assert np.array_equal(out["visc"], np.array([1, 2, 3], np.float32))
    # non-float input: integers, float64, a strided view, a generator-built list, -0.0 keeps its sign
    out = member_values(4, dt=np.arange(8, dtype=np.int64)[::2], visc=np.linspace(0, 1, 4), diff=[-0.0, 0, 1, 2])
    assert np.array_equal(out["dt"], np.array([0, 2, 4, 6], np.float32)) and out["dt"].flags.c_contiguous
    assert out["visc"].dtype == np.float32
    assert np.signbit(out["diff"][0]) and not np.signbit(out["diff"][1])
    # a sequence of one on a one-member solver is still the per-member path (which the library maps to the scalar call)
    out = member_values(1, dt=[0.25])
    assert out["dt"].shape == (1,) and out["dt"][0] == np.float32(0.25)
    # the caller's array is not aliased: what the library is handed does not change when the caller overwrites theirs
    mine = np.array([1, 2, 3], np.float64)
    out = member_values(3, dt=mine)
    mine[:] = 9
    assert np.array_equal(out["dt"], np.array([1, 2, 3], np.float32))


@pytest.mark.parametrize("bad", [[0.1, 0.2], [0.1, 0.2, 0.3, 0.4], [], [[0.1, 0.2, 0.3]], np.zeros((3, 1))])
def test_broadcast_wrong_length(bad):
    from fluidsimulationcuda_amd.solver import member_values
    with pytest.raises(ValueError, match="visc"):
        member_values(3, dt=0.016, visc=bad)


def test_broadcast_rejects_what_is_not_a_number():
    from fluidsimulationcuda_amd.solver import member_values
    with pytest.raises((ValueError, TypeError)):
        member_values(3, dt=["a", "b", "c"])


def test_wrong_length_raises_before_any_library_call():
    """a solver object without a context: the length error must come first (a library call on the null handle would raise
    FluidError instead)"""
    from fluidsimulationcuda_amd.solver import FluidSolver
    s = FluidSolver.__new__(FluidSolver)
    s._h, s.n, s.members = C.c_void_p(), 30, 3
    for call in (lambda: s.step(1, visc=[1, 2]), lambda: s.vel_step(visc=[1, 2, 3, 4]), lambda: s.dens_step(dt=[1.0]),
                 lambda: s.add_source("u", "u_prev", dt=[1, 2]), lambda: s.diffuse(0, "u", "u_prev", [1, 2], 4.0),
                 lambda: s.jacobi_sweep(0, "u", "u_prev", "dens", 1.0, [4, 4]), lambda: s.advect(0, "dens", "dens_prev", "u", "v", [1])):
        with pytest.raises(ValueError):
            call()


def test_solver_signatures_keep_their_defaults():
    from fluidsimulationcuda_amd import solver
    S = solver.FluidSolver

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()][1:]

    E = inspect.Parameter.empty
    assert sig(S.step) == [("nsteps", 1), ("use_sources", False), ("dt", solver.DT), ("diff", solver.DIFF), ("visc", solver.VIS),
                           ("iters", solver.ITERS)]
    assert sig(S.vel_step) == [("visc", solver.VIS), ("dt", solver.DT), ("iters", solver.ITERS)]
    assert sig(S.dens_step) == [("diff", solver.DIFF), ("dt", solver.DT), ("iters", solver.ITERS)]
    assert sig(S.add_source) == [("x", E), ("s", E), ("dt", solver.DT)]
    assert sig(S.jacobi_sweep) == [("b", E), ("x", E), ("x0", E), ("out", E), ("alpha", E), ("beta", E)]
    assert sig(S.diffuse) == [("b", E), ("x", E), ("x0", E), ("alpha", E), ("beta", E), ("iters", solver.ITERS)]
    assert sig(S.advect) == [("b", E), ("d", E), ("d0", E), ("u", E), ("v", E), ("dt", solver.DT)]
    assert (solver.DT, solver.VIS, solver.DIFF, solver.ITERS) == (0.016, 0.0025, 0.1, 40)
