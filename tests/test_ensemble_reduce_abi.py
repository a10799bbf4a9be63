"""CPU: the ensemble diagnostics (fluid_residual_members, fluid_absmax_velocity_members, fluid_member_moments,
fluid_ensemble_stats, fluid_ensemble_stats_ptr) refuse a null context before they touch a device, and FluidSolver has
the methods that wrap them.  (test_abi.py holds header, exports and the ctypes table against each other by itself.)"""
import ctypes as C

import numpy as np


def test_null_context_is_refused_by_name():
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    f = np.zeros(4, np.float32)
    d = (C.c_double * 4)()
    p, q = C.c_void_p(), C.c_void_p()
    mf = f.ctypes.data_as(capi._MF)
    calls = {
        "fluid_residual_members": lambda: L.fluid_residual_members(None, 0, 3, mf, mf, mf),
        "fluid_absmax_velocity_members": lambda: L.fluid_absmax_velocity_members(None, 0, 1, mf),
        "fluid_member_moments": lambda: L.fluid_member_moments(None, 0, d, d),
        "fluid_ensemble_stats": lambda: L.fluid_ensemble_stats(None, 0, None, None),
        "fluid_ensemble_stats_ptr": lambda: L.fluid_ensemble_stats_ptr(None, C.byref(p), C.byref(q)),
    }
    for name, call in calls.items():
        L.fluid_synchronize(None)                      # leaves another message behind
        assert call() == capi.E_INVALID, name
        msg = L.fluid_last_error()
        assert name.encode() in msg and b"null context" in msg, (name, msg)
    # null arrays are found before the context is looked at
    assert L.fluid_residual_members(None, 0, 3, None, mf, mf) == capi.E_INVALID
    assert b"fluid_residual_members" in L.fluid_last_error() and b"alpha" in L.fluid_last_error()


def test_solver_methods_exist():
    from fluidsimulationcuda_amd import FluidSolver
    for name in ("residual_members", "absmax_velocity_members", "member_moments", "ensemble_stats", "ensemble_stats_ptr"):
        assert callable(getattr(FluidSolver, name)), name


def test_bindings_take_the_headers_types():
    from fluidsimulationcuda_amd import capi
    dp = C.POINTER(C.c_double)
    assert capi.SIGNATURES["fluid_residual_members"] == [C.c_void_p, C.c_int, C.c_int, capi._MF, capi._MF, capi._MF]
    assert capi.SIGNATURES["fluid_absmax_velocity_members"] == [C.c_void_p, C.c_int, C.c_int, capi._MF]
    assert capi.SIGNATURES["fluid_member_moments"] == [C.c_void_p, C.c_int, dp, dp]
    assert capi.SIGNATURES["fluid_ensemble_stats"] == [C.c_void_p, C.c_int, capi._MF, capi._MF]
    assert capi.SIGNATURES["fluid_ensemble_stats_ptr"] == [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
