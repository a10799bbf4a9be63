"""ctypes binding of include/fluid_amd.h (libfluid_amd.so).

There is no fallback: if the HIP library is missing or a call fails, this
module raises.  Nothing here (or anywhere in this package) touches oracle/.
"""
import ctypes as C
import os

import numpy as np

from ._build import LIB

OK, E_INVALID, E_NOMEM, E_HIP, E_COMM = 0, 1, 2, 3, 4
U, V, DENS, U_PREV, V_PREV, DENS_PREV, TMP0, TMP1, TMP2, TMP3, TMP4, TMP5 = range(12)
NFIELDS = 12
JACOBI_STREAM, JACOBI_LDS, JACOBI_NAIVE, JACOBI_TB = 0, 1, 2, 3
STORAGE_F32, STORAGE_F16 = 0, 1
PARAM_TB_MAX_SWEEPS, PARAM_TB_ROWS, PARAM_HALO, PARAM_TB_FAST_DIVISION, PARAM_TB_MIN_CELLS, PARAM_TB_EDGE_ROWS_PCT = 0, 1, 2, 3, 4, 5
PARAM_TB_LANE_COLUMNS = 6
PARAM_TB_T16_MIN_CELLS = 7
PARAM_TB_AUTOTUNE = 8
PARAM_FUSE_DIVERGENCE = 9
PARAM_SLAB_OVERLAP = 10
PARAM_EARLY_ADVECT = 11
PARAM_FUSE_ADD_SOURCE = 12
PARAM_XCHG_OVERLAP = 13
PARAM_F16_PRESSURE_SCALE = 14
PARAM_TB_FILL = 15
XCHG_HALO, XCHG_GATHER, XCHG_MAX, XCHG_MAX_BEGIN, XCHG_MAX_END = 0, 1, 2, 3, 4
RCCL_ID_BYTES = 128
FIELD_NAMES = ("u", "v", "dens", "u_prev", "v_prev", "dens_prev", "tmp0", "tmp1", "tmp2", "tmp3", "tmp4", "tmp5")


class FluidError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libfluid_amd error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [("n", C.c_int), ("rank", C.c_int), ("nranks", C.c_int), ("halo", C.c_int),
                ("jacobi_variant", C.c_int), ("stream", C.c_void_p), ("arena", C.c_void_p),
                ("arena_bytes", C.c_size_t), ("storage", C.c_int)]


TIME_SOURCE, TIME_DIFFUSION, TIME_DIVERGENCE, TIME_PROJECTION, TIME_ADVECTION = range(5)
TIMING_CATEGORIES = ("source", "diffusion", "divergence", "projection", "advection")


class Timing(C.Structure):
    _fields_ = [("jacobi_ms", C.c_double), ("sweeps", C.c_longlong), ("solves", C.c_longlong),
                ("category_ms", C.c_double * 5), ("category_calls", C.c_longlong * 5),
                ("jacobi_launches", C.c_longlong), ("jacobi_field_launches", C.c_longlong),
                ("pressure_ms", C.c_double), ("pressure_sweeps", C.c_longlong)]


class RunPlan(C.Structure):
    """fluid_run_plan: a run of nsteps steps with optional forcing (sources) and optional recording (snapshots)"""
    _fields_ = [("iters", C.c_int), ("nsteps", C.c_int), ("use_sources", C.c_int), ("sources", C.c_void_p),
                ("every", C.c_int), ("fields", C.POINTER(C.c_int)), ("nfields", C.c_int),
                ("snapshots", C.c_void_p), ("capacity", C.c_size_t)]


class ObsWindow(C.Structure):
    """fluid_obs_window: which points of the resident network a windowed run observes after which step, and into what record"""
    _fields_ = [("field", C.c_int), ("nslots", C.c_int), ("slot_first", C.POINTER(C.c_int)), ("slot_step", C.POINTER(C.c_int)),
                ("record_dev", C.c_void_p), ("member_stride", C.c_size_t)]


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int,
                          C.POINTER(C.c_float))

_HOSTF = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_ctx = C.c_void_p
_i, _f = C.c_int, C.c_float
_MF = C.POINTER(C.c_float)          # one float per ensemble member (the *_members calls); None passes as a null pointer

# name -> argtypes; every listed function returns int status.  This table is
# also what tests/test_abi.py checks against include/fluid_amd.h.
SIGNATURES = {
    "step": [_i, _f, _f, _f, _HOSTF, _HOSTF, _HOSTF],
    "step_src": [_i, _f, _f, _f, _i] + [_HOSTF] * 6,
    "fluid_release_cached": [],
    "fluid_coefficients": [_i, _f, _f, C.POINTER(_f), C.POINTER(_f)],
    "fluid_layout": [_i, C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_size_t)],
    "fluid_create": [_i, C.POINTER(_ctx)],
    "fluid_create_ex": [C.POINTER(Config), C.POINTER(_ctx)],
    "fluid_create_ensemble": [C.POINTER(Config), _i, C.POINTER(_ctx)],
    "fluid_members": [_ctx, C.POINTER(_i)],
    "fluid_upload_member": [_ctx, _i, _i, _HOSTF],
    "fluid_download_member": [_ctx, _i, _i, _HOSTF],
    "fluid_step_members": [_ctx, _MF, _MF, _MF, _i, _i, _i],
    "fluid_vel_step_members": [_ctx, _MF, _MF, _i],
    "fluid_dens_step_members": [_ctx, _MF, _MF, _i],
    "fluid_op_add_source_members": [_ctx, _i, _i, _MF],
    "fluid_op_jacobi_sweep_members": [_ctx, _i, _i, _i, _i, _MF, _MF],
    "fluid_op_diffuse_members": [_ctx, _i, _i, _i, _MF, _MF, _i],
    "fluid_op_advect_members": [_ctx, _i, _i, _i, _i, _i, _MF],
    "fluid_destroy": [_ctx],
    "fluid_synchronize": [_ctx],
    "fluid_owned_rows": [_ctx, C.POINTER(_i), C.POINTER(_i)],
    "fluid_field_ptr": [_ctx, _i, C.POINTER(C.c_void_p)],
    "fluid_scalar_ptr": [_ctx, C.POINTER(C.c_void_p)],
    "fluid_upload": [_ctx, _i, _HOSTF],
    "fluid_download": [_ctx, _i, _HOSTF],
    "fluid_upload_rows": [_ctx, _i, _HOSTF, _i, _i],
    "fluid_download_rows": [_ctx, _i, _HOSTF, _i, _i],
    "fluid_fill": [_ctx, _i, _f],
    "fluid_step": [_ctx, _f, _f, _f, _i, _i, _i],
    "fluid_vel_step": [_ctx, _f, _f, _i],
    "fluid_dens_step": [_ctx, _f, _f, _i],
    "fluid_op_set_bnd": [_ctx, _i, _i],
    "fluid_op_add_source": [_ctx, _i, _i, _f],
    "fluid_op_jacobi_sweep": [_ctx, _i, _i, _i, _i, _f, _f],
    "fluid_op_diffuse": [_ctx, _i, _i, _i, _f, _f, _i],
    "fluid_op_advect": [_ctx, _i, _i, _i, _i, _i, _f],
    "fluid_op_divergence": [_ctx, _i, _i, _i, _i],
    "fluid_op_subtract_gradient": [_ctx, _i, _i, _i],
    "fluid_residual": [_ctx, _i, _i, _f, _f, C.POINTER(_f)],
    "fluid_absmax_velocity": [_ctx, _i, _i, C.POINTER(_f)],
    "fluid_residual_members": [_ctx, _i, _i, _MF, _MF, _MF],
    "fluid_absmax_velocity_members": [_ctx, _i, _i, _MF],
    "fluid_member_moments": [_ctx, _i, C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "fluid_ensemble_stats": [_ctx, _i, _MF, _MF],
    "fluid_ensemble_stats_ptr": [_ctx, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)],
    "fluid_member_gram": [_ctx, _i, _i, C.POINTER(C.c_double)],
    "fluid_pack_members": [_ctx, _i, _i, _i, C.c_void_p, C.c_size_t],
    "fluid_unpack_members": [_ctx, _i, _i, _i, C.c_void_p, C.c_size_t],
    "fluid_download_members": [_ctx, _i, _MF],
    "fluid_upload_members": [_ctx, _i, _MF],
    "fluid_run": [_ctx, _f, _f, _f, C.POINTER(RunPlan), C.POINTER(_i)],
    "fluid_run_members": [_ctx, _MF, _MF, _MF, C.POINTER(RunPlan), C.POINTER(_i)],
    "fluid_coarse_size": [_i, _i, C.POINTER(_i)],
    "fluid_pack_members_coarse": [_ctx, _i, _i, _i, _i, C.c_void_p, C.c_size_t],
    "fluid_download_members_coarse": [_ctx, _i, _i, _MF],
    "fluid_run_coarse": [_ctx, _f, _f, _f, C.POINTER(RunPlan), _i, C.POINTER(_i)],
    "fluid_run_members_coarse": [_ctx, _MF, _MF, _MF, C.POINTER(RunPlan), _i, C.POINTER(_i)],
    "fluid_transform_members": [_ctx, C.POINTER(_i), _i, _MF],
    "fluid_select_members": [_ctx, C.POINTER(_i), _i, C.POINTER(_i)],
    "fluid_set_observation_points": [_ctx, _MF, _MF, _i],
    "fluid_observation_points": [_ctx, C.POINTER(_i)],
    "fluid_observe_members": [_ctx, _i, C.c_void_p, C.c_size_t],
    "fluid_observe_members_host": [_ctx, _i, _MF],
    "fluid_observation_gram": [_ctx, _i, _i, _MF, _MF, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "fluid_set_observation_network": [_ctx, _MF, _MF, C.POINTER(_i), _i],
    "fluid_observation_network_fields": [_ctx, C.POINTER(C.c_uint)],
    "fluid_transform_members_local": [_ctx, C.POINTER(_i), _i, _MF, C.c_void_p, C.POINTER(_i)],
    "fluid_transform_members_lattice": [_ctx, C.POINTER(_i), _i, _MF, _i, _i, _i, _i, _i],
    "fluid_taper_gaspari_cohn": [_ctx, _f, _f, _f, C.c_void_p, C.POINTER(_i)],
    "fluid_observation_gram_lattice": [_ctx, _i, _i, _MF, _MF, _i, _i, _i, _i, _i, _f, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), C.POINTER(_i)],
    "fluid_etkf_increments": [_ctx, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i), _f, _MF, C.POINTER(_i)],
    "fluid_analyse_lattice": [_ctx, _i, _MF, _MF, _i, _i, _i, _i, _i, _f, _f, C.POINTER(_i), _i],
    "fluid_analyse_lattice_status": [_ctx, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)],
    "fluid_member_spread": [_ctx, C.POINTER(_i), _i, C.c_void_p, C.c_size_t],
    "fluid_relax_spread": [_ctx, C.POINTER(_i), _i, C.c_void_p, C.c_size_t, _f],
    "fluid_noise_members": [_ctx, C.POINTER(_i), _i, _i, _MF, C.c_ulonglong, C.c_uint, _i],
    "fluid_noise_dense": [_ctx, C.c_void_p, C.c_size_t, _f, C.c_ulonglong, C.c_uint, _i],
    "fluid_noise_value": [C.c_ulonglong, C.c_uint, _i, _i, C.c_uint, C.c_uint, C.POINTER(C.c_double)],
    "fluid_observe_members_range": [_ctx, _i, _i, _i, C.c_void_p, C.c_size_t],
    "fluid_run_window": [_ctx, _MF, _MF, _MF, C.POINTER(RunPlan), _i, C.POINTER(ObsWindow), C.POINTER(_i)],
    "fluid_observation_gram_recorded": [_ctx, C.c_void_p, C.c_size_t, _i, _MF, _MF, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double)],
    "fluid_observation_gram_lattice_recorded": [_ctx, C.c_void_p, C.c_size_t, _i, _MF, _MF, _i, _i, _i, _i, _i, _f,
                                                C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i)],
    "fluid_analyse_lattice_recorded": [_ctx, C.c_void_p, C.c_size_t, _MF, _MF, _i, _i, _i, _i, _i, _f, _f, C.POINTER(_i), _i],
    "fluid_observation_departures": [_ctx, _i, _MF, _MF, _f, _MF, _MF, _MF, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte),
                                     C.POINTER(C.c_double)],
    "fluid_observation_departures_recorded": [_ctx, C.c_void_p, C.c_size_t, _MF, _MF, _f, _MF, _MF, _MF, C.POINTER(C.c_ubyte),
                                              C.POINTER(C.c_ubyte), C.POINTER(C.c_double)],
    "fluid_set_observation_qc": [_ctx, _f],
    "fluid_observation_qc": [_ctx, _MF],
    "fluid_observation_qc_result": [_ctx, C.POINTER(C.c_ubyte), C.POINTER(_i), C.POINTER(_i)],
    "fluid_verify_members": [_ctx, C.POINTER(_i), _i, C.c_void_p, C.c_size_t, C.POINTER(_i), _i, C.c_void_p, C.c_void_p],
    "fluid_quantile_position": [_i, _f, C.POINTER(_i), C.POINTER(C.c_double)],
    "fluid_member_quantiles": [_ctx, _i, _MF, _i, C.c_void_p, C.c_size_t],
    "fluid_member_exceedance": [_ctx, _i, _MF, _i, _i, C.c_void_p, C.c_size_t],
    "fluid_set_jacobi_variant": [_ctx, _i],
    "fluid_division_mode": [_ctx, _f, _f, C.POINTER(_i)],
    "fluid_autotune_pending": [_ctx, C.POINTER(_i)],
    "fluid_plan_sweeps": [_i, _i, _i, _i, _i, _i, _i, C.POINTER(_i), _i, C.POINTER(_i)],
    "fluid_set_param": [_ctx, _i, _i],
    "fluid_timing_enable": [_ctx, _i],
    "fluid_timing_read": [_ctx, C.POINTER(Timing), _i],
    "fluid_op_diffuse_tol": [_ctx, _i, _i, _i, _f, _f, _f, _i, _i, C.POINTER(_i), C.POINTER(_f)],
    "fluid_set_exchange": [_ctx, EXCHANGE_FN, C.c_void_p],
    "fluid_exchange_now": [_ctx, _i, C.POINTER(_i), _i, _i],
    "fluid_exchange_stream": [_ctx, C.POINTER(C.c_void_p)],
    "fluid_split_launches": [_ctx, C.POINTER(C.c_longlong)],
    "fluid_rccl_available": [],
    "fluid_rccl_unique_id": [C.c_void_p, C.c_size_t],
    "fluid_exchange_rccl_attach": [_ctx, C.c_void_p, C.c_size_t],
    "fluid_exchange_rccl_attach_comm": [_ctx, C.c_void_p],
    "fluid_exchange_rccl_detach": [_ctx],
    "fluid_exchange_rccl_calls": [_ctx, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)],
}
# symbols with a non-status return type
OTHER_SYMBOLS = {"fluid_last_error": (C.c_char_p, []), "fluid_arena_bytes": (C.c_size_t, [_i]),
                 "fluid_arena_bytes_ex": (C.c_size_t, [_i, _i]),
                 "fluid_arena_bytes_ensemble": (C.c_size_t, [_i, _i, _i])}
MAX_MEMBERS = 21845
COARSE_FACTORS = (1, 2, 4, 8, 16, 32, 64)
TRANSFORM_MAX_MEMBERS = 64
OBSERVE_MAX_POINTS = 1 << 20
FIELD_OF_POINT = -2                  # FLUID_FIELD_OF_POINT: every point of a typed network observes its own field
LATTICE_MAX_NODES = 4096
LATTICE_GRAM_MAX_ENTRIES = 1 << 24
ETKF_MAX_SWEEPS = 28
ETKF_SOLVED, ETKF_EMPTY, ETKF_FAILED = 0, 1, 2
NOISE_SET, NOISE_ADD = 0, 1
NOISE_DENSE_TAG = 15                 # the counter tag of fluid_noise_dense: no field id
NOISE_IDS = 65536                    # member ids and stream ids lie below it
WINDOW_MAX_SLOTS = 65536             # FLUID_WINDOW_MAX_SLOTS: slots of one fluid_run_window
VERIFY_SUMS = 5                      # FLUID_VERIFY_SUMS: count, then the sums of e, se, var and crps
VERIFY_ROW = VERIFY_SUMS + TRANSFORM_MAX_MEMBERS + 1      # FLUID_VERIFY_ROW: doubles per field of a score row
VERIFY_FAIR = 1                      # FLUID_VERIFY_FAIR
QUANTILE_MAX_LEVELS = 16             # FLUID_QUANTILE_MAX_LEVELS: levels of one quantiles call, thresholds of one exceedance call
EXCEED_ABOVE, EXCEED_BELOW = 0, 1

_lib = None


def lib():
    """The loaded library; raises if libfluid_amd.so has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise ImportError("%s not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB)
        try:
            # torch wheels bundle their own libamdhip64/libhsa-runtime64; two HIP
            # runtimes in one process cannot both own the GPU.  Loading torch
            # first makes our DT_NEEDED libamdhip64.so.7 resolve to that copy.
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB)
        for name, args in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = C.c_int, args
        for name, (res, args) in OTHER_SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def check(rc):
    if rc != OK:
        raise FluidError(rc, lib().fluid_last_error().decode(errors="replace"))
