"""CPU: the ensemble entry points of include/fluid_amd.h that need no device -- the arena's size and every argument
error of fluid_create_ensemble (found before the device is touched, as fluid_create(-3) is).  The header <-> exports <->
binding comparison is test_abi.py's and covers the new functions through capi.SIGNATURES."""
import ctypes as C

import pytest

MAX_MEMBERS = 21845      # 3 solves x members <= 65535 blocks in z


def cfg_for(capi, n=30, nranks=1, rank=0, storage=0, variant=3):
    return capi.Config(n=n, rank=rank, nranks=nranks, halo=0, jacobi_variant=variant, stream=None, arena=None,
                       arena_bytes=0, storage=storage)


def test_arena_bytes_of_an_ensemble():
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    assert capi.MAX_MEMBERS == MAX_MEMBERS
    for n in (1, 254, 4094):
        ff = C.c_size_t()
        assert L.fluid_layout(n, None, None, C.byref(ff)) == capi.OK
        for storage, esz in ((capi.STORAGE_F32, 4), (capi.STORAGE_F16, 2)):
            assert L.fluid_arena_bytes_ensemble(n, storage, 1) == L.fluid_arena_bytes_ex(n, storage)
            for m in (1, 2, 3, 16, 64, MAX_MEMBERS):
                assert L.fluid_arena_bytes_ensemble(n, storage, m) == ff.value * esz * 12 * m + 256, (n, storage, m)
    assert L.fluid_arena_bytes_ensemble(30, 0, 1) == L.fluid_arena_bytes(30)
    for bad in ((0, 0, 2), (-1, 0, 2), (65534, 0, 2), (30, 2, 2), (30, -1, 2), (30, 0, 0), (30, 0, -4), (30, 0, MAX_MEMBERS + 1)):
        assert L.fluid_arena_bytes_ensemble(*bad) == 0, bad


@pytest.mark.parametrize("members, kw, needle", [
    (0, {}, b"members"),
    (-1, {}, b"members"),
    (MAX_MEMBERS + 1, {}, b"members"),
    (2, {"nranks": 2, "n": 64}, b"nranks"),
    (3, {"nranks": 4, "rank": 1, "n": 64}, b"nranks"),
    (2, {"n": 0}, b"N must be"),
    (2, {"storage": 7}, b"storage"),
    (2, {"variant": 9}, b"variant"),
])
def test_create_ensemble_argument_errors(members, kw, needle):
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    h = C.c_void_p(0x1234)
    cfg = cfg_for(capi, **kw)
    assert L.fluid_create_ensemble(C.byref(cfg), members, C.byref(h)) == capi.E_INVALID
    assert not h.value, "the handle must be left null"
    assert needle in L.fluid_last_error(), L.fluid_last_error()


def test_create_ensemble_null_pointers():
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    h = C.c_void_p()
    cfg = cfg_for(capi)
    assert L.fluid_create_ensemble(None, 2, C.byref(h)) == capi.E_INVALID and b"null" in L.fluid_last_error()
    assert L.fluid_create_ensemble(C.byref(cfg), 2, None) == capi.E_INVALID and b"null" in L.fluid_last_error()
    m = C.c_int()
    assert L.fluid_members(None, C.byref(m)) == capi.E_INVALID
    import numpy as np
    a = np.zeros((32, 32), np.float32)
    assert L.fluid_upload_member(None, 0, 0, a) == capi.E_INVALID
    assert L.fluid_download_member(None, 0, 0, a) == capi.E_INVALID


def test_valid_ensemble_without_a_gpu_fails_loudly():
    """as test_abi.test_no_gpu_means_loud_failure has it for fluid_create: no device, no context; with one, a context of that many members"""
    import torch
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    h = C.c_void_p()
    cfg = cfg_for(capi)
    for members in (1, 2, 16):
        rc = L.fluid_create_ensemble(C.byref(cfg), members, C.byref(h))
        if torch.cuda.is_available():
            m = C.c_int()
            assert rc == capi.OK and h.value and L.fluid_members(h, C.byref(m)) == capi.OK and m.value == members
            assert L.fluid_destroy(h) == capi.OK
        else:
            assert rc in (capi.E_HIP, capi.E_NOMEM) and not h.value


def test_python_surface():
    """FluidSolver grew `members` and the member calls (no context is made here)"""
    import inspect
    from fluidsimulationcuda_amd import FluidSolver
    assert "members" in inspect.signature(FluidSolver.__init__).parameters
    assert "member" in inspect.signature(FluidSolver.upload).parameters
    assert "member" in inspect.signature(FluidSolver.download).parameters
    assert hasattr(FluidSolver, "upload_members") and hasattr(FluidSolver, "download_members")
