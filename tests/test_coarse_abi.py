"""CPU: the ABI of the block-averaged ensemble snapshots -- fluid_coarse_size, fluid_pack_members_coarse,
fluid_download_members_coarse, fluid_run_coarse / fluid_run_members_coarse (include/fluid_amd.h, "coarse snapshots").
fluid_coarse_size is host logic and is checked in full; of the other five only the refusals that come before the context
is looked at can be exercised without a device: every call names itself when it refuses a null context, and null pointers
are found first.  tests/test_abi.py holds the header, the exports and the bindings together."""
import ctypes as C
import inspect
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

NEW = ("fluid_coarse_size", "fluid_pack_members_coarse", "fluid_download_members_coarse", "fluid_run_coarse",
       "fluid_run_members_coarse")
FACTORS = (1, 2, 4, 8, 16, 32, 64)


def lib():
    import __graft_entry__ as g
    g.build()
    from fluidsimulationcuda_amd import capi
    return capi, capi.lib()


def refused(L, capi, rc, *words):
    assert rc == capi.E_INVALID
    msg = L.fluid_last_error()
    for w in words:
        assert w in msg, msg


@pytest.mark.parametrize("n", [2, 6, 14, 62, 1022, 4094, 8190])
def test_coarse_size_values(n):
    capi, L = lib()
    from fluidsimulationcuda_amd import coarse_size
    assert capi.COARSE_FACTORS == FACTORS
    for r in FACTORS:
        side = C.c_int(-5)
        rc = L.fluid_coarse_size(n, r, C.byref(side))
        if (n + 2) % r == 0:
            assert rc == capi.OK and side.value == (n + 2) // r, (n, r, side.value)
            assert coarse_size(n, r) == (n + 2) // r
        else:       # (6 + 2 and 14 + 2 are too small for the larger factors)
            refused(L, capi, rc, b"fluid_coarse_size", b"N = %d" % n, b"factor %d" % r, b"divide")
            assert side.value == -5


def test_coarse_size_refusals():
    capi, L = lib()
    from fluidsimulationcuda_amd import coarse_size
    side = C.c_int(-5)
    for r in (0, 3, 128, -2):
        refused(L, capi, L.fluid_coarse_size(62, r, C.byref(side)), b"fluid_coarse_size", b"N = 62", b"factor %d" % r, b"one of 1, 2, 4")
        with pytest.raises(capi.FluidError):
            coarse_size(62, r)
    refused(L, capi, L.fluid_coarse_size(61, 2, C.byref(side)), b"fluid_coarse_size", b"N = 61", b"factor 2", b"divide N + 2 = 63")
    for n in (0, -1, -64):
        refused(L, capi, L.fluid_coarse_size(n, 1, C.byref(side)), b"fluid_coarse_size", b"N = %d" % n, b"factor 1", b"at least 1")
    refused(L, capi, L.fluid_coarse_size(62, 2, None), b"fluid_coarse_size", b"side")
    assert side.value == -5
    assert L.fluid_coarse_size(61, 1, C.byref(side)) == capi.OK and side.value == 63
    assert L.fluid_coarse_size(1, 1, C.byref(side)) == capi.OK and side.value == 3


def test_null_context_is_refused_by_name():
    capi, L = lib()
    host = np.zeros(16, np.float32).ctypes.data_as(capi._MF)
    plan = capi.RunPlan(iters=4, nsteps=1)
    one = (C.c_float * 1)(0.5)
    n = C.c_int(7)
    somewhere = C.c_void_p(4096)        # never dereferenced: there is no context to run on
    refused(L, capi, L.fluid_pack_members_coarse(None, 0, 0, 0, 2, somewhere, 0), b"fluid_pack_members_coarse", b"null context")
    refused(L, capi, L.fluid_download_members_coarse(None, 0, 2, host), b"fluid_download_members_coarse", b"null context")
    refused(L, capi, L.fluid_run_coarse(None, 0.1, 0.1, 0.1, C.byref(plan), 2, C.byref(n)), b"fluid_run_coarse", b"null context")
    refused(L, capi, L.fluid_run_members_coarse(None, one, one, one, C.byref(plan), 2, C.byref(n)), b"fluid_run_members_coarse", b"null context")
    assert n.value == 7


def test_null_pointers_are_found_before_the_context_is_looked_at():
    capi, L = lib()
    plan = capi.RunPlan(iters=4, nsteps=1)
    one = (C.c_float * 1)(0.5)
    refused(L, capi, L.fluid_pack_members_coarse(None, 0, 0, 0, 2, None, 0), b"fluid_pack_members_coarse", b"dst_dev")
    refused(L, capi, L.fluid_download_members_coarse(None, 0, 2, None), b"fluid_download_members_coarse", b"null host pointer")
    refused(L, capi, L.fluid_run_coarse(None, 0.1, 0.1, 0.1, None, 2, None), b"fluid_run_coarse", b"null plan")
    refused(L, capi, L.fluid_run_members_coarse(None, one, one, one, None, 2, None), b"fluid_run_members_coarse", b"null plan")
    for k, name in enumerate((b"dt", b"diff", b"visc")):
        args = [one, one, one]
        args[k] = None
        refused(L, capi, L.fluid_run_members_coarse(None, *args, C.byref(plan), 2, None), b"fluid_run_members_coarse", name)


def test_factor_zero_is_no_way_into_the_dense_calls():
    """inside the library factor 0 stands for the dense path: from outside it is refused like any other bad factor"""
    capi, L = lib()
    plan = capi.RunPlan(iters=4, nsteps=1)
    one = (C.c_float * 1)(0.5)
    host = np.zeros(16, np.float32).ctypes.data_as(capi._MF)
    somewhere = C.c_void_p(4096)
    refused(L, capi, L.fluid_pack_members_coarse(None, 0, 0, 0, 0, somewhere, 0), b"fluid_pack_members_coarse", b"factor 0")
    refused(L, capi, L.fluid_download_members_coarse(None, 0, 0, host), b"fluid_download_members_coarse", b"factor 0")
    refused(L, capi, L.fluid_run_coarse(None, 0.1, 0.1, 0.1, C.byref(plan), 0, None), b"fluid_run_coarse", b"factor 0")
    refused(L, capi, L.fluid_run_members_coarse(None, one, one, one, C.byref(plan), 0, None), b"fluid_run_members_coarse", b"factor 0")


def header_text():
    src = open(ROOT + "/include/fluid_amd.h").read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_signatures_carry_the_headers_types():
    capi, _ = lib()
    ctype = {"fluid_ctx*": C.c_void_p, "int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "void*": C.c_void_p,
             "const void*": C.c_void_p, "float*": capi._MF, "const float*": capi._MF, "int*": C.POINTER(C.c_int),
             "const int*": C.POINTER(C.c_int), "const fluid_run_plan*": C.POINTER(capi.RunPlan)}
    src = header_text()
    for name in NEW:
        m = re.search(r"^int\s+%s\s*\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, name
        want = []
        for d in m.group(1).split(","):
            d = " ".join(d.split())
            t = re.match(r"(.*?)(\*?)\s*(\w+)$", d)           # type, star, name
            want.append(ctype[(t.group(1).strip() + t.group(2)).replace(" *", "*")])
        assert capi.SIGNATURES[name] == want, (name, capi.SIGNATURES[name], want)


def test_solver_takes_coarse_and_needs_no_torch_at_import():
    from fluidsimulationcuda_amd import FluidSolver
    for name in ("pack", "download_members", "run"):
        p = inspect.signature(getattr(FluidSolver, name)).parameters
        assert "coarse" in p and p["coarse"].default is None, name
    code = ("import sys; sys.modules['torch'] = None\n"          # any `import torch` now raises ImportError
            "import fluidsimulationcuda_amd.solver as s\n"
            "assert s.coarse_size(62, 8) == 8 and s.coarse_size(61, 1) == 63\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
