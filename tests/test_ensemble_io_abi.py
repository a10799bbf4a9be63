"""CPU: the ABI of moving whole ensembles -- fluid_pack_members / fluid_unpack_members, fluid_download_members /
fluid_upload_members, fluid_run / fluid_run_members (include/fluid_amd.h, "moving ensembles").  Without a device only the
refusals that come before the context is looked at can be exercised: every call names itself when it refuses a null
context, and null pointers are found first.  tests/test_abi.py holds the header, the exports and the bindings together."""
import ctypes as C
import re

import numpy as np

from conftest import ROOT

NEW = ("fluid_pack_members", "fluid_unpack_members", "fluid_download_members", "fluid_upload_members", "fluid_run",
       "fluid_run_members")


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


def test_null_context_is_refused_by_name():
    capi, L = lib()
    host = np.zeros(16, np.float32).ctypes.data_as(capi._MF)
    plan = capi.RunPlan(iters=4, nsteps=1)
    one = (C.c_float * 1)(0.5)
    n = C.c_int(7)
    somewhere = C.c_void_p(4096)        # never dereferenced: there is no context to run on
    refused(L, capi, L.fluid_pack_members(None, 0, 0, 0, somewhere, 0), b"fluid_pack_members", b"null context")
    refused(L, capi, L.fluid_unpack_members(None, 0, 0, 0, somewhere, 0), b"fluid_unpack_members", b"null context")
    refused(L, capi, L.fluid_download_members(None, 0, host), b"fluid_download_members", b"null context")
    refused(L, capi, L.fluid_upload_members(None, 0, host), b"fluid_upload_members", b"null context")
    refused(L, capi, L.fluid_run(None, 0.1, 0.1, 0.1, C.byref(plan), C.byref(n)), b"fluid_run", b"null context")
    refused(L, capi, L.fluid_run_members(None, one, one, one, C.byref(plan), C.byref(n)), b"fluid_run_members", b"null context")
    assert n.value == 7


def test_null_pointers_are_found_before_the_context_is_looked_at():
    capi, L = lib()
    plan = capi.RunPlan(iters=4, nsteps=1)
    one = (C.c_float * 1)(0.5)
    refused(L, capi, L.fluid_pack_members(None, 0, 0, 0, None, 0), b"fluid_pack_members", b"dst_dev")
    refused(L, capi, L.fluid_unpack_members(None, 0, 0, 0, None, 0), b"fluid_unpack_members", b"src_dev")
    refused(L, capi, L.fluid_download_members(None, 0, None), b"fluid_download_members", b"null host pointer")
    refused(L, capi, L.fluid_upload_members(None, 0, None), b"fluid_upload_members", b"null host pointer")
    refused(L, capi, L.fluid_run(None, 0.1, 0.1, 0.1, None, None), b"fluid_run", b"null plan")
    refused(L, capi, L.fluid_run_members(None, one, one, one, None, None), b"fluid_run_members", b"null plan")
    for k, name in enumerate((b"dt", b"diff", b"visc")):
        args = [one, one, one]
        args[k] = None
        refused(L, capi, L.fluid_run_members(None, *args, C.byref(plan), None), b"fluid_run_members", name)


def header_text():
    src = open(ROOT + "/include/fluid_amd.h").read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_signatures_carry_the_headers_types():
    capi, _ = lib()
    ctype = {"fluid_ctx*": C.c_void_p, "int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "void*": C.c_void_p,
             "const void*": C.c_void_p, "float*": capi._MF, "const float*": capi._MF, "int*": C.POINTER(C.c_int),
             "const int*": C.POINTER(C.c_int), "const fluid_run_plan*": C.POINTER(capi.RunPlan)}

    def types_of(decls):
        out = []
        for d in decls:
            d = " ".join(d.split())
            m = re.match(r"(.*?)(\*?)\s*(\w+)$", d)           # type, star, name
            out.append((m.group(3), ctype[(m.group(1).strip() + m.group(2)).replace(" *", "*")]))
        return out

    src = header_text()
    for name in NEW:
        m = re.search(r"^int\s+%s\s*\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, name
        want = [t for _, t in types_of(m.group(1).split(","))]
        assert capi.SIGNATURES[name] == want, (name, capi.SIGNATURES[name], want)
    # the plan: the header's members in the header's order
    body = re.search(r"typedef struct fluid_run_plan \{(.*?)\} fluid_run_plan;", src, flags=re.S).group(1)
    members = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        first, *more = [p.strip() for p in stmt.split(",")]
        (name, t), = types_of([first])
        members.append((name, t))
        members += [(p, t) for p in more]          # `int a, b, c`
    assert [(n, t) for n, t in capi.RunPlan._fields_] == members


def test_solver_has_the_new_methods_and_needs_no_torch_at_import():
    import subprocess
    import sys
    from fluidsimulationcuda_amd import FluidSolver
    for name in ("pack", "unpack", "run", "upload_members", "download_members"):
        assert callable(getattr(FluidSolver, name))
    code = ("import sys; sys.modules['torch'] = None\n"          # any `import torch` now raises ImportError
            "import fluidsimulationcuda_amd.solver as s\n"
            "assert s.device_address(4096) == 4096 and hasattr(s.FluidSolver, 'run')\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
