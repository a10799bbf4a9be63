"""CPU: the ABI of recombining ensembles -- fluid_transform_members, fluid_select_members (include/fluid_amd.h,
"recombining ensembles").  Without a device only the refusals that come before the context is looked at can be exercised:
both calls name themselves when they refuse a null context, and null pointers are found first.  tests/test_abi.py holds
the header, the exports and the bindings together."""
import ctypes as C
import inspect
import re

from conftest import ROOT

NEW = ("fluid_transform_members", "fluid_select_members")


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
    ids = (C.c_int * 1)(0)
    one = (C.c_float * 1)(1.0)
    src = (C.c_int * 1)(0)
    refused(L, capi, L.fluid_transform_members(None, ids, 1, one), b"fluid_transform_members", b"null context")
    refused(L, capi, L.fluid_select_members(None, ids, 1, src), b"fluid_select_members", b"null context")


def test_null_pointers_are_found_before_the_context_is_looked_at():
    capi, L = lib()
    ids = (C.c_int * 1)(0)
    one = (C.c_float * 1)(1.0)
    src = (C.c_int * 1)(0)
    refused(L, capi, L.fluid_transform_members(None, None, 1, one), b"fluid_transform_members", b"fields")
    refused(L, capi, L.fluid_transform_members(None, ids, 1, None), b"fluid_transform_members", b"weights")
    refused(L, capi, L.fluid_select_members(None, None, 1, src), b"fluid_select_members", b"fields")
    refused(L, capi, L.fluid_select_members(None, ids, 1, None), b"fluid_select_members", b"source")


def header_text():
    src = open(ROOT + "/include/fluid_amd.h").read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_signatures_carry_the_headers_types():
    capi, _ = lib()
    ctype = {"fluid_ctx*": C.c_void_p, "int": C.c_int, "const float*": capi._MF, "const int*": C.POINTER(C.c_int)}
    _, src = header_text()
    for name in NEW:
        m = re.search(r"^int\s+%s\s*\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, name
        want = []
        for d in m.group(1).split(","):
            d = " ".join(d.split())
            t = re.match(r"(.*?)(\*?)\s*(\w+)$", d)           # type, star, name
            want.append(ctype[(t.group(1).strip() + t.group(2)).replace(" *", "*")])
        assert capi.SIGNATURES[name] == want, (name, capi.SIGNATURES[name], want)


def test_the_cap_is_the_headers():
    capi, _ = lib()
    raw, src = header_text()
    m = re.search(r"^#define\s+FLUID_TRANSFORM_MAX_MEMBERS\s+(\d+)\s*$", src, flags=re.M)
    assert m and int(m.group(1)) == 64
    assert capi.TRANSFORM_MAX_MEMBERS == 64 == int(m.group(1))
    assert "recombining ensembles" in raw


def test_solver_has_transform_and_select():
    from fluidsimulationcuda_amd import FluidSolver
    for name, first in (("transform", "weights"), ("select", "source")):
        p = inspect.signature(getattr(FluidSolver, name)).parameters
        assert list(p) == ["self", first, "fields"], (name, list(p))
        assert p[first].default is inspect.Parameter.empty
        assert p["fields"].default == ("u", "v", "dens"), name
