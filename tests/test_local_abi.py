"""CPU: the ABI of localised updates -- fluid_transform_members_local, fluid_taper_gaspari_cohn (include/fluid_amd.h,
"localised updates").  Without a device only the refusals that come before the context is looked at can be exercised:
both calls name themselves when they refuse a null context, and null pointers are found first.  tests/test_abi.py holds
the header, the exports and the bindings together."""
import ctypes as C
import inspect
import re

from conftest import ROOT

NEW = ("fluid_transform_members_local", "fluid_taper_gaspari_cohn")


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
    box = (C.c_int * 4)()
    refused(L, capi, L.fluid_transform_members_local(None, ids, 1, one, None, None), b"fluid_transform_members_local", b"null context")
    refused(L, capi, L.fluid_transform_members_local(None, ids, 1, one, 256, box), b"fluid_transform_members_local", b"null context")
    refused(L, capi, L.fluid_taper_gaspari_cohn(None, 1.0, 1.0, 1.0, 256, box), b"fluid_taper_gaspari_cohn", b"null context")
    refused(L, capi, L.fluid_taper_gaspari_cohn(None, 1.0, 1.0, 1.0, 256, None), b"fluid_taper_gaspari_cohn", b"null context")


def test_null_pointers_are_found_before_the_context_is_looked_at():
    capi, L = lib()
    ids = (C.c_int * 1)(0)
    one = (C.c_float * 1)(1.0)
    refused(L, capi, L.fluid_transform_members_local(None, None, 1, one, None, None), b"fluid_transform_members_local", b"fields")
    refused(L, capi, L.fluid_transform_members_local(None, ids, 1, None, None, None), b"fluid_transform_members_local", b"increments")
    refused(L, capi, L.fluid_taper_gaspari_cohn(None, 1.0, 1.0, 1.0, None, None), b"fluid_taper_gaspari_cohn", b"out_dev")


def header_text():
    src = open(ROOT + "/include/fluid_amd.h").read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_signatures_carry_the_headers_types():
    capi, _ = lib()
    ctype = {"fluid_ctx*": C.c_void_p, "int": C.c_int, "float": C.c_float, "const float*": capi._MF,
             "const int*": C.POINTER(C.c_int), "int*": C.POINTER(C.c_int), "const void*": C.c_void_p, "void*": C.c_void_p}
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


def test_the_header_has_the_section_after_observing_ensembles():
    raw, _ = header_text()
    assert "localised updates" in raw
    assert raw.index("observing ensembles") < raw.index("localised updates")
    assert raw.index("localised updates") < raw.index("fluid_transform_members_local(fluid_ctx")


def test_solver_has_transform_local_and_taper():
    from fluidsimulationcuda_amd import FluidSolver
    p = inspect.signature(FluidSolver.transform_local).parameters
    assert list(p) == ["self", "increments", "taper", "box", "fields"], list(p)
    assert p["increments"].default is inspect.Parameter.empty
    assert p["taper"].default is None and p["box"].default is None
    assert p["fields"].default == ("u", "v", "dens")
    p = inspect.signature(FluidSolver.taper_gaspari_cohn).parameters
    assert list(p) == ["self", "col", "row", "c"], list(p)
    assert all(p[k].default is inspect.Parameter.empty for k in ("col", "row", "c"))
