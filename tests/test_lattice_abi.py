"""CPU: the ABI of lattice updates -- fluid_transform_members_lattice (include/fluid_amd.h, "lattice updates").  Without a
device only the refusals that come before the context is looked at can be exercised: the call names itself when it
refuses a null context, and null pointers are found first.  tests/test_abi.py holds the header, the exports and the
bindings together."""
import ctypes as C
import inspect
import re

from conftest import ROOT

NEW = ("fluid_transform_members_lattice",)


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
    refused(L, capi, L.fluid_transform_members_lattice(None, ids, 1, one, 1, 1, 0, 0, 8), b"fluid_transform_members_lattice", b"null context")
    refused(L, capi, L.fluid_transform_members_lattice(None, ids, 1, one, 0, -1, -5, 9, 7), b"fluid_transform_members_lattice", b"null context")


def test_null_pointers_are_found_before_the_context_is_looked_at():
    capi, L = lib()
    ids = (C.c_int * 1)(0)
    one = (C.c_float * 1)(1.0)
    refused(L, capi, L.fluid_transform_members_lattice(None, None, 1, one, 1, 1, 0, 0, 8), b"fluid_transform_members_lattice", b"fields")
    refused(L, capi, L.fluid_transform_members_lattice(None, ids, 1, None, 1, 1, 0, 0, 8), b"fluid_transform_members_lattice", b"increments")


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
        assert len(want) == 9


def test_the_header_has_the_section_after_localised_updates():
    raw, src = header_text()
    assert "lattice updates" in raw
    assert raw.index("localised updates") < raw.index("fluid_transform_members_local(fluid_ctx") < raw.index("lattice updates")
    assert raw.index("lattice updates") < raw.index("fluid_transform_members_lattice(fluid_ctx")
    m = re.search(r"^#define\s+FLUID_LATTICE_MAX_NODES\s+(\d+)\s*$", src, flags=re.M)
    assert m and int(m.group(1)) == 4096
    from fluidsimulationcuda_amd import capi
    assert capi.LATTICE_MAX_NODES == 4096


def test_solver_has_transform_lattice():
    from fluidsimulationcuda_amd import FluidSolver
    p = inspect.signature(FluidSolver.transform_lattice).parameters
    assert list(p) == ["self", "increments", "origin", "step", "fields"], list(p)
    assert all(p[k].default is inspect.Parameter.empty for k in ("increments", "origin", "step"))
    assert p["fields"].default == ("u", "v", "dens")
