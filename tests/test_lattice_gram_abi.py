"""CPU: the ABI of lattice observations -- fluid_observation_gram_lattice (include/fluid_amd.h, "lattice observations").
Without a device only the refusals that come before the context is looked at can be exercised: the call names itself when
it refuses a null context, and null pointers are found first.  tests/test_abi.py holds the header, the exports and the
bindings together."""
import ctypes as C
import inspect
import re

from conftest import ROOT

NEW = ("fluid_observation_gram_lattice",)


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
    gram = (C.c_double * 1)(7.0)
    refused(L, capi, L.fluid_observation_gram_lattice(None, 2, 1, None, None, 1, 1, 0, 0, 8, 1.0, gram, None, None, None),
            b"fluid_observation_gram_lattice", b"null context")
    refused(L, capi, L.fluid_observation_gram_lattice(None, -4, 0, None, None, 0, -1, -5, 9, 7, -1.0, gram, None, None, None),
            b"fluid_observation_gram_lattice", b"null context")
    assert gram[0] == 7.0


def test_null_pointers_are_found_before_the_context_is_looked_at():
    capi, L = lib()
    d = (C.c_double * 1)(7.0)
    one = (C.c_float * 1)(1.0)
    refused(L, capi, L.fluid_observation_gram_lattice(None, 2, 1, None, None, 1, 1, 0, 0, 8, 1.0, None, None, None, None),
            b"fluid_observation_gram_lattice", b"gram")
    refused(L, capi, L.fluid_observation_gram_lattice(None, 2, 1, None, None, 1, 1, 0, 0, 8, 1.0, d, d, None, None),
            b"fluid_observation_gram_lattice", b"rhs", b"obs")
    refused(L, capi, L.fluid_observation_gram_lattice(None, 2, 1, None, one, 1, 1, 0, 0, 8, 1.0, d, None, d, None),
            b"fluid_observation_gram_lattice", b"dd", b"obs")
    assert d[0] == 7.0


def header_text():
    src = open(ROOT + "/include/fluid_amd.h").read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_signatures_carry_the_headers_types():
    capi, _ = lib()
    ctype = {"fluid_ctx*": C.c_void_p, "int": C.c_int, "float": C.c_float, "const float*": capi._MF, "double*": C.POINTER(C.c_double),
             "int*": C.POINTER(C.c_int)}
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
        assert len(want) == 15


def test_the_header_has_the_section_after_lattice_updates():
    raw, src = header_text()
    assert "lattice observations" in raw
    assert raw.index("lattice updates") < raw.index("fluid_transform_members_lattice(fluid_ctx") < raw.index("lattice observations")
    assert raw.index("lattice observations") < raw.index("fluid_observation_gram_lattice(fluid_ctx") < raw.index("fluid_set_jacobi_variant(fluid_ctx")
    m = re.search(r"^#define\s+FLUID_LATTICE_GRAM_MAX_ENTRIES\s+\(1\s*<<\s*(\d+)\)\s*$", src, flags=re.M)
    assert m and int(m.group(1)) == 24
    from fluidsimulationcuda_amd import capi
    assert capi.LATTICE_GRAM_MAX_ENTRIES == 1 << 24


def test_solver_has_observation_gram_lattice():
    from fluidsimulationcuda_amd import FluidSolver
    p = inspect.signature(FluidSolver.observation_gram_lattice).parameters
    assert list(p) == ["self", "field", "shape", "origin", "step", "c", "obs", "inv_sigma", "centre"], list(p)
    assert all(p[k].default is inspect.Parameter.empty for k in ("field", "shape", "origin", "step", "c"))
    assert p["obs"].default is None and p["inv_sigma"].default is None and p["centre"].default is True
