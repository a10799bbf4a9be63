"""CPU: the ABI of the ensemble Gram matrix -- fluid_member_gram (include/fluid_amd.h, "ensemble diagnostics").  Without a
device only the refusals that come before the context is looked at can be exercised: the call names itself when it refuses
a null context, and a null `gram` is found first.  tests/test_abi.py holds the header, the exports and the bindings
together."""
import ctypes as C
import inspect
import re

from conftest import ROOT

NAME = "fluid_member_gram"


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


def test_null_gram_is_found_before_the_context_is_looked_at():
    capi, L = lib()
    for centre in (0, 1):
        refused(L, capi, L.fluid_member_gram(None, 0, centre, None), b"fluid_member_gram", b"gram")
        assert b"context" not in L.fluid_last_error()


def test_null_context_is_refused_by_name():
    capi, L = lib()
    one = (C.c_double * 1)(7.0)
    for centre in (0, 1):
        refused(L, capi, L.fluid_member_gram(None, 0, centre, one), b"fluid_member_gram", b"null context")
    assert one[0] == 7.0


def header_text():
    src = open(ROOT + "/include/fluid_amd.h").read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_signature_carries_the_headers_types():
    capi, _ = lib()
    ctype = {"fluid_ctx*": C.c_void_p, "int": C.c_int, "double*": C.POINTER(C.c_double)}
    _, src = header_text()
    m = re.search(r"^int\s+%s\s*\((.*?)\);" % NAME, src, flags=re.S | re.M)
    assert m, NAME
    want, names = [], []
    for d in m.group(1).split(","):
        d = " ".join(d.split())
        t = re.match(r"(.*?)(\*?)\s*(\w+)$", d)           # type, star, name
        want.append(ctype[(t.group(1).strip() + t.group(2)).replace(" *", "*")])
        names.append(t.group(3))
    assert names == ["ctx", "field", "centre", "gram"]
    assert capi.SIGNATURES[NAME] == want, (capi.SIGNATURES[NAME], want)


def test_the_header_section_names_the_cap():
    capi, _ = lib()
    raw, src = header_text()
    # the declaration sits in the section "ensemble diagnostics", behind fluid_ensemble_stats_ptr
    assert re.search(r"^int\s+fluid_ensemble_stats_ptr\s*\([^;]*\);\s*^int\s+fluid_member_gram\s*\(", src, flags=re.S | re.M)
    start = raw.index("ensemble diagnostics")
    section = raw[start:raw.index("int fluid_residual_members", start)]
    at = section.index("- fluid_member_gram:")
    entry = section[at:section.index("\n * - ", at + 1)]
    assert "FLUID_TRANSFORM_MAX_MEMBERS" in entry
    for word in ("fluid_pack_members", "fluid_ensemble_stats", "member order", "interior", "atomics", "mirrored", "EVERY entry"):
        assert word in entry, word
    assert capi.TRANSFORM_MAX_MEMBERS == 64


def test_solver_has_member_gram():
    from fluidsimulationcuda_amd import FluidSolver
    p = inspect.signature(FluidSolver.member_gram).parameters
    assert list(p) == ["self", "field", "centre"]
    assert p["centre"].default is False
    assert "ensemble diagnostics" in FluidSolver.member_gram.__doc__
