"""CPU: the ABI of typed observation networks -- fluid_set_observation_network, fluid_observation_network_fields and the sentinel
FLUID_FIELD_OF_POINT (include/fluid_amd.h, "typed networks").  Without a device only the refusals that come before the context
is looked at can be exercised: each call names itself when it refuses a null context, and a null required pointer is found
first.  tests/test_abi.py holds the header, the exports and the bindings together; this file holds the two declarations against
the binding type by type, the sentinel's value, and the words the section's contract rests on."""
import ctypes as C
import inspect
import re

from conftest import ROOT

NAMES = ("fluid_set_observation_network", "fluid_observation_network_fields")
ARGS = {
    "fluid_set_observation_network": ["ctx", "col", "row", "field", "npoints"],
    "fluid_observation_network_fields": ["ctx", "mask"],
}
FIVE = ("fluid_observe_members", "fluid_observe_members_host", "fluid_observation_gram", "fluid_observation_gram_lattice",
        "fluid_analyse_lattice")


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
    return msg


def header_text():
    src = open(ROOT + "/include/fluid_amd.h").read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_exports_and_binding_agree():
    capi, L = lib()
    ctype = {"fluid_ctx*": C.c_void_p, "int": C.c_int, "const int*": C.POINTER(C.c_int), "const float*": C.POINTER(C.c_float),
             "unsigned*": C.POINTER(C.c_uint)}
    _, src = header_text()
    for name in NAMES:
        assert hasattr(L, name), "%s is declared but not exported" % name
        m = re.search(r"^int\s+%s\s*\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, name
        want, names = [], []
        for d in m.group(1).split(","):
            d = " ".join(d.split())
            t = re.match(r"(.*?)(\*?)\s*(\w+)$", d)           # type, star, name
            want.append(ctype[(t.group(1).strip() + t.group(2)).replace(" *", "*")])
            names.append(t.group(3))
        assert names == ARGS[name], (name, names)
        assert capi.SIGNATURES[name] == want, (name, capi.SIGNATURES[name], want)


def test_the_sentinel_is_the_headers():
    capi, _ = lib()
    _, src = header_text()
    m = re.search(r"^#define\s+FLUID_FIELD_OF_POINT\s+\((-?\d+)\)", src, flags=re.M)
    assert m and capi.FIELD_OF_POINT == int(m.group(1)) == -2
    assert not 0 <= capi.FIELD_OF_POINT < len(capi.FIELD_NAMES) and capi.FIELD_OF_POINT != -1      # -1 stays a bad field id


def test_the_section_says_what_the_contract_rests_on():
    raw, _ = header_text()
    start = raw.index("typed networks: observation points that each observe their own field")
    assert start > raw.index("#define FLUID_OBSERVE_MAX_POINTS"), "the section comes after `observing ensembles`"
    section = raw[start:raw.index("#define FLUID_FIELD_OF_POINT", start)]
    section = " ".join(section.replace(" * ", " ").split())
    for word in ("FLUID_FIELD_OF_POINT", "typed", "untyped", "fluid_pack_members", "field[p]", "[0, FLUID_NFIELDS)", "33 bytes per point",
                 "that field's OWN scale", "Everything after rule 1 is untouched", "The order of every addition is unchanged",
                 "fixed by the point index", "not touched", "fluid_set_observation_points", "row slabs", "bad field id", "typed network is needed",
                 "without any per-point lookup", "poisons row k, column k and rhs[k] only") + FIVE:
        assert word in section, word


def test_null_pointers_are_found_before_the_context_is_looked_at():
    capi, L = lib()
    one = (C.c_float * 1)(1.5)
    ids = (C.c_int * 1)(2)
    cases = [
        (lambda: L.fluid_set_observation_network(None, None, one, ids, 1), b"fluid_set_observation_network", b"col"),
        (lambda: L.fluid_set_observation_network(None, one, None, ids, 1), b"fluid_set_observation_network", b"row"),
        (lambda: L.fluid_set_observation_network(None, None, one, None, 1), b"fluid_set_observation_network", b"col"),
        (lambda: L.fluid_observation_network_fields(None, None), b"fluid_observation_network_fields", b"mask"),
    ]
    for call, name, pointer in cases:
        msg = refused(L, capi, call(), name, pointer)
        assert b"context" not in msg, msg
    assert one[0] == 1.5 and ids[0] == 2


def test_null_context_is_refused_by_name():
    capi, L = lib()
    one = (C.c_float * 1)(1.5)
    ids = (C.c_int * 1)(2)
    mask = C.c_uint(77)
    g = (C.c_double * 1)(7.0)
    dev = C.c_void_p(64)                    # never dereferenced: the context is refused first
    fop = capi.FIELD_OF_POINT
    for call, name in [
        (lambda: L.fluid_set_observation_network(None, one, one, ids, 1), b"fluid_set_observation_network"),
        (lambda: L.fluid_set_observation_network(None, one, one, None, 1), b"fluid_set_observation_network"),
        (lambda: L.fluid_set_observation_network(None, None, None, None, 0), b"fluid_set_observation_network"),
        (lambda: L.fluid_observation_network_fields(None, C.byref(mask)), b"fluid_observation_network_fields"),
        (lambda: L.fluid_observe_members(None, fop, dev, 0), b"fluid_observe_members"),
        (lambda: L.fluid_observe_members_host(None, fop, one), b"fluid_observe_members_host"),
        (lambda: L.fluid_observation_gram(None, fop, 1, one, one, g, g, g), b"fluid_observation_gram"),
    ]:
        refused(L, capi, call(), name, b"null context")
    assert one[0] == 1.5 and ids[0] == 2 and mask.value == 77 and g[0] == 7.0


def test_solver_has_the_network_methods():
    from fluidsimulationcuda_amd import FluidSolver, solver
    p = inspect.signature(FluidSolver.set_observation_network).parameters
    assert list(p) == ["self", "cols", "rows", "fields"] and p["fields"].default is None
    assert list(inspect.signature(FluidSolver.observation_fields).parameters) == ["self"]
    for name in ("observe", "observe_device", "observation_gram"):
        assert inspect.signature(getattr(FluidSolver, name)).parameters["field"].default is None, name
    from fluidsimulationcuda_amd import capi
    assert solver._ofid(None) == solver._ofid("point") == capi.FIELD_OF_POINT
    assert solver._ofid("dens") == 2 and solver._ofid(7) == 7
    assert "typed networks" in FluidSolver.set_observation_network.__doc__
