"""CPU: the ABI of observing ensembles -- fluid_set_observation_points, fluid_observation_points, fluid_observe_members,
fluid_observe_members_host, fluid_observation_gram (include/fluid_amd.h, "observing ensembles").  Without a device only the
refusals that come before the context is looked at can be exercised: every call names itself when it refuses a null
context, and a null required pointer is found first.  tests/test_abi.py holds the header, the exports and the bindings
together; this file holds the five declarations against the binding type by type."""
import ctypes as C
import inspect
import re

from conftest import ROOT

NAMES = ("fluid_set_observation_points", "fluid_observation_points", "fluid_observe_members", "fluid_observe_members_host",
         "fluid_observation_gram")
ARGS = {
    "fluid_set_observation_points": ["ctx", "col", "row", "npoints"],
    "fluid_observation_points": ["ctx", "npoints"],
    "fluid_observe_members": ["ctx", "field", "out_dev", "member_stride"],
    "fluid_observe_members_host": ["ctx", "field", "host"],
    "fluid_observation_gram": ["ctx", "field", "centre", "obs", "inv_sigma", "gram", "rhs", "dd"],
}


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
    ctype = {"fluid_ctx*": C.c_void_p, "int": C.c_int, "int*": C.POINTER(C.c_int), "double*": C.POINTER(C.c_double),
             "const float*": C.POINTER(C.c_float), "float*": C.POINTER(C.c_float), "void*": C.c_void_p, "size_t": C.c_size_t}
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


def test_the_cap_on_points_is_the_headers():
    capi, _ = lib()
    raw, src = header_text()
    m = re.search(r"^#define\s+FLUID_OBSERVE_MAX_POINTS\s+\(1 << (\d+)\)", src, flags=re.M)
    assert m and capi.OBSERVE_MAX_POINTS == 1 << int(m.group(1)) == 1 << 20
    start = raw.index("observing ensembles")
    section = raw[start:raw.index("#define FLUID_OBSERVE_MAX_POINTS", start)]
    for word in ("fluid_pack_members", "FluidSequential.c:120-123", "[0.5, N + 0.5]", "fluid_ensemble_stats", "atomics", "bit-symmetric",
                 "FLUID_TRANSFORM_MAX_MEMBERS", "row slabs", "fluid_timing"):
        assert word in section, word


def test_null_pointers_are_found_before_the_context_is_looked_at():
    capi, L = lib()
    one = (C.c_float * 1)(1.5)
    g = (C.c_double * 1)(7.0)
    cases = [
        (lambda: L.fluid_set_observation_points(None, None, one, 1), b"fluid_set_observation_points", b"col"),
        (lambda: L.fluid_set_observation_points(None, one, None, 1), b"fluid_set_observation_points", b"row"),
        (lambda: L.fluid_observation_points(None, None), b"fluid_observation_points", b"npoints"),
        (lambda: L.fluid_observe_members(None, 0, None, 0), b"fluid_observe_members", b"out_dev"),
        (lambda: L.fluid_observe_members_host(None, 0, None), b"fluid_observe_members_host", b"host"),
        (lambda: L.fluid_observation_gram(None, 0, 1, None, None, None, None, None), b"fluid_observation_gram", b"gram"),
    ]
    for call, name, pointer in cases:
        msg = refused(L, capi, call(), name, pointer)
        assert b"context" not in msg, msg
    assert one[0] == 1.5 and g[0] == 7.0


def test_null_context_is_refused_by_name():
    capi, L = lib()
    one = (C.c_float * 1)(1.5)
    n = C.c_int(7)
    g = (C.c_double * 1)(7.0)
    dev = C.c_void_p(64)                    # never dereferenced: the context is refused first
    for call, name in [
        (lambda: L.fluid_set_observation_points(None, one, one, 1), b"fluid_set_observation_points"),
        (lambda: L.fluid_set_observation_points(None, None, None, 0), b"fluid_set_observation_points"),
        (lambda: L.fluid_observation_points(None, C.byref(n)), b"fluid_observation_points"),
        (lambda: L.fluid_observe_members(None, 0, dev, 0), b"fluid_observe_members"),
        (lambda: L.fluid_observe_members_host(None, 0, one), b"fluid_observe_members_host"),
        (lambda: L.fluid_observation_gram(None, 0, 0, None, None, g, None, None), b"fluid_observation_gram"),
        (lambda: L.fluid_observation_gram(None, 0, 1, one, one, g, g, g), b"fluid_observation_gram"),
    ]:
        refused(L, capi, call(), name, b"null context")
    assert one[0] == 1.5 and n.value == 7 and g[0] == 7.0


def test_rhs_or_dd_without_obs_is_refused():
    capi, L = lib()
    g, r, d = (C.c_double * 1)(7.0), (C.c_double * 1)(7.0), (C.c_double * 1)(7.0)
    msg = refused(L, capi, L.fluid_observation_gram(None, 0, 1, None, None, g, r, None), b"fluid_observation_gram", b"rhs", b"obs")
    assert b"context" not in msg
    refused(L, capi, L.fluid_observation_gram(None, 0, 0, None, None, g, None, d), b"fluid_observation_gram", b"dd", b"obs")
    assert g[0] == r[0] == d[0] == 7.0


def test_solver_has_the_observing_methods():
    from fluidsimulationcuda_amd import FluidSolver
    sig = {name: inspect.signature(getattr(FluidSolver, name)).parameters for name in
           ("set_observation_points", "observation_points", "observe", "observe_device", "observation_gram")}
    assert list(sig["set_observation_points"]) == ["self", "cols", "rows"]
    assert list(sig["observation_points"]) == ["self"]
    assert list(sig["observe"]) == ["self", "field"]
    assert list(sig["observe_device"]) == ["self", "field", "out", "member_stride", "wait"]
    assert sig["observe_device"]["out"].default is None and sig["observe_device"]["member_stride"].default == 0
    assert sig["observe_device"]["wait"].default is True
    assert list(sig["observation_gram"]) == ["self", "field", "obs", "inv_sigma", "centre"]
    assert sig["observation_gram"]["centre"].default is True and sig["observation_gram"]["obs"].default is None
    assert "observing ensembles" in FluidSolver.observation_gram.__doc__
