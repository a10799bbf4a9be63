"""CPU: the ABI of asynchronous observations -- fluid_observe_members_range, fluid_run_window, the three recorded analysis calls,
fluid_obs_window and FLUID_WINDOW_MAX_SLOTS (include/fluid_amd.h, "asynchronous observations").  Without a device only the
refusals that come before the context is looked at can be exercised: a null required pointer is found first, and each call
names itself when it refuses a null context.  tests/test_abi.py holds the header, the exports and the bindings together; this
file holds the five declarations and the struct against the binding type by type, the words the section's contract rests on,
the solver's new methods, and the signatures of the methods the new ones stand beside."""
import ctypes as C
import inspect
import re

from conftest import ROOT

ARGS = {
    "fluid_observe_members_range": ["ctx", "field", "first", "count", "record_dev", "member_stride"],
    "fluid_run_window": ["ctx", "dt", "diff", "visc", "plan", "factor", "window", "snapshots_written"],
    "fluid_observation_gram_recorded": ["ctx", "record_dev", "member_stride", "centre", "obs", "inv_sigma", "gram", "rhs", "dd"],
    "fluid_observation_gram_lattice_recorded": ["ctx", "record_dev", "member_stride", "centre", "obs", "inv_sigma", "nodes_row",
                                                "nodes_col", "row0", "col0", "step", "c", "gram", "rhs", "dd", "counts"],
    "fluid_analyse_lattice_recorded": ["ctx", "record_dev", "member_stride", "obs", "inv_sigma", "nodes_row", "nodes_col", "row0",
                                       "col0", "step", "c", "rho", "fields", "nfields"],
}
NAMESAKE = {"fluid_observation_gram_recorded": "fluid_observation_gram",
            "fluid_observation_gram_lattice_recorded": "fluid_observation_gram_lattice",
            "fluid_analyse_lattice_recorded": "fluid_analyse_lattice"}


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


def ctypes_of(capi):
    return {"fluid_ctx*": C.c_void_p, "int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "void*": C.c_void_p,
            "const void*": C.c_void_p, "int*": C.POINTER(C.c_int), "const int*": C.POINTER(C.c_int),
            "const float*": C.POINTER(C.c_float), "double*": C.POINTER(C.c_double),
            "const fluid_run_plan*": C.POINTER(capi.RunPlan), "const fluid_obs_window*": C.POINTER(capi.ObsWindow)}


def declared(decls, ctype):
    """[(ctypes type, name)] of a comma- or semicolon-separated list of C declarations"""
    out = []
    for d in decls:
        d = " ".join(d.split())
        if not d:
            continue
        t = re.match(r"(.*?)(\*?)\s*(\w+)$", d)           # type, star, name
        out.append((ctype[(t.group(1).strip() + t.group(2)).replace(" *", "*")], t.group(3)))
    return out


def test_header_exports_and_binding_agree():
    capi, L = lib()
    _, src = header_text()
    ctype = ctypes_of(capi)
    for name, args in ARGS.items():
        assert hasattr(L, name), "%s is declared but not exported" % name
        m = re.search(r"^int\s+%s\s*\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, name
        got = declared(m.group(1).split(","), ctype)
        assert [n for _, n in got] == args, (name, got)
        assert capi.SIGNATURES[name] == [t for t, _ in got], (name, capi.SIGNATURES[name], got)


def test_a_recorded_call_is_its_namesake_with_the_record_for_the_field():
    capi, _ = lib()
    for name, namesake in NAMESAKE.items():
        assert ARGS[name][:3] == ["ctx", "record_dev", "member_stride"]
        want = list(capi.SIGNATURES[namesake])
        assert want[1] == C.c_int                                   # the field
        want[1:2] = [C.c_void_p, C.c_size_t]
        assert capi.SIGNATURES[name] == want, name
    run = list(capi.SIGNATURES["fluid_run_members_coarse"])         # (ctx, dt, diff, visc, plan, factor, written)
    run.insert(6, C.POINTER(capi.ObsWindow))
    assert capi.SIGNATURES["fluid_run_window"] == run
    assert capi.SIGNATURES["fluid_observe_members_range"] == [C.c_void_p, C.c_int, C.c_int, C.c_int] + capi.SIGNATURES["fluid_observe_members"][2:]


def test_the_window_struct_and_its_cap_are_the_headers():
    capi, _ = lib()
    _, src = header_text()
    m = re.search(r"typedef struct fluid_obs_window \{(.*?)\} fluid_obs_window;", src, flags=re.S)
    assert m
    ctype = ctypes_of(capi)
    got = declared(m.group(1).split(";"), ctype)
    assert [n for _, n in got] == ["field", "nslots", "slot_first", "slot_step", "record_dev", "member_stride"]
    assert [(n, t) for t, n in got] == list(capi.ObsWindow._fields_)
    m = re.search(r"^#define\s+FLUID_WINDOW_MAX_SLOTS\s+(\d+)", src, flags=re.M)
    assert m and capi.WINDOW_MAX_SLOTS == int(m.group(1)) == 65536


def test_the_section_says_what_the_contract_rests_on():
    raw, _ = header_text()
    start = raw.index("asynchronous observations: record H x during a run")
    assert start > raw.index("int fluid_noise_value("), "the section comes after `ensemble noise`"
    section = raw[start:raw.index("#define FLUID_WINDOW_MAX_SLOTS", start)]
    norm = lambda text: " ".join(text.replace(" * ", " ").split())        # the comment's own stars go; so do a product's
    section = norm(section)
    for word in ("4D-LETKF", "Hunt et al.", "RECORD", "record[m * member_stride + p] = h_m[p]", "member_stride = 0: P",
                 "(M - 1) * member_stride + P", "out_dev of fluid_observe_members", "Every other float of the record keeps its bits",
                 "count = 0 launches nothing", "One kernel launch whatever M and count are", "FLUID_FIELD_OF_POINT on a typed network is allowed",
                 "SLOT", "fluid_run_members when factor == 0", "fluid_run_members_coarse", "in slot order", "behind that step's snapshot packs",
                 "Empty slots launch nothing", "points in no slot are never written", "several slots may share a step",
                 "need not be in time order", "No wait anywhere", "nslots == 0 is the plain run",
                 "h_k[p] = record[k * member_stride + p]", "read in stream order", "Everything after rule 1 is untouched",
                 "the same cache", "fluid_analyse_lattice_status serves both", "gives the direct call's bits",
                 "No field is settled or read by the two Gram calls", "settles and updates only the listed `fields`",
                 "END of the window", "Whether it is typed does not matter", "a non-finite float in the record",
                 "zero-fill the record first", "inv_sigma 0", "FLUID_E_INVALID", "null pointers before the context is looked at",
                 "the slot is named", "FLUID_WINDOW_MAX_SLOTS", "a stride below P", "inside one allocation", "no network set",
                 "FLUID_TRANSFORM_MAX_MEMBERS", "row slabs") + tuple(ARGS):
        assert norm(word) in section, word


def window_case(capi):
    """a window and a plan that would pass, but for what a test takes out; the arrays are kept alive by the caller"""
    first, step = (C.c_int * 2)(0, 1), (C.c_int * 1)(0)
    w = capi.ObsWindow(field=2, nslots=1, slot_first=first, slot_step=step, record_dev=64, member_stride=0)
    plan = capi.RunPlan(iters=4, nsteps=1)
    return w, plan, (first, step)


def test_null_pointers_are_found_before_the_context_is_looked_at():
    capi, L = lib()
    one = (C.c_float * 1)(1.5)
    ids = (C.c_int * 1)(2)
    g = (C.c_double * 1)(7.0)
    n = (C.c_int * 1)(3)
    dev = C.c_void_p(64)                    # never dereferenced: a null pointer is refused first
    w, plan, keep = window_case(capi)
    pw, pp, written = C.byref(w), C.byref(plan), C.byref(C.c_int(5))
    no_record, _, keep2 = window_case(capi)
    no_record.record_dev = None
    no_first, _, keep3 = window_case(capi)
    no_first.slot_first = None
    no_step, _, keep4 = window_case(capi)
    no_step.slot_step = None
    many, _, keep5 = window_case(capi)
    many.nslots = capi.WINDOW_MAX_SLOTS + 1
    cases = [
        (lambda: L.fluid_observe_members_range(None, 2, 0, 1, None, 0), b"fluid_observe_members_range", b"record_dev"),
        (lambda: L.fluid_run_window(None, one, one, one, pp, 0, None, written), b"fluid_run_window", b"window"),
        (lambda: L.fluid_run_window(None, one, one, one, None, 0, pw, written), b"fluid_run_window", b"plan"),
        (lambda: L.fluid_run_window(None, None, one, one, pp, 0, pw, written), b"fluid_run_window", b"dt"),
        (lambda: L.fluid_run_window(None, one, None, one, pp, 0, pw, written), b"fluid_run_window", b"diff"),
        (lambda: L.fluid_run_window(None, one, one, None, pp, 0, pw, written), b"fluid_run_window", b"visc"),
        (lambda: L.fluid_run_window(None, one, one, one, pp, 0, C.byref(no_record), written), b"fluid_run_window", b"record_dev"),
        (lambda: L.fluid_run_window(None, one, one, one, pp, 0, C.byref(no_first), written), b"fluid_run_window", b"slot_first"),
        (lambda: L.fluid_run_window(None, one, one, one, pp, 0, C.byref(no_step), written), b"fluid_run_window", b"slot_step"),
        (lambda: L.fluid_run_window(None, one, one, one, pp, 0, C.byref(many), written), b"fluid_run_window", b"65537"),
        (lambda: L.fluid_observation_gram_recorded(None, None, 0, 1, one, one, g, g, g), b"fluid_observation_gram_recorded", b"record_dev"),
        (lambda: L.fluid_observation_gram_recorded(None, dev, 0, 1, one, one, None, g, g), b"fluid_observation_gram_recorded", b"gram"),
        (lambda: L.fluid_observation_gram_recorded(None, dev, 0, 1, None, one, g, g, None), b"fluid_observation_gram_recorded", b"rhs"),
        (lambda: L.fluid_observation_gram_lattice_recorded(None, None, 0, 1, one, one, 1, 1, 0, 0, 8, 2.0, g, g, g, n),
         b"fluid_observation_gram_lattice_recorded", b"record_dev"),
        (lambda: L.fluid_observation_gram_lattice_recorded(None, dev, 0, 1, one, one, 1, 1, 0, 0, 8, 2.0, None, g, g, n),
         b"fluid_observation_gram_lattice_recorded", b"gram"),
        (lambda: L.fluid_observation_gram_lattice_recorded(None, dev, 0, 1, None, one, 1, 1, 0, 0, 8, 2.0, g, None, g, n),
         b"fluid_observation_gram_lattice_recorded", b"dd"),
        (lambda: L.fluid_analyse_lattice_recorded(None, None, 0, one, one, 1, 1, 0, 0, 8, 2.0, 1.0, ids, 1),
         b"fluid_analyse_lattice_recorded", b"record_dev"),
        (lambda: L.fluid_analyse_lattice_recorded(None, dev, 0, None, one, 1, 1, 0, 0, 8, 2.0, 1.0, ids, 1),
         b"fluid_analyse_lattice_recorded", b"obs"),
        (lambda: L.fluid_analyse_lattice_recorded(None, dev, 0, one, one, 1, 1, 0, 0, 8, 2.0, 1.0, None, 1),
         b"fluid_analyse_lattice_recorded", b"fields"),
    ]
    for call, name, pointer in cases:
        msg = refused(L, capi, call(), name, pointer)
        assert b"context" not in msg, msg
    msg = refused(L, capi, L.fluid_run_window(None, one, one, one, pp, 0, C.byref(many), written), b"65537", b"65536")
    assert one[0] == 1.5 and ids[0] == 2 and g[0] == 7.0 and n[0] == 3
    del keep, keep2, keep3, keep4, keep5


def test_null_context_is_refused_by_name():
    capi, L = lib()
    one = (C.c_float * 1)(1.5)
    ids = (C.c_int * 1)(2)
    g = (C.c_double * 1)(7.0)
    n = (C.c_int * 1)(3)
    dev = C.c_void_p(64)                    # never dereferenced: the context is refused first
    w, plan, keep = window_case(capi)
    empty, _, keep2 = window_case(capi)     # the plain run: no slots, no slot arrays
    empty.nslots, empty.slot_first, empty.slot_step = 0, None, None
    written = C.c_int(5)
    for call, name in [
        (lambda: L.fluid_observe_members_range(None, capi.FIELD_OF_POINT, 0, 1, dev, 0), b"fluid_observe_members_range"),
        (lambda: L.fluid_run_window(None, one, one, one, C.byref(plan), 0, C.byref(w), C.byref(written)), b"fluid_run_window"),
        (lambda: L.fluid_run_window(None, one, one, one, C.byref(plan), 2, C.byref(empty), None), b"fluid_run_window"),
        (lambda: L.fluid_observation_gram_recorded(None, dev, 0, 1, one, one, g, g, g), b"fluid_observation_gram_recorded"),
        (lambda: L.fluid_observation_gram_recorded(None, dev, 0, 0, None, None, g, None, None), b"fluid_observation_gram_recorded"),
        (lambda: L.fluid_observation_gram_lattice_recorded(None, dev, 0, 1, one, one, 1, 1, 0, 0, 8, 2.0, g, g, g, n),
         b"fluid_observation_gram_lattice_recorded"),
        (lambda: L.fluid_analyse_lattice_recorded(None, dev, 0, one, one, 1, 1, 0, 0, 8, 2.0, 1.0, ids, 1), b"fluid_analyse_lattice_recorded"),
    ]:
        refused(L, capi, call(), name + b":", b"null context")
    assert one[0] == 1.5 and ids[0] == 2 and g[0] == 7.0 and n[0] == 3 and written.value == 5
    del keep, keep2


def test_solver_has_the_window_methods():
    from fluidsimulationcuda_amd import FluidSolver
    sig = {name: inspect.signature(getattr(FluidSolver, name)).parameters for name in
           ("observe_range", "run_window", "observation_gram_recorded", "observation_gram_lattice_recorded", "analyse_lattice_recorded")}
    p = sig["observe_range"]
    assert list(p) == ["self", "first", "count", "out", "field", "member_stride", "wait"]
    assert p["field"].default is None and p["member_stride"].default == 0 and p["wait"].default is True
    p = sig["run_window"]
    assert list(p)[:6] == ["self", "nsteps", "slot_first", "slot_step", "record", "field"]
    assert p["record"].default is None and p["field"].default is None and p["member_stride"].default == 0
    run = inspect.signature(FluidSolver.run).parameters
    for name in list(run)[2:]:                      # run's keywords, with run's defaults
        assert name in p and p[name].default == run[name].default, name
    # each recorded method takes `record` where its namesake takes `field`, plus member_stride=0
    for name in ("observation_gram", "observation_gram_lattice", "analyse_lattice"):
        old, new = inspect.signature(getattr(FluidSolver, name)).parameters, sig[name + "_recorded"]
        assert [("record" if k == "field" else k) for k in old] + ["member_stride"] == list(new), name
        assert new["member_stride"].default == 0 and new["record"].default is inspect.Parameter.empty
        for k in old:
            if k != "field":
                assert new[k].default == old[k].default, (name, k)
    for name in ("observe_range", "observation_gram_recorded"):
        assert "asynchronous observations" in getattr(FluidSolver, name).__doc__, name


def test_the_pinned_signatures_still_hold():
    from fluidsimulationcuda_amd import FluidSolver

    def params(name):
        return [(k, v.default) for k, v in inspect.signature(getattr(FluidSolver, name)).parameters.items()][1:]

    E = inspect.Parameter.empty
    assert params("observe_device") == [("field", None), ("out", None), ("member_stride", 0), ("wait", True)]
    assert params("observation_gram") == [("field", None), ("obs", None), ("inv_sigma", None), ("centre", True)]
    assert params("observation_gram_lattice") == [("field", E), ("shape", E), ("origin", E), ("step", E), ("c", E), ("obs", None),
                                                  ("inv_sigma", None), ("centre", True)]
    assert params("analyse_lattice") == [("field", E), ("shape", E), ("origin", E), ("step", E), ("c", E), ("obs", E), ("inv_sigma", None),
                                         ("rho", 1.0), ("fields", ("dens", "u", "v")), ("wait", True)]
