"""CPU: the ABI of relaxation to prior spread -- fluid_member_spread / fluid_relax_spread (include/fluid_amd.h, "relaxation
to prior spread").  Without a device only the refusals that come before the context is looked at can be exercised: both
calls name themselves when they refuse a null context, and null pointers are found first.  The reference model of
tests/relax_model.py is run here on the inputs of the GPU property test (tests/test_gpu_relax.py, part 4) and shown to stay
within that test's bound: the bound is checked against the reference, not against the code under test.
tests/test_abi.py holds the header, the exports and the bindings together."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from conftest import ROOT
from relax_model import narrow, property_bound, property_inputs, relax_model, spread_model

NEW = ("fluid_member_spread", "fluid_relax_spread")
PROPERTY_SIZES = (14, 30)
PROPERTY_MEMBERS = (2, 3, 5, 64, 70)


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
    somewhere = C.c_void_p(64)                      # (never looked at: the context comes first)
    refused(L, capi, L.fluid_member_spread(None, ids, 1, somewhere, 0), b"fluid_member_spread", b"null context")
    refused(L, capi, L.fluid_member_spread(None, ids, -3, somewhere, 7), b"fluid_member_spread", b"null context")
    refused(L, capi, L.fluid_relax_spread(None, ids, 1, somewhere, 0, 0.5), b"fluid_relax_spread", b"null context")
    refused(L, capi, L.fluid_relax_spread(None, ids, 99, somewhere, 1, 0.5), b"fluid_relax_spread", b"null context")


def test_null_pointers_are_found_before_the_context_is_looked_at():
    capi, L = lib()
    ids = (C.c_int * 1)(0)
    somewhere = C.c_void_p(64)
    refused(L, capi, L.fluid_member_spread(None, None, 1, somewhere, 0), b"fluid_member_spread", b"fields")
    refused(L, capi, L.fluid_member_spread(None, ids, 1, None, 0), b"fluid_member_spread", b"out_dev")
    refused(L, capi, L.fluid_relax_spread(None, None, 1, somewhere, 0, 0.5), b"fluid_relax_spread", b"fields")
    refused(L, capi, L.fluid_relax_spread(None, ids, 1, None, 0, 0.5), b"fluid_relax_spread", b"prior_dev")


def header_text():
    src = open(ROOT + "/include/fluid_amd.h").read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_signatures_carry_the_headers_types():
    capi, _ = lib()
    ctype = {"fluid_ctx*": C.c_void_p, "int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "const int*": C.POINTER(C.c_int),
             "const void*": C.c_void_p, "void*": C.c_void_p}
    _, src = header_text()
    count = {"fluid_member_spread": 5, "fluid_relax_spread": 6}
    for name in NEW:
        m = re.search(r"^int\s+%s\s*\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, name
        want = []
        for d in m.group(1).split(","):
            d = " ".join(d.split())
            t = re.match(r"(.*?)(\*?)\s*(\w+)$", d)           # type, star, name
            want.append(ctype[(t.group(1).strip() + t.group(2)).replace(" *", "*")])
        assert capi.SIGNATURES[name] == want, (name, capi.SIGNATURES[name], want)
        assert len(want) == count[name]


def test_the_header_has_the_section_between_the_analysis_and_the_jacobi_variant():
    raw, _ = header_text()
    assert "relaxation to prior spread" in raw
    section = raw.index("---- relaxation to prior spread")
    assert raw.index("---- one-call analysis") < raw.index("fluid_analyse_lattice_status(fluid_ctx") < section
    assert section < raw.index("fluid_member_spread(fluid_ctx") < raw.index("fluid_relax_spread(fluid_ctx")
    assert raw.index("fluid_relax_spread(fluid_ctx") < raw.index("fluid_set_jacobi_variant(fluid_ctx")


def test_solver_has_spread_and_relax_spread():
    from fluidsimulationcuda_amd import FluidSolver
    p = inspect.signature(FluidSolver.spread).parameters
    assert list(p) == ["self", "fields", "out", "wait"], list(p)
    assert p["fields"].default == ("u", "v", "dens") and p["out"].default is None and p["wait"].default is True
    p = inspect.signature(FluidSolver.relax_spread).parameters
    assert list(p) == ["self", "prior", "alpha", "fields", "wait"], list(p)
    assert all(p[k].default is inspect.Parameter.empty for k in ("prior", "alpha"))
    assert p["fields"].default == ("u", "v", "dens") and p["wait"].default is True


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", PROPERTY_MEMBERS)
def test_the_model_stays_within_the_property_tests_bound(members, storage):
    """alpha = 1 on the GPU property test's inputs, by the model alone: the spread afterwards is the prior one to within
    the bound that test asserts."""
    for n in PROPERTY_SIZES:
        x = property_inputs(n, members, storage, seed=4000 + 100 * storage + members)
        assert np.isfinite(x).all()
        if storage:
            assert (np.abs(x) >= 2.0 ** -14).all()                  # normal halves
        sd_b = spread_model(x)
        assert (sd_b > 0).all()
        y, stored = relax_model(x, sd_b, 1.0, storage)
        assert np.array_equal(narrow(y, storage), y)
        err = np.abs(spread_model(y).astype(np.float64) - sd_b.astype(np.float64))
        bound = property_bound(y, sd_b, storage)
        assert (err <= bound).all(), "n=%d M=%d storage=%d: the model misses the bound by %g" % (n, members, storage, (err - bound).max())
        # ... and alpha = 1 does something: the prior of a perturbed ensemble is restored, not met by accident
        shrunk = narrow(x.mean(axis=0, dtype=np.float64) + 0.5 * (x - x.mean(axis=0, dtype=np.float64)), storage)
        y, stored = relax_model(shrunk, sd_b, 1.0, storage)
        assert stored.mean() > 0.9
        err = np.abs(spread_model(y).astype(np.float64) - sd_b.astype(np.float64))
        assert (err <= property_bound(y, sd_b, storage)).all(), "n=%d M=%d storage=%d (shrunk ensemble)" % (n, members, storage)

