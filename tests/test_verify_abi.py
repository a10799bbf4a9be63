"""CPU: the ABI of "verifying ensembles" -- fluid_verify_members (include/fluid_amd.h).  Without a device only the refusals
that come before the context is looked at can be exercised: the call names itself when it refuses a null context, and null
pointers are found first.  The reference model of tests/verify_model.py is run here on the inputs of the GPU tests
(tests/test_gpu_verify.py) and shown to have the properties those tests lean on: the bounds are checked against the model,
not against the code under test.  tests/test_abi.py holds the header, the exports and the bindings together."""
import ctypes as C
import inspect
import math
import re

import numpy as np
import pytest

from conftest import ROOT
from verify_model import (F32, F64, ROW, cell_scores, crps_pairwise, dyadic_inputs, in_box, interior, pairwise_bound, random_inputs,
                          recursive_sums, score_row)

NAME = "fluid_verify_members"
SIZES = (14, 30, 61)
MEMBERS = (2, 3, 5, 8, 33, 64)
DYADIC_MEMBERS = (2, 8, 64)


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
    ids = (C.c_int * 1)(2)
    somewhere = C.c_void_p(64)                      # (never looked at: the context comes first)
    refused(L, capi, L.fluid_verify_members(None, ids, 1, somewhere, 0, None, 0, None, somewhere), b"fluid_verify_members", b"null context")
    refused(L, capi, L.fluid_verify_members(None, ids, -3, somewhere, 7, None, 99, somewhere, somewhere), b"fluid_verify_members",
            b"null context")


def test_null_pointers_are_found_before_the_context_is_looked_at():
    capi, L = lib()
    ids = (C.c_int * 1)(2)
    somewhere = C.c_void_p(64)
    refused(L, capi, L.fluid_verify_members(None, None, 1, somewhere, 0, None, 0, None, somewhere), b"fluid_verify_members", b"fields")
    refused(L, capi, L.fluid_verify_members(None, ids, 1, None, 0, None, 0, None, somewhere), b"fluid_verify_members", b"truth_dev")
    refused(L, capi, L.fluid_verify_members(None, ids, 1, somewhere, 0, None, 0, None, None), b"fluid_verify_members", b"scores_dev")


def header_text():
    src = open(ROOT + "/include/fluid_amd.h").read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_the_signature_carries_the_headers_types():
    capi, _ = lib()
    ctype = {"fluid_ctx*": C.c_void_p, "int": C.c_int, "size_t": C.c_size_t, "const int*": C.POINTER(C.c_int), "const void*": C.c_void_p,
             "void*": C.c_void_p}
    _, src = header_text()
    m = re.search(r"^int\s+%s\s*\((.*?)\);" % NAME, src, flags=re.S | re.M)
    assert m
    want = []
    for d in m.group(1).split(","):
        d = " ".join(d.split())
        t = re.match(r"(.*?)(\*?)\s*(\w+)$", d)           # type, star, name
        want.append(ctype[(t.group(1).strip() + t.group(2)).replace(" *", "*")])
    assert capi.SIGNATURES[NAME] == want, (capi.SIGNATURES[NAME], want)
    assert len(want) == 9


def test_the_header_has_the_section_and_its_constants():
    capi, _ = lib()
    raw, src = header_text()
    section = raw.index("---- verifying ensembles")
    assert raw.index("---- screening observations") < section < raw.index("fluid_verify_members(fluid_ctx")
    assert raw.index("fluid_verify_members(fluid_ctx") < raw.index("fluid_set_jacobi_variant(fluid_ctx")
    assert re.search(r"#define\s+FLUID_VERIFY_SUMS\s+5\b", src)
    assert re.search(r"#define\s+FLUID_VERIFY_ROW\s+\(FLUID_VERIFY_SUMS \+ FLUID_TRANSFORM_MAX_MEMBERS \+ 1\)", src)
    assert re.search(r"#define\s+FLUID_VERIFY_FAIR\s+1\b", src)
    assert (capi.VERIFY_SUMS, capi.VERIFY_ROW, capi.VERIFY_FAIR) == (5, 70, 1) and ROW == capi.VERIFY_ROW


def test_solver_has_verify_and_verify_scores():
    from fluidsimulationcuda_amd import FluidSolver
    p = inspect.signature(FluidSolver.verify).parameters
    assert list(p) == ["self", "truth", "fields", "box", "fair", "crps_map", "out", "wait"], list(p)
    assert p["truth"].default is inspect.Parameter.empty and p["fields"].default == ("dens",)
    assert p["box"].default is None and p["fair"].default is False and p["crps_map"].default is None and p["out"].default is None
    assert p["wait"].default is True
    assert list(inspect.signature(FluidSolver.verify_scores).parameters) == ["self", "out"]


# ---- the model on the GPU tests' inputs ------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def the_call_exists():
    """the model is the model of a call the library has: without the symbol nothing here says anything"""
    _, L = lib()
    assert hasattr(L, NAME)


def gpu_inputs(members):
    for n in SIZES:
        yield n, 0, random_inputs(n, members, 0, seed=100 * n + members)
    for n in (14, 66):
        yield n, 1, random_inputs(n, members, 1, seed=100 * n + members + 7)


@pytest.mark.parametrize("fair", [False, True], ids=["plain", "fair"])
@pytest.mark.parametrize("members", MEMBERS)
def test_the_sorted_form_is_the_pairwise_definition_and_is_not_negative(members, fair):
    """(i), (ii): on the inputs of the GPU model test"""
    for n, storage, (x, y) in gpu_inputs(members):
        c = cell_scores(x, y, fair)
        bound = pairwise_bound(x, y)
        err = np.abs(c["crps"] - crps_pairwise(x, y, fair))
        assert (err <= bound).all(), "n=%d M=%d storage=%d: off the pairwise form by %g, bound %g" % (n, members, storage, err.max(), bound.max())
        assert (c["crps"] >= -bound).all(), "n=%d M=%d storage=%d" % (n, members, storage)
        ties = (x[0] == x[1]).mean()
        assert 0.05 < ties < 0.3 and 0.05 < (y == x[members // 2]).mean() < 0.3, "the inputs have ties and truths equal to a member"
        assert np.abs(x).max() > 50.0 / (16 if storage else 1), "... and offsets"


@pytest.mark.parametrize("members", MEMBERS)
def test_equal_members_give_the_absolute_error_and_no_variance(members):
    """(iii)"""
    rng = np.random.default_rng(members)
    v = rng.uniform(-100, 100, (16, 16)).astype(F32)
    y = rng.uniform(-100, 100, (16, 16)).astype(F32)
    for fair in (False, True):
        c = cell_scores(np.broadcast_to(v, (members, 16, 16)), y, fair)
        # (the partial sums k * v of a float are exact in double for k <= 64, and (M * v) / M rounds to v: the mean is v)
        assert np.array_equal(c["var"], np.zeros((16, 16)))
        assert np.array_equal(c["e"], v.astype(F64) - y.astype(F64))
        assert np.array_equal(c["crps"], np.abs(v.astype(F64) - y.astype(F64)))
        assert np.array_equal(c["rank"], np.where(v < y, members, 0))


@pytest.mark.parametrize("members", DYADIC_MEMBERS)
def test_dyadic_sums_are_exact_in_every_order(members):
    """(iv): on the inputs of the GPU exact-sum test, recursive summation forwards, backwards and pairwise all equal fsum: for
    e, se and the CRPS (without FLUID_VERIFY_FAIR, whose divisor M (M - 1) is a power of two at M = 2 only), and for var at
    M = 2 (at other M the division by M - 1 is inexact)."""
    for n in (14, 61):
        x, y = dyadic_inputs(n, members, seed=9000 + 10 * n + members)
        for fair in ((False, True) if members == 2 else (False,)):
            c = cell_scores(x, y, fair)
            for name in ("e", "se", "crps") + (("var",) if members == 2 else ()):
                t = in_box(c[name], interior(n)).ravel()
                want = math.fsum(t)
                assert recursive_sums(t) == (want, want, want), "n=%d M=%d %s fair=%s" % (n, members, name, fair)


def test_the_rows_layout():
    x, y = random_inputs(14, 5, 0, seed=1)
    c = cell_scores(x, y)
    row = score_row(c, interior(14), 5)
    assert row.shape == (ROW,) and row[0] == 196 and row[5:11].sum() == 196 and not row[11:].any()
    assert score_row(c, (3, 3, 0, 16), 5)[0] == 0
