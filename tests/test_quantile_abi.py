"""CPU: the ABI of "ensemble products" -- fluid_quantile_position, fluid_member_quantiles, fluid_member_exceedance
(include/fluid_amd.h).  Without a device only the refusals that come before the context is looked at can be exercised, and
fluid_quantile_position, which is host logic: it is held to the model bit for bit.  The reference model of
tests/quantile_model.py is run here on the inputs of the GPU tests (tests/test_gpu_quantile.py) and shown to have the
properties a quantile has.  tests/test_abi.py holds the header, the exports and the bindings together."""
import ctypes as C
import functools
import inspect
import re
import struct

import numpy as np
import pytest

from conftest import ROOT
from quantile_model import ABOVE, BELOW, F32, LEVELS, exceedance, inputs, quantile_position, quantiles, sorted_members

NAMES = ("fluid_quantile_position", "fluid_member_quantiles", "fluid_member_exceedance")
SIZES = (14, 30, 61)
MEMBERS = (1, 2, 3, 5, 8, 33, 64)


@functools.lru_cache(maxsize=None)
def lib():
    """(built once for this file)"""
    import __graft_entry__ as g
    g.build()
    from fluidsimulationcuda_amd import capi
    return capi, capi.lib()


def refused(L, capi, rc, *words):
    assert rc == capi.E_INVALID
    msg = L.fluid_last_error()
    for w in words:
        assert w in msg, msg


def floats(*v):
    return (C.c_float * len(v))(*v)


def test_null_contexts_are_refused_by_name():
    capi, L = lib()
    somewhere = C.c_void_p(64)                      # (never looked at: the context comes first)
    refused(L, capi, L.fluid_member_quantiles(None, 2, floats(0.5), 1, somewhere, 0), b"fluid_member_quantiles", b"null context")
    refused(L, capi, L.fluid_member_quantiles(None, 99, floats(7.0), -3, somewhere, 5), b"fluid_member_quantiles", b"null context")
    refused(L, capi, L.fluid_member_exceedance(None, 2, floats(0.5), 1, 0, somewhere, 0), b"fluid_member_exceedance", b"null context")
    refused(L, capi, L.fluid_member_exceedance(None, 99, floats(np.nan), 77, 9, somewhere, 5), b"fluid_member_exceedance", b"null context")


def test_null_pointers_are_found_before_the_context_is_looked_at():
    capi, L = lib()
    somewhere = C.c_void_p(64)
    refused(L, capi, L.fluid_member_quantiles(None, 2, None, 1, somewhere, 0), b"fluid_member_quantiles", b"levels")
    refused(L, capi, L.fluid_member_quantiles(None, 2, floats(0.5), 1, None, 0), b"fluid_member_quantiles", b"out_dev")
    refused(L, capi, L.fluid_member_exceedance(None, 2, None, 1, 0, somewhere, 0), b"fluid_member_exceedance", b"thresholds")
    refused(L, capi, L.fluid_member_exceedance(None, 2, floats(0.5), 1, 0, None, 0), b"fluid_member_exceedance", b"out_dev")
    lo, frac = C.c_int(), C.c_double()
    refused(L, capi, L.fluid_quantile_position(5, 0.5, None, C.byref(frac)), b"fluid_quantile_position", b"lo")
    refused(L, capi, L.fluid_quantile_position(5, 0.5, C.byref(lo), None), b"fluid_quantile_position", b"frac")


def header_text():
    src = open(ROOT + "/include/fluid_amd.h").read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


@pytest.mark.parametrize("name,count", zip(NAMES, (4, 6, 7)))
def test_the_signatures_carry_the_headers_types(name, count):
    capi, _ = lib()
    ctype = {"fluid_ctx*": C.c_void_p, "int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "int*": C.POINTER(C.c_int),
             "double*": C.POINTER(C.c_double), "const float*": C.POINTER(C.c_float), "void*": C.c_void_p}
    _, src = header_text()
    m = re.search(r"^int\s+%s\s*\((.*?)\);" % name, src, flags=re.S | re.M)
    assert m
    want = []
    for d in m.group(1).split(","):
        d = " ".join(d.split())
        t = re.match(r"(.*?)(\*?)\s*(\w+)$", d)           # type, star, name
        want.append(ctype[(t.group(1).strip() + t.group(2)).replace(" *", "*")])
    assert capi.SIGNATURES[name] == want, (capi.SIGNATURES[name], want)
    assert len(want) == count


def test_the_header_has_the_section_and_its_constants():
    capi, _ = lib()
    raw, src = header_text()
    section = raw.index("---- ensemble products: quantile fields and exceedance probabilities")
    assert raw.index("---- verifying ensembles") < raw.index("fluid_verify_members(fluid_ctx") < section
    at = [raw.index(name + "(") for name in NAMES]
    assert section < min(at) and max(at) < raw.index("fluid_set_jacobi_variant(fluid_ctx")
    assert re.search(r"#define\s+FLUID_QUANTILE_MAX_LEVELS\s+16\b", src)
    assert re.search(r"enum\s*\{\s*FLUID_EXCEED_ABOVE\s*=\s*0\s*,\s*FLUID_EXCEED_BELOW\s*=\s*1\s*\}", src)
    assert (capi.QUANTILE_MAX_LEVELS, capi.EXCEED_ABOVE, capi.EXCEED_BELOW) == (16, 0, 1) == (16, ABOVE, BELOW)


def test_solver_has_quantiles_exceedance_and_quantile_position():
    import fluidsimulationcuda_amd as f
    p = inspect.signature(f.FluidSolver.quantiles).parameters
    assert list(p) == ["self", "field", "levels", "out", "wait"], list(p)
    assert p["field"].default == "dens" and p["levels"].default == (0.5,) and p["out"].default is None and p["wait"].default is True
    p = inspect.signature(f.FluidSolver.exceedance).parameters
    assert list(p) == ["self", "field", "thresholds", "below", "out", "wait"], list(p)
    assert p["field"].default is inspect.Parameter.empty and p["thresholds"].default is inspect.Parameter.empty
    assert p["below"].default is False and p["out"].default is None and p["wait"].default is True
    assert list(inspect.signature(f.quantile_position).parameters) == ["members", "level"]
    assert f.quantile_position(5, 0.5) == (2, 0.0) and "coefficients" in dir(f)


# ---- fluid_quantile_position: host logic, bit for bit --------------------------------------------------------------------------
POSITION_LEVELS = (0.0, 1.0, 0.5, 1.0 / 3.0, 0.05, 0.95, float(np.nextafter(F32(1.0), F32(0.0))), float(np.nextafter(F32(0.0), F32(1.0))))


def bits(v):
    return struct.pack("<d", v)


def test_quantile_position_is_the_models_bit_for_bit():
    capi, L = lib()
    assert POSITION_LEVELS[-1] == 2.0 ** -149 and POSITION_LEVELS[-2] == 1.0 - 2.0 ** -24
    lo, frac = C.c_int(), C.c_double()
    for members in range(1, 65):
        for level in POSITION_LEVELS:
            lo.value, frac.value = -7, -7.0
            assert L.fluid_quantile_position(members, level, C.byref(lo), C.byref(frac)) == capi.OK, L.fluid_last_error()
            want = quantile_position(members, level)
            assert (lo.value, bits(frac.value)) == (want[0], bits(want[1])), (members, level, lo.value, frac.value, want)
            assert 0 <= lo.value <= members - 1 and 0.0 <= frac.value < 1.0 and (lo.value < members - 1 or frac.value == 0.0)
            # numpy's "linear" position: lo + frac is level * (M - 1), exactly
            assert lo.value + frac.value == float(F32(level)) * (members - 1) or level == 1.0
    assert quantile_position(64, 0.5) == (31, 0.5) and quantile_position(5, 0.5) == (2, 0.0) and quantile_position(1, 0.7) == (0, 0.0)
    assert quantile_position(64, 1.0) == (63, 0.0) and quantile_position(64, POSITION_LEVELS[-2])[0] == 62


def test_quantile_position_refusals():
    capi, L = lib()
    lo, frac = C.c_int(-7), C.c_double(-7.0)
    for members, level, words in ((0, 0.5, (b"members 0",)), (65, 0.5, (b"members 65", b"64")), (-1, 0.5, (b"members -1",)),
                                  (5, -0.1, (b"level -0.1",)), (5, 1.5, (b"level 1.5",)), (5, float("nan"), (b"level nan",)),
                                  (5, float("inf"), (b"level inf",)), (5, float(np.nextafter(F32(1.0), F32(2.0))), (b"level 1",))):
        refused(L, capi, L.fluid_quantile_position(members, level, C.byref(lo), C.byref(frac)), b"fluid_quantile_position", *words)
        assert (lo.value, frac.value) == (-7, -7.0), "a refusal writes nothing"


# ---- the model on the GPU tests' inputs ------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def the_calls_exist():
    """the model is the model of calls the library has: without the symbols nothing here says anything"""
    _, L = lib()
    for name in NAMES:
        assert hasattr(L, name)


def gpu_inputs(members):
    for n in SIZES:
        yield n, 0, inputs(n, members, 0, seed=100 * n + members)
    for n in (14, 66):
        yield n, 1, inputs(n, members, 1, seed=100 * n + members + 7)


@pytest.mark.parametrize("members", MEMBERS)
def test_the_models_quantiles_are_quantiles(members):
    levels = sorted(LEVELS)
    for n, storage, x in gpu_inputs(members):
        what = "n=%d M=%d storage=%d" % (n, members, storage)
        assert x.shape == (members, n + 2, n + 2) and x.dtype == F32
        q = quantiles(x, levels)
        s = sorted_members(x)
        assert np.isfinite(q).all(), what
        assert (np.diff(q, axis=0) >= 0).all(), what + ": not non-decreasing in the level"
        for l, level in enumerate(levels):
            lo, frac = quantile_position(members, level)
            hi = min(lo + 1, members - 1)
            assert ((s[lo] <= q[l]) & (q[l] <= s[hi])).all(), what + ": level %g leaves [s_lo, s_lo+1]" % level
        assert np.array_equal(q[0], x.min(axis=0) + F32(0)) and np.array_equal(q[-1], x.max(axis=0) + F32(0)), what
        # numpy's own quantile, in float64, rounds elsewhere: close, not equal
        ref = np.quantile(x.astype(np.float64), [float(F32(v)) for v in levels], axis=0)
        assert np.allclose(q, ref, rtol=1e-6, atol=1e-6 * np.abs(x).max()), what
        if members > 1:
            assert 0.05 < (x[0] == x[1]).mean() < 0.3, "the inputs have ties"


@pytest.mark.parametrize("members", MEMBERS)
def test_equal_members_give_that_value_at_every_level(members):
    rng = np.random.default_rng(members)
    v = rng.uniform(-100, 100, (16, 16)).astype(F32)
    v[0, :4] = [0.0, -0.0, 1e-45, -1e-45]
    q = quantiles(np.broadcast_to(v, (members, 16, 16)), LEVELS)
    for l in range(len(LEVELS)):
        assert np.array_equal((v + F32(0)).view(np.uint32), q[l].view(np.uint32))
    for mode in (ABOVE, BELOW):
        e = exceedance(np.broadcast_to(v, (members, 16, 16)), [0.0], mode)[0]
        assert np.array_equal(e, np.where((v < 0) if mode == BELOW else (v > 0), 1, 0).astype(F32))


def test_the_models_exceedance_counts():
    x = np.array([[1.0, 0.0, np.nan, np.inf], [2.0, -0.0, 1.0, -np.inf], [3.0, 0.0, 3.0, 5.0]], F32)
    above, below = exceedance(x, [2.0, 0.0], ABOVE), exceedance(x, [2.0, 0.0], BELOW)
    third = F32(1.0 / 3.0)
    assert np.array_equal(above[0], np.array([third, 0, third, F32(2.0 / 3.0)], F32))
    assert np.array_equal(below[0], np.array([third, 1, third, third], F32))
    assert np.array_equal(above[1], np.array([1, 0, F32(2.0 / 3.0), F32(2.0 / 3.0)], F32))
    assert np.array_equal(below[1], np.array([0, 0, 0, third], F32))
    # complementary where nothing ties and nothing is a NaN
    x = inputs(14, 5, 0, seed=3)
    t = [0.37]
    assert not (x == F32(0.37)).any()
    assert np.array_equal(np.rint(exceedance(x, t, ABOVE)[0] * 5) + np.rint(exceedance(x, t, BELOW)[0] * 5), np.full(x.shape[1:], 5.0))


# ---- one body each -------------------------------------------------------------------------------------------------------------
def test_one_sorting_network_and_one_position_body():
    src = {f: open(ROOT + "/fluidsimulationcuda_amd/csrc/" + f).read() for f in ("fluid_sort.h", "fluid_quantile.h", "fluid_quantile.hip",
                                                                                "fluid_verify.hip", "fluid_solver.hip")}
    define = r"void\s+verify_sort\s*\("
    assert len(re.findall(define, src["fluid_sort.h"])) == 1
    for f in ("fluid_quantile.hip", "fluid_verify.hip"):
        assert '#include "fluid_sort.h"' in src[f] and "verify_sort<MP>(v)" in src[f] and not re.search(define, src[f]), f
    assert len(re.findall(r"inline void quantile_position\(", src["fluid_quantile.h"])) == 1
    # fluid_quantile_position and fluid_member_quantiles both go through it, and neither restates it
    assert src["fluid_solver.hip"].count("fluid::quantile_position(") == 2 and "floor" not in src["fluid_quantile.hip"]
    body = src["fluid_solver.hip"]
    body = body[body.index("int fluid_quantile_position("):body.index("int fluid_member_exceedance(")]
    assert "floor" not in body
