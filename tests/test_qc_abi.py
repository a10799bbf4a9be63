"""CPU: the ABI of screening observations -- fluid_observation_departures(_recorded), fluid_set_observation_qc,
fluid_observation_qc, fluid_observation_qc_result (include/fluid_amd.h, "screening observations").  Without a device only the
refusals that come before the context is looked at can be exercised.  The reference model of tests/qc_model.py, which
tests/test_gpu_qc.py holds the device to bit for bit, is checked here against what the header promises of it: threshold 0
rejects nothing, a point with sigma 0 is never rejected, a NaN rejects nothing, the rank lies in 0 .. M, the sums are the exact
sums on dyadic data.  tests/test_abi.py holds the header, the exports and the bindings together."""
import ctypes as C
import inspect
import math
import re

import numpy as np
import pytest

from conftest import ROOT
from qc_model import chunk_sum, gated_inv_sigma, moments, screen

F32 = np.float32
NEW = ("fluid_observation_departures", "fluid_observation_departures_recorded", "fluid_set_observation_qc", "fluid_observation_qc",
       "fluid_observation_qc_result")


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


def test_symbols_exist_and_are_bound():
    capi, L = lib()
    for name in NEW:
        assert hasattr(L, name) and name in capi.SIGNATURES, name


def test_null_context_is_refused_by_name():
    capi, L = lib()
    somewhere = C.c_void_p(64)                      # (never looked at: the context comes first)
    t = C.c_float(7.0)
    refused(L, capi, L.fluid_observation_departures(None, 2, None, None, 0.0, None, None, None, None, None, None),
            b"fluid_observation_departures", b"null context")
    refused(L, capi, L.fluid_observation_departures_recorded(None, somewhere, 0, None, None, 0.0, None, None, None, None, None, None),
            b"fluid_observation_departures_recorded", b"null context")
    refused(L, capi, L.fluid_set_observation_qc(None, 3.0), b"fluid_set_observation_qc", b"null context")
    refused(L, capi, L.fluid_observation_qc(None, C.byref(t)), b"fluid_observation_qc", b"null context")
    refused(L, capi, L.fluid_observation_qc_result(None, None, None, None), b"fluid_observation_qc_result", b"null context")
    assert t.value == 7.0


def test_refusals_found_before_the_context_is_looked_at():
    capi, L = lib()
    somewhere = C.c_void_p(64)
    one = np.ones(1, F32)
    f = one.ctypes.data_as(capi._MF)
    b = (C.c_ubyte * 1)(7)
    d = (C.c_double * 3)(7.0, 7.0, 7.0)
    for name, head in (("fluid_observation_departures", (None, 2)), ("fluid_observation_departures_recorded", (None, somewhere, 0))):
        fn, word = getattr(L, name), name.encode()
        # a per-observation output or `sums` without obs
        refused(L, capi, fn(*head, None, None, 0.0, None, None, f, None, None, None), word + b":", b"departure", b"obs")
        refused(L, capi, fn(*head, None, None, 0.0, None, None, None, b, None, None), word + b":", b"rank", b"obs")
        refused(L, capi, fn(*head, None, None, 0.0, None, None, None, None, b, None), word + b":", b"flag", b"obs")
        refused(L, capi, fn(*head, None, None, 0.0, None, None, None, None, None, d), word + b":", b"sums", b"obs")
        # the threshold
        for bad in (float("nan"), float("inf"), -1.0):
            refused(L, capi, fn(*head, f, None, bad, None, None, None, None, None, None), word + b":", b"threshold")
        refused(L, capi, fn(*head, None, None, 3.0, None, None, None, None, None, None), word + b":", b"threshold", b"obs")
    refused(L, capi, L.fluid_observation_departures_recorded(None, None, 0, f, None, 0.0, None, None, None, None, None, None),
            b"fluid_observation_departures_recorded", b"record_dev")
    for bad in (float("nan"), float("inf"), -0.5):
        refused(L, capi, L.fluid_set_observation_qc(None, bad), b"fluid_set_observation_qc", b"threshold")
    refused(L, capi, L.fluid_observation_qc(None, None), b"fluid_observation_qc", b"threshold")
    assert one[0] == 1.0 and b[0] == 7 and list(d) == [7.0, 7.0, 7.0]


def header_text():
    src = open(ROOT + "/include/fluid_amd.h").read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_signatures_carry_the_headers_types():
    capi, _ = lib()
    ctype = {"fluid_ctx*": C.c_void_p, "int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "const float*": C.POINTER(C.c_float),
             "float*": C.POINTER(C.c_float), "const void*": C.c_void_p, "unsigned char*": C.POINTER(C.c_ubyte), "double*": C.POINTER(C.c_double),
             "int*": C.POINTER(C.c_int)}
    _, src = header_text()
    count = dict(zip(NEW, (11, 12, 2, 2, 4)))
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


def test_the_header_has_the_section_and_says_what_the_gate_is_not():
    raw, _ = header_text()
    section = raw.index("---- screening observations")
    assert raw.index("---- asynchronous observations") < raw.index("fluid_analyse_lattice_recorded(fluid_ctx") < section
    assert section < raw.index("fluid_observation_departures(fluid_ctx") < raw.index("fluid_set_jacobi_variant(fluid_ctx")
    text = raw[section:raw.index("fluid_observation_departures(fluid_ctx")]
    assert "NO guard" in text and "inf * 0 = NaN" in text                 # the gate is no guard against non-finite values
    assert "(sums[1] - sums[0]) /" in text                                # the inflation recipe


def test_solver_has_the_four_methods():
    from fluidsimulationcuda_amd import FluidSolver
    assert list(inspect.signature(FluidSolver.set_observation_qc).parameters) == ["self", "threshold"]
    assert list(inspect.signature(FluidSolver.observation_qc).parameters) == ["self"]
    assert list(inspect.signature(FluidSolver.observation_qc_result).parameters) == ["self"]
    p = inspect.signature(FluidSolver.observation_departures).parameters
    assert list(p)[:3] == ["self", "field", "record"] and p["field"].default is None and p["record"].default is None
    assert p["threshold"].default == 0.0 and p["obs"].default is None and p["inv_sigma"].default is None


# ---- the model's own sanity ---------------------------------------------------------------------------------------------
def ensemble(rng, members, points):
    return (rng.normal(size=(1, points)) * 3 + rng.normal(size=(members, points))).astype(F32)


@pytest.mark.parametrize("members", [2, 5, 9, 33, 64])
def test_the_model_keeps_the_headers_promises(members):
    rng = np.random.default_rng(900 + members)
    points = 130
    h = ensemble(rng, members, points)
    mean, var = moments(h)
    y = (mean + 100.0 * np.sqrt(var + 1.0) * rng.choice([-1.0, 1.0], points)).astype(F32)    # every point a gross error
    sg = rng.uniform(0.5, 2.0, points).astype(F32)
    # threshold 0 rejects nothing, whatever the departures
    r = screen(h, y, sg, 0.0)
    assert not r["flag"].any() and r["sums"][0] == points
    # ... and a threshold rejects them all: 100^2 (var + 1) sg^2 >= 2500 + 10^4 var sg^2 against 9 (1 + var sg^2)
    r = screen(h, y, sg, 3.0)
    assert r["flag"].all() and r["sums"].view(np.uint64).tolist() == [np.float64(-0.0).view(np.uint64)] * 3
    # a point with sigma 0 is never rejected: d = 0
    sg0 = sg.copy()
    sg0[::3] = 0.0
    r = screen(h, y, sg0, 3.0)
    assert not r["flag"][::3].any() and r["flag"][1::3].all() and (r["d"][::3] == 0).all()
    s, flag = gated_inv_sigma(h, y, sg0, 3.0)
    assert np.array_equal(flag, r["flag"]) and not s[flag != 0].any() and np.array_equal(s[flag == 0], sg0[flag == 0])
    s, _ = gated_inv_sigma(h, y, None, 0.0)
    assert (s == 1.0).all()
    # a NaN anywhere rejects nothing at that point
    hn, yn, sn = h.copy(), y.copy(), sg.copy()
    hn[1, 4] = yn[5] = sn[6] = np.nan
    yn[7] = np.inf                                                      # (an inf is rejected: the gate is no guard against it)
    r = screen(hn, yn, sn, 3.0)
    assert not r["flag"][4:7].any() and r["flag"][7] == 1 and r["flag"][8:].all()
    # an obs at the mean lies between the members: its rank is in 0 .. M, and no rank leaves that range
    r = screen(h, mean.astype(F32), sg, 3.0)
    assert (r["rank"] >= 0).all() and (r["rank"] <= members).all() and not r["flag"].any()
    assert (r["rank"] > 0).any() and (r["rank"] < members).any()
    assert (screen(h, np.full(points, 1e6, F32))["rank"] == members).all() and not screen(h, np.full(points, -1e6, F32))["rank"].any()
    # a tie is "not below"
    assert (screen(h, h[0])["rank"] == (h < h[0][None]).sum(axis=0)).all() and screen(h[:, :1] * 0, np.zeros(1, F32))["rank"][0] == 0
    # the spread is the sample standard deviation
    assert np.allclose(screen(h)["spread"], h.astype(np.float64).std(axis=0, ddof=1), rtol=1e-6)
    assert set(screen(h)) == {"mean", "spread"}


def test_the_models_sums_are_exact_on_dyadic_data():
    rng = np.random.default_rng(77)
    for points in (1, 63, 65, 130, 64 * 16 + 5, 3000):
        terms = rng.integers(-64, 65, points) / 16.0
        keep = rng.random(points) < 0.7
        assert chunk_sum(terms, keep) == math.fsum(terms[keep]), points
        assert chunk_sum(np.ones(points), keep) == keep.sum()
    none = chunk_sum(np.ones(130), np.zeros(130, bool))
    assert none == 0 and np.signbit(none)                              # nothing kept: -0.0
