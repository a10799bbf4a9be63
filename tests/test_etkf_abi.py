"""CPU: the ABI of the one-call analysis -- fluid_etkf_increments, fluid_analyse_lattice, fluid_analyse_lattice_status
(include/fluid_amd.h, "one-call analysis").  Without a device only the refusals that come before the context is looked at
can be exercised: the calls name themselves when they refuse a null context, and null pointers are found first.
tests/test_abi.py holds the header, the exports and the bindings together.  The numpy model of the kernel's ordering
(tests/test_gpu_etkf.py: jacobi_model) needs no device either: it is run here, against its long-double self and eigh, and
its sweep count is what FLUID_ETKF_MAX_SWEEPS is held to."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = {"fluid_etkf_increments": 8, "fluid_analyse_lattice": 13, "fluid_analyse_lattice_status": 4}


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
    d = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    out = (C.c_float * 4)(7.0, 7.0, 7.0, 7.0)
    ids = (C.c_int * 1)(2)
    one = (C.c_float * 1)(1.0)
    n = C.c_int(7)
    refused(L, capi, L.fluid_etkf_increments(None, 1, d, d, None, 1.0, out, None), b"fluid_etkf_increments", b"null context")
    refused(L, capi, L.fluid_etkf_increments(None, -5, d, d, None, float("nan"), out, None), b"fluid_etkf_increments", b"null context")
    refused(L, capi, L.fluid_analyse_lattice(None, 2, one, None, 1, 1, 0, 0, 8, 1.0, 1.0, ids, 1), b"fluid_analyse_lattice", b"null context")
    refused(L, capi, L.fluid_analyse_lattice(None, -2, one, one, 0, -1, 5, 5, 7, -1.0, 0.0, ids, 40), b"fluid_analyse_lattice", b"null context")
    refused(L, capi, L.fluid_analyse_lattice_status(None, C.byref(n), None, None), b"fluid_analyse_lattice_status", b"null context")
    assert list(out) == [7.0] * 4 and n.value == 7


def test_null_pointers_are_found_before_the_context_is_looked_at():
    capi, L = lib()
    d = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    out = (C.c_float * 4)(7.0, 7.0, 7.0, 7.0)
    ids = (C.c_int * 1)(2)
    one = (C.c_float * 1)(1.0)
    refused(L, capi, L.fluid_etkf_increments(None, 1, None, d, None, 1.0, out, None), b"fluid_etkf_increments", b"gram")
    refused(L, capi, L.fluid_etkf_increments(None, 1, d, None, None, 1.0, out, None), b"fluid_etkf_increments", b"rhs")
    refused(L, capi, L.fluid_etkf_increments(None, 1, d, d, None, 1.0, None, None), b"fluid_etkf_increments", b"increments")
    refused(L, capi, L.fluid_analyse_lattice(None, 2, None, None, 1, 1, 0, 0, 8, 1.0, 1.0, ids, 1), b"fluid_analyse_lattice", b"obs")
    refused(L, capi, L.fluid_analyse_lattice(None, 2, one, None, 1, 1, 0, 0, 8, 1.0, 1.0, None, 1), b"fluid_analyse_lattice", b"fields")
    assert list(out) == [7.0] * 4


def header_text():
    src = open(ROOT + "/include/fluid_amd.h").read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_signatures_carry_the_headers_types():
    capi, _ = lib()
    ctype = {"fluid_ctx*": C.c_void_p, "int": C.c_int, "float": C.c_float, "const float*": capi._MF, "float*": capi._MF,
             "const double*": C.POINTER(C.c_double), "int*": C.POINTER(C.c_int), "const int*": C.POINTER(C.c_int)}
    _, src = header_text()
    for name, count in NEW.items():
        m = re.search(r"^int\s+%s\s*\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, name
        want = []
        for d in m.group(1).split(","):
            d = " ".join(d.split())
            t = re.match(r"(.*?)(\*?)\s*(\w+)$", d)           # type, star, name
            want.append(ctype[(t.group(1).strip() + t.group(2)).replace(" *", "*")])
        assert capi.SIGNATURES[name] == want, (name, capi.SIGNATURES[name], want)
        assert len(want) == count


def test_the_header_has_the_section_and_the_cap():
    raw, src = header_text()
    assert raw.index("lattice observations") < raw.index("one-call analysis") < raw.index("fluid_etkf_increments(fluid_ctx")
    assert raw.index("fluid_etkf_increments(fluid_ctx") < raw.index("fluid_analyse_lattice(fluid_ctx") < raw.index("fluid_set_jacobi_variant(fluid_ctx")
    m = re.search(r"^#define\s+FLUID_ETKF_MAX_SWEEPS\s+(\d+)\s*$", src, flags=re.M)
    from fluidsimulationcuda_amd import capi
    assert m and int(m.group(1)) == capi.ETKF_MAX_SWEEPS >= 16
    k = open(ROOT + "/fluidsimulationcuda_amd/csrc/fluid_etkf.h").read()
    assert re.search(r"kEtkfMaxSweeps\s*=\s*%d;" % capi.ETKF_MAX_SWEEPS, k)


def test_solver_has_the_three_calls():
    from fluidsimulationcuda_amd import FluidSolver
    p = inspect.signature(FluidSolver.etkf_increments).parameters
    assert list(p)[1:] == ["C_", "rhs", "counts", "rho"] and p["counts"].default is None and p["rho"].default == 1.0
    p = inspect.signature(FluidSolver.analyse_lattice).parameters
    assert list(p) == ["self", "field", "shape", "origin", "step", "c", "obs", "inv_sigma", "rho", "fields", "wait"], list(p)
    assert p["inv_sigma"].default is None and p["rho"].default == 1.0 and p["fields"].default == ("dens", "u", "v") and p["wait"].default is True
    assert list(inspect.signature(FluidSolver.analyse_status).parameters) == ["self"]


def test_the_model_the_arbiter_and_the_sweep_cap():
    """The float64 model of the kernel and eigh against the long-double model, in units of M 2^-53 sqrt(rho) kappa
    (measured: both within 1.2; asserted: 4), and the sweeps the float64 model needs over the inputs of the GPU tests, the
    last sweep -- the one without a rotation -- included.  FLUID_ETKF_MAX_SWEEPS is twice that and not below 16."""
    import test_gpu_etkf as E
    from fluidsimulationcuda_amd import capi
    most, worst = 0, 0.0
    for m in E.MEMBERS:
        gram, rhs = E.node_inputs(m)
        for rho in E.RHOS:
            for b in range(6):
                d_ref, _, kappa = E.reference(gram[b], rhs[b], rho)
                d64, sweeps = E.jacobi_model(gram[b], rhs[b], rho)
                dld, _ = E.jacobi_model(gram[b], rhs[b], rho, np.longdouble)
                most = max(most, sweeps)
                u = m * E.U * np.sqrt(rho) * kappa
                for name, d in (("the float64 model", d64), ("eigh", d_ref)):
                    err = float(np.abs(d.astype(np.longdouble) - dld).max()) / u
                    worst = max(worst, err)
                    assert err <= 4.0, (name, m, rho, E.KINDS[b], err)
    print("sweeps needed: %d; worst float64 error: %.2f units" % (most, worst))
    assert capi.ETKF_MAX_SWEEPS == max(16, 2 * most), (most, capi.ETKF_MAX_SWEEPS)


@pytest.mark.parametrize("padded", [2, 4, 8, 16, 32, 64])
def test_the_model_at_every_member_count(padded):
    """The round-robin ordering is another one for every M, so the float64 model is run at every M in 2 .. 64 (one instance
    per padded count, as in tests/test_gpu_member_counts.py) -- on the two node kinds that set the maxima of the full sweep,
    "P=5" and "P=40 scale 4", and rho in (1, 2).  (All six kinds and all three rho, run once by hand: at most 14 sweeps,
    which "P=40 scale 4" needs at M = 56 and at M = 64, and at most 1.25 units from eigh, at M = 3.)  The sweeps the model needs, the
    last one included, stay within half of FLUID_ETKF_MAX_SWEEPS, and it stays within the 4 units of M 2^-53 sqrt(rho) kappa
    of eigh that the test above asserts at its own counts: what the GPU test of every M rests its tolerance on."""
    import test_gpu_etkf as E
    from fluidsimulationcuda_amd import capi
    assert capi.TRANSFORM_MAX_MEMBERS == 64
    most, worst = (0, ()), (0.0, ())
    for m in range(padded // 2 + 1, padded + 1):
        gram, rhs = E.node_inputs(m)
        for rho in (1.0, 2.0):
            for b in (0, 1):
                d_ref, _, kappa = E.reference(gram[b], rhs[b], rho)
                d64, sweeps = E.jacobi_model(gram[b], rhs[b], rho)
                err = float(np.abs(d64 - d_ref).max()) / (m * E.U * np.sqrt(rho) * kappa)
                most, worst = max(most, (sweeps, (m, rho, E.KINDS[b]))), max(worst, (err, (m, rho, E.KINDS[b])))
                assert sweeps <= capi.ETKF_MAX_SWEEPS // 2, (m, rho, E.KINDS[b], sweeps)
                assert err <= 4.0, (m, rho, E.KINDS[b], err)
    print("most sweeps: %d at %s; worst distance from eigh: %.2f units at %s" % (most + worst))
