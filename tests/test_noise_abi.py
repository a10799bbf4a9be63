"""CPU: the ABI of the ensemble noise -- fluid_noise_members / fluid_noise_dense / fluid_noise_value (include/fluid_amd.h,
"ensemble noise").  The generator is host logic as much as device code -- one body for both --, so fluid_noise_value is
checked here against the numpy model of tests/noise_model.py, bit for bit, and the model against the published known
answers of Philox4x32-10.  Without a device the other two calls can only show the refusals that come before the context
is looked at.  The statistics of the definition are checked on the model alone, with fixed seeds."""
import ctypes as C
import inspect
import re

import numpy as np

from conftest import ROOT
from noise_model import C as NOISE_C, DENSE_TAG, KNOWN_ANSWERS, field_z, halves_sum, philox, z_of

NEW = {"fluid_noise_members": 8, "fluid_noise_dense": 7, "fluid_noise_value": 7}


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


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def test_the_model_reproduces_the_known_answers():
    for counter, key, want in KNOWN_ANSWERS:
        got = philox(*counter, *key)
        assert tuple(int(w) for w in got) == want, [hex(int(w)) for w in got]
    # ... and as arrays, all three at once
    cols = [np.array([ka[0][k] for ka in KNOWN_ANSWERS]) for k in range(4)] + [np.array([ka[1][k] for ka in KNOWN_ANSWERS]) for k in range(2)]
    got = philox(*cols)
    for k in range(4):
        assert [int(w) for w in got[k]] == [ka[2][k] for ka in KNOWN_ANSWERS]


def test_the_constant_is_the_one_rounding_of_its_definition():
    from fractions import Fraction
    # C^2 * 8 * (2^32 - 1) / 12 = 1 to within the rounding of C: |C - exact| <= ulp(C) / 2 = 2^-69
    exact_sq = Fraction(12, 8 * (2 ** 32 - 1))
    c = Fraction(NOISE_C)
    lo, hi = c - Fraction(1, 2 ** 69), c + Fraction(1, 2 ** 69)
    assert lo * lo <= exact_sq <= hi * hi
    assert 262140 * NOISE_C <= 4.899 and 262140 * NOISE_C > 4.898


def value(L, capi, seed, sequence, tag, ident, c0, c1):
    z = C.c_double()
    assert L.fluid_noise_value(seed, sequence, tag, ident, c0, c1, C.byref(z)) == capi.OK, L.fluid_last_error()
    return z.value


def test_noise_value_equals_the_model_bit_for_bit():
    capi, L = lib()
    # the known-answer counters: word 2 = (tag << 16) | id must be split into a legal tag and id, so the key and the other
    # three words are the known answers' and word 2 is their word 2 with the tag's top 12 bits cleared
    for counter, key, _ in KNOWN_ANSWERS:
        seed = key[0] | (key[1] << 32)
        tag, ident = (counter[2] >> 16) & 15, counter[2] & 0xFFFF
        got = value(L, capi, seed, counter[3], tag, ident, counter[0], counter[1])
        want = z_of(seed, counter[3], tag, ident, counter[0], counter[1])
        assert bits(got) == bits(want), (got, float(want))
    # the first known answer needs no clearing: its z follows from the published words themselves
    w = KNOWN_ANSWERS[0][2]
    s = sum((x & 0xFFFF) + (x >> 16) for x in w)
    assert value(L, capi, 0, 0, 0, 0, 0, 0) == (s - 262140) * NOISE_C
    rng = np.random.default_rng(20260101)
    n = 1000
    seeds = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    words = rng.integers(0, 2 ** 32, (3, n), dtype=np.uint64)
    tags = rng.integers(0, 16, n)
    ids = rng.integers(0, 65536, n)
    for k in range(n):
        got = value(L, capi, int(seeds[k]), int(words[0, k]), int(tags[k]), int(ids[k]), int(words[1, k]), int(words[2, k]))
        want = z_of(int(seeds[k]), int(words[0, k]), int(tags[k]), int(ids[k]), int(words[1, k]), int(words[2, k]))
        assert bits(got) == bits(want), (k, got, float(want))
    # small counters, as field cells have them, and the extremes of every argument
    for seed in (0, 1, 2 ** 32, 2 ** 64 - 1):
        for seq in (0, 1, 2 ** 32 - 1):
            for tag, ident in ((0, 0), (11, 65535), (DENSE_TAG, 7)):
                for c0, c1 in ((0, 0), (255, 3), (2 ** 32 - 1, 2 ** 32 - 1)):
                    assert bits(value(L, capi, seed, seq, tag, ident, c0, c1)) == bits(z_of(seed, seq, tag, ident, c0, c1))


def test_solver_noise_value_is_the_same_call():
    from fluidsimulationcuda_amd import noise_value
    assert bits(noise_value(5, 6, 2, 3, 4, 1)) == bits(z_of(5, 6, 2, 3, 4, 1))


def test_noise_value_refusals():
    capi, L = lib()
    z = C.c_double(123.0)
    refused(L, capi, L.fluid_noise_value(0, 0, 0, 0, 0, 0, None), b"fluid_noise_value", b"`z`")
    refused(L, capi, L.fluid_noise_value(0, 0, -1, 0, 0, 0, C.byref(z)), b"fluid_noise_value", b"tag -1")
    refused(L, capi, L.fluid_noise_value(0, 0, 16, 0, 0, 0, C.byref(z)), b"fluid_noise_value", b"tag 16")
    refused(L, capi, L.fluid_noise_value(0, 0, 0, -1, 0, 0, C.byref(z)), b"fluid_noise_value", b"member_id -1")
    refused(L, capi, L.fluid_noise_value(0, 0, 0, 65536, 0, 0, C.byref(z)), b"fluid_noise_value", b"member_id 65536")
    assert z.value == 123.0


def test_null_context_is_refused_by_name():
    capi, L = lib()
    ids = (C.c_int * 1)(0)
    amp = (C.c_float * 1)(1.0)
    somewhere = C.c_void_p(64)                      # (never looked at: the context comes first)
    refused(L, capi, L.fluid_noise_members(None, ids, 1, capi.NOISE_SET, amp, 1, 0, 0), b"fluid_noise_members", b"null context")
    refused(L, capi, L.fluid_noise_members(None, ids, -3, 7, amp, 1, 0, -5), b"fluid_noise_members", b"null context")
    refused(L, capi, L.fluid_noise_dense(None, somewhere, 4, 1.0, 1, 0, 0), b"fluid_noise_dense", b"null context")
    refused(L, capi, L.fluid_noise_dense(None, somewhere, 4, float("nan"), 1, 0, -1), b"fluid_noise_dense", b"null context")


def test_null_pointers_are_found_before_the_context_is_looked_at():
    capi, L = lib()
    ids = (C.c_int * 1)(0)
    amp = (C.c_float * 1)(1.0)
    refused(L, capi, L.fluid_noise_members(None, None, 1, capi.NOISE_SET, amp, 1, 0, 0), b"fluid_noise_members", b"fields")
    refused(L, capi, L.fluid_noise_members(None, ids, 1, capi.NOISE_ADD, None, 1, 0, 0), b"fluid_noise_members", b"amplitude")
    refused(L, capi, L.fluid_noise_dense(None, None, 4, 1.0, 1, 0, 0), b"fluid_noise_dense", b"out_dev")


def header_text():
    src = open(ROOT + "/include/fluid_amd.h").read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_signatures_carry_the_headers_types():
    capi, L = lib()
    ctype = {"fluid_ctx*": C.c_void_p, "int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "const int*": C.POINTER(C.c_int),
             "const float*": C.POINTER(C.c_float), "void*": C.c_void_p, "double*": C.POINTER(C.c_double),
             "unsigned long long": C.c_ulonglong, "unsigned int": C.c_uint}
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
        assert hasattr(L, name)
    assert re.search(r"enum\s*\{\s*FLUID_NOISE_SET\s*=\s*0\s*,\s*FLUID_NOISE_ADD\s*=\s*1\s*\}", src)
    assert (capi.NOISE_SET, capi.NOISE_ADD, capi.NOISE_DENSE_TAG, capi.NOISE_IDS) == (0, 1, DENSE_TAG, 65536)


def test_the_header_has_the_section_between_the_relaxation_and_the_jacobi_variant():
    raw, _ = header_text()
    section = raw.index("---- ensemble noise")
    assert raw.index("fluid_relax_spread(fluid_ctx") < section < raw.index("fluid_noise_members(fluid_ctx")
    assert raw.index("fluid_noise_members(fluid_ctx") < raw.index("fluid_noise_dense(fluid_ctx") < raw.index("fluid_noise_value(unsigned")
    assert raw.index("fluid_noise_value(unsigned") < raw.index("fluid_set_jacobi_variant(fluid_ctx")
    text = raw[section:raw.index("fluid_noise_members(fluid_ctx")]
    for word in ("Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "0x1.3988e1412ed76p-16", "APPROXIMATELY normal",
                 "6627e8d5 e169c58d bc57ac4c 9b00dbd8", "408f276d 41c83b0e a20bc7c6 6d5451fd", "d16cfe09 94fdcceb 5001e420 24126ea1"):
        assert word in text, word


def test_kernel_and_host_share_one_body():
    k = open(ROOT + "/fluidsimulationcuda_amd/csrc/fluid_noise.h").read()
    assert re.search(r"__host__ __device__ inline void philox4x32_10", k) and re.search(r"__host__ __device__ inline double noise_z", k)
    for src in ("fluid_noise.hip", "fluid_solver.hip"):
        text = open(ROOT + "/fluidsimulationcuda_amd/csrc/" + src).read()
        assert '#include "fluid_noise.h"' in text and "noise_z(" in text and "0xD2511F53" not in text, src


def test_solver_has_the_noise_calls():
    from fluidsimulationcuda_amd import FluidSolver
    p = inspect.signature(FluidSolver.noise).parameters
    assert list(p) == ["self", "fields", "amplitude", "seed", "sequence", "mode", "member_offset"], list(p)
    assert p["sequence"].default == 0 and p["mode"].default == 0 and p["member_offset"].default == 0
    p = inspect.signature(FluidSolver.noise_dense).parameters
    assert list(p) == ["self", "out", "amplitude", "seed", "sequence", "stream_id", "count", "wait"], list(p)
    p = inspect.signature(FluidSolver.perturb).parameters
    assert list(p) == ["self", "field", "scratch", "amplitude", "seed", "sequence", "alpha", "beta", "iters", "b"], list(p)
    assert p["b"].default == 0
    assert "member_moments" in FluidSolver.perturb.__doc__ and "rescale" in FluidSolver.perturb.__doc__


# ---- the statistics of the definition, on the model alone: n = 2^20 values per stream, fixed seeds.  Every bound is 5 / sqrt(n):
# five standard errors of a mean of n unit-variance values (the standard error of a sample variance of Irwin-Hall(8) values
# is sqrt((2 - 0.15) / n) = 1.36 / sqrt(n), of a correlation 1 / sqrt(n)) ----
STAT_W, STAT_M = 512, 4                   # 4 members of 512 x 512 cells = 2^20
STAT_SEED = 0x5EED0123456789AB


def corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))


def test_the_models_statistics():
    n = STAT_M * STAT_W * STAT_W
    assert n == 2 ** 20
    tol = 5.0 / np.sqrt(n)
    z = field_z(STAT_W, STAT_M, STAT_SEED, 3, 2)
    figures = {"mean": float(z.mean()), "variance - 1": float(z.var() - 1.0), "max |z|": float(np.abs(z).max()),
               "kurtosis": float(((z - z.mean()) ** 4).mean() / z.var() ** 2 - 3.0),
               "horizontal": corr(z[:, :, :-1], z[:, :, 1:]), "vertical": corr(z[:, :-1, :], z[:, 1:, :]),
               "members": corr(z[:-1], z[1:]),
               "fields": corr(z, field_z(STAT_W, STAT_M, STAT_SEED, 3, 3)),
               "sequences": corr(z, field_z(STAT_W, STAT_M, STAT_SEED, 4, 2))}
    print(figures, "tolerance", tol)
    assert abs(figures["mean"]) <= tol
    assert abs(figures["variance - 1"]) <= tol
    assert figures["max |z|"] <= 4.899
    for name in ("horizontal", "vertical", "members", "fields", "sequences"):
        assert abs(figures[name]) <= tol, (name, figures[name])
    # (not bounded by the issue; the definition says -0.15, its standard error at this n is about sqrt(24 / n) = 0.005)
    assert abs(figures["kurtosis"] + 0.15) <= 5 * np.sqrt(24.0 / n)
    s = halves_sum(philox(np.arange(4096), 0, 0, 0, 1, 2))
    assert s.min() >= 0 and s.max() <= 524280
