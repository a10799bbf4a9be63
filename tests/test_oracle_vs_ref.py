"""CPU: the restatement against the reference itself on seeded random inputs --
every operator on its own, and whole steps from the reference's own
initializeParameters.  The reference's outputs are pinned by the CRC-32 of
their bytes in tests/golden/oracle_vs_ref.json, which tests/golden/make_golden.py
records by running the recipes below on the compiled reference
(oracle/_ref/*.so); here the restatement runs the same recipes and must
reproduce every checksum, so neither the reference nor its build is needed."""
import json
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, rnd
from oracle.oracle import DIFF, DT, VISC

CHECKSUMS = os.path.join(GOLDEN, "oracle_vs_ref.json")
OPERATOR_SIZES = [14, 30, 61, 126]
STEP_CASES = [(30, 40), (61, 40), (126, 40), (126, 20), (254, 40)]
FIELDS = ("dens", "dens_prev", "u", "u_prev", "v", "v_prev")      # initializeParameters' order


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.float32).view(np.uint8).reshape(-1))


def each_operator(eng, n, coefficients, stale):
    """(label, CRC-32) of every operator's output on inputs drawn from PCG64 seed n, then ("inputs", CRC-32 of every
    array drawn, as drawn).  `eng` is the reference or the restatement (same method names and argument order).  Each
    advect writes into one of a freshly drawn pair -- the first for `stale` 0, the second for 1 -- so the recorded run
    and the checked one start from different stale contents."""
    rng = np.random.default_rng(n)
    drawn = [0]

    def draw(lo=-1.0, hi=1.0):
        a = rnd(rng, n, lo, hi)
        drawn[0] = zlib.crc32(a.view(np.uint8).reshape(-1), drawn[0])
        return a

    for b in (0, 1, 2):
        x = draw()
        eng.set_bnd(b, x)
        yield "set_bnd b=%d" % b, crc(x)
    x, s = draw(), draw()
    eng.add_source(x, s)
    yield "add_source", crc(x)
    for b, coef in ((1, VISC), (2, VISC), (0, DIFF), (0, None)):
        a, be = (1.0, 4.0) if coef is None else coefficients(n, DT, coef)
        x, x0 = draw(), draw()
        eng.diffuse(b, x, x0.copy(), a, be)
        yield "diffuse b=%d %s" % (b, "pressure" if coef is None else "coef=%g" % coef), crc(x)
    u, v = draw(), draw()
    p, d = draw(), draw()
    eng.divergence(u, v, p, d)
    yield "p", crc(p)
    yield "div", crc(d)
    pr = draw()
    eng.subtract_gradient(u, v, pr)
    yield "grad u", crc(u)
    yield "grad v", crc(v)
    for amp in (0.01, 1.0, 4.0 / DT):
        u, v, d0 = draw(-amp, amp), draw(-amp, amp), draw()
        for b in (0, 1, 2):
            d = (draw(), draw())[stale]
            eng.advect(b, d, d0, u, v)
            yield "advect amp=%g b=%d" % (amp, b), crc(d)
    yield "inputs", drawn[0]


def steps_from_reference_init(eng, steps=3):
    """(label, CRC-32) of the six fields initializeParameters draws (glibc rand, seed 1), then of all six after each of
    `steps` steps of the reference's loop, the first with the sources.  `eng`: initialize(), step_src(), step() as the
    oracle.Reference class has them."""
    fs = eng.initialize()
    for name, f in zip(FIELDS, fs):
        yield "initializeParameters %s" % name, crc(f)
    dens, dens0, u, u0, v, v0 = fs
    for z in range(1, steps + 1):
        (eng.step_src if z == 1 else eng.step)(u, v, dens, u0, v0, dens0)
        for name, f in zip(FIELDS, fs):
            yield "%s after step %d" % (name, z), crc(f)


class Restatement:
    """The oracle behind the interface of oracle.Reference for one sweep count."""

    def __init__(self, oracle, n, iters):
        self.oracle, self.n, self.iters = oracle, n, iters

    def initialize(self):
        return self.oracle.initialize_glibc(self.n)

    def step_src(self, *fields):
        self.oracle.step_src(*fields, iters=self.iters)

    def step(self, *fields):
        self.oracle.step(*fields, iters=self.iters)


@pytest.fixture(scope="module")
def recorded():
    with open(CHECKSUMS) as f:
        return json.load(f)


def check(got, want, what):
    got = dict(got)
    assert list(got) == list(want), "%s: the recipe's outputs are not the recorded ones" % what
    assert got.get("inputs") == want.get("inputs"), "%s: the inputs drawn are not those the checksums were recorded on" % what
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, "%s: the restatement's bytes differ from the reference's in %s" % (what, ", ".join(bad))


@pytest.mark.parametrize("n", OPERATOR_SIZES)
def test_each_operator(oracle, recorded, n):
    check(each_operator(oracle, n, oracle.coefficients, stale=1), recorded["each_operator"][str(n)], "N=%d" % n)


@pytest.mark.parametrize("n,iters", STEP_CASES)
def test_steps_from_reference_init(oracle, recorded, n, iters):
    check(steps_from_reference_init(Restatement(oracle, n, iters)), recorded["steps"]["%d:%d" % (n, iters)],
          "N=%d, %d sweeps" % (n, iters))


def test_portable_init_shape(oracle):
    """The portable generator follows the same recipe as initializeParameters
    (FluidSequential.c:244-271): density only in the centred square, velocities
    k/100 everywhere, current fields zero."""
    n = 62
    dens, dens0, u, u0, v, v0 = oracle.initialize_portable(n, seed=1)
    w, c, r = n + 2, (n + 2) // 2, (n + 2) // 8
    mask = np.zeros((w, w), bool)
    mask[c - r:c + r, c - r:c + r] = True
    assert (dens0[~mask] == 0).all() and dens0[mask].max() < 0.1
    assert not u.any() and not v.any() and not dens.any()
    for f in (u0, v0):
        k = np.rint(f * 100)
        assert np.array_equal((k / 100.0).astype(np.float32), f) and k.min() >= 0 and k.max() <= 99
