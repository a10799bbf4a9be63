"""The reference model of "ensemble products" (include/fluid_amd.h: fluid_quantile_position, fluid_member_quantiles,
fluid_member_exceedance): the header's rules in numpy float64, vectorised over the cells -- np.sort along the member axis for
the order statistics, the three double operations of the interpolation one at a time and in the header's order, the
exceedance as integer counts.  The inputs come from tests/verify_model.py (random_inputs: ties in every eighth cell, offsets
up to 100, both storage types), so the CPU and the GPU tests see the very same numbers."""
import math

import numpy as np

from verify_model import F32, F64, random_inputs

MAX_MEMBERS, MAX_LEVELS = 64, 16
ABOVE, BELOW = 0, 1
# the levels of the tests: both ends, the envelope, the quartiles, one that is no dyadic fraction, the median
LEVELS = (0.0, 0.05, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.9, 0.95, 1.0)


def quantile_position(members, level):
    """(lo, frac) in Python floats, which are IEEE doubles: h = (double)(float)level * (members - 1), exact"""
    assert 1 <= members <= MAX_MEMBERS
    level = float(F32(level))
    assert math.isfinite(level) and 0.0 <= level <= 1.0
    h = level * float(members - 1)
    lo = int(math.floor(h))
    frac = h - float(lo)
    if lo >= members - 1:
        lo, frac = members - 1, 0.0
    return lo, frac


def sorted_members(x):
    """rule 1: -0 counts as +0, then the order statistics, as float32"""
    with np.errstate(all="ignore"):
        return np.sort(np.asarray(x, F32) + F32(0.0), axis=0)


def quantiles(x, levels):
    """x (M, ...) float32 as the pack shows it -> (nlevels, ...) float32: rules 1 - 3"""
    x = np.asarray(x, F32)
    M = x.shape[0]
    s = sorted_members(x)
    finite = np.isfinite(x).all(axis=0)
    out = np.empty((len(levels),) + x.shape[1:], F32)
    with np.errstate(all="ignore"):
        for l, level in enumerate(levels):
            lo, frac = quantile_position(M, level)
            if frac == 0.0:
                q = s[lo].copy()
            else:
                a, b = s[lo].astype(F64), s[lo + 1].astype(F64)
                d = b - a
                t = F64(frac) * d
                q = (a + t).astype(F32)
            out[l] = np.where(finite, q, F32(np.nan))
    return out


def exceedance(x, thresholds, mode=ABOVE):
    """x (M, ...) float32 -> (nthresholds, ...) float32: integer counts, one double division, one narrowing"""
    x = np.asarray(x, F32)
    M = x.shape[0]
    out = np.empty((len(thresholds),) + x.shape[1:], F32)
    with np.errstate(all="ignore"):
        for l, t in enumerate(thresholds):
            t = F32(t)
            count = ((x < t) if mode == BELOW else (x > t)).sum(axis=0).astype(np.int64)
            out[l] = (count.astype(F64) / F64(M)).astype(F32)
    return out


def inputs(n, members, storage, seed):
    """x (M, W, W): the members of verify_model.random_inputs; for M = 1 the first member of a two-member draw"""
    x, _ = random_inputs(n, max(members, 2), storage, seed)
    return np.ascontiguousarray(x[:members])
