"""The reference model of "verifying ensembles" (include/fluid_amd.h, fluid_verify_members): the header's rules in numpy
float64, vectorised over the cells and looped over the members -- every operation one IEEE double operation, in the header's
order -- np.sort along the member axis for the order statistics, and math.fsum for the reference sums.  Also the inputs the
CPU and GPU tests share, so that every bound is checked on the CPU against the model, on the very numbers the GPU sees."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
SUMS, MAX_MEMBERS = 5, 64
ROW = SUMS + MAX_MEMBERS + 1
EPS = 2.0 ** -53


def narrow(x, storage):
    """what a field of the storage type holds after an upload: fp16 storage rounds once, to nearest even"""
    x = np.asarray(x, F32)
    return x.astype(np.float16).astype(F32) if storage else x


def cell_scores(x, y, fair=False):
    """rules 1 - 5 per cell: x (M, ...) float32 as the pack shows it, y (...) float32 -> dict of float64 arrays e, se, var,
    crps and the int rank"""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    M = x.shape[0]
    assert 2 <= M <= MAX_MEMBERS and x.shape[1:] == y.shape
    with np.errstate(all="ignore"):
        xd, yd = x.astype(F64), y.astype(F64)
        s = xd[0].copy()
        for m in range(1, M):
            s = s + xd[m]
        mean = s / F64(M)
        d = xd[0] - mean
        q = d * d
        for m in range(1, M):
            d = xd[m] - mean
            q = q + d * d
        var = q / F64(M - 1)
        e = mean - yd
        se = e * e
        # rule 3: -0 counts as +0, then the order statistics
        xs = np.sort(x + F32(0.0), axis=0).astype(F64)
        yc = (y + F32(0.0)).astype(F64)
        a = np.abs(xs[0] - yc)
        g = F64(1 - M) * xs[0]
        for i in range(2, M + 1):
            a = a + np.abs(xs[i - 1] - yc)
            g = g + F64(2 * i - M - 1) * xs[i - 1]
        t1 = a / F64(M)
        t2 = g / F64(M * (M - 1) if fair else M * M)
        crps = t1 - t2
        finite = np.isfinite(x).all(axis=0) & np.isfinite(y)
        crps = np.where(finite, crps, np.nan)
        rank = (x < y).sum(axis=0)
    return {"e": e, "se": se, "var": var, "crps": crps, "rank": rank.astype(np.int64)}


def interior(n):
    return (1, n + 1, 1, n + 1)


def in_box(a, box):
    return a[..., box[0]:box[1], box[2]:box[3]]


def score_row(c, box, members):
    """the score row of the cells of `box` from cell_scores' result on the whole (W, W) array: ROW float64, the four sums by
    math.fsum (a NaN or an infinite term: what numpy's sum gives -- only its kind is compared)"""
    row = np.zeros(ROW, F64)
    cells = in_box(c["rank"], box).size
    row[0] = cells
    for k, name in enumerate(("e", "se", "var", "crps")):
        t = in_box(c[name], box).ravel()
        row[1 + k] = math.fsum(t) if np.isfinite(t).all() else t.sum()
    row[SUMS:SUMS + members + 1] = np.bincount(in_box(c["rank"], box).ravel(), minlength=members + 1)
    return row


def sum_bounds(c, box):
    """n * 2^-53 * sum |terms| for each of the four sums: the bound for summing n doubles in any order (valid while n (n - 1)
    2^-53 <= 1)"""
    n = in_box(c["rank"], box).size
    assert n * (n - 1) * EPS <= 1.0
    return [n * EPS * math.fsum(np.abs(in_box(c[name], box)).ravel()) for name in ("e", "se", "var", "crps")]


def crps_pairwise(x, y, fair=False):
    """the O(M^2) definition in float64: (1/M) sum |x_m - y| - (1 / 2 M^2) sum sum |x_m - x_k| (fair: 1 / 2 M (M - 1))"""
    xd, yd = np.asarray(x, F32).astype(F64), np.asarray(y, F32).astype(F64)
    M = xd.shape[0]
    a = np.zeros(yd.shape, F64)
    p = np.zeros(yd.shape, F64)
    for m in range(M):
        a = a + np.abs(xd[m] - yd)
        for k in range(M):
            p = p + np.abs(xd[m] - xd[k])
    return a / M - p / (2.0 * (M * (M - 1) if fair else M * M))


def pairwise_bound(x, y):
    """(M^2 + 4 M) 2^-53 (max |x_k| + |y|) per cell: the rounding of both forms"""
    M = x.shape[0]
    return (M * M + 4 * M) * EPS * (np.abs(np.asarray(x, F64)).max(axis=0) + np.abs(np.asarray(y, F64)))


# ---- the inputs the CPU and the GPU tests share ----------------------------------------------------------------------------------
def random_inputs(n, members, storage, seed):
    """(x (M, W, W), y (W, W)): values over some binades around per-cell offsets up to 100, both signs, and in every eighth
    cell ties among the members or a truth equal to a member"""
    rng = np.random.default_rng(seed)
    w = n + 2
    lo, hi = (-6, 2) if storage else (-12, 4)
    off = rng.uniform(-100.0, 100.0, (w, w)) * (rng.uniform(size=(w, w)) < 0.5)
    if storage:
        off = off / 16.0
    x = off + np.ldexp(rng.uniform(1.0, 2.0, (members, w, w)), rng.integers(lo, hi, (w, w))) * rng.choice([-1.0, 1.0], (members, w, w))
    x = narrow(x.astype(F32), storage)
    y = (off + np.ldexp(rng.uniform(1.0, 2.0, (w, w)), rng.integers(lo, hi, (w, w))) * rng.choice([-1.0, 1.0], (w, w))).astype(F32)
    tie = rng.uniform(size=(w, w)) < 0.125
    x[1][tie] = x[0][tie]
    if members > 2:
        x[members - 1][tie] = x[0][tie]
    eq = rng.uniform(size=(w, w)) < 0.125
    y[eq] = x[members // 2][eq]
    return x, y


def dyadic_inputs(n, members, seed):
    """multiples of 2^-6 with |x| <= 8: at M = 2, 8, 64 the mean, e, se and the CRPS without FLUID_VERIFY_FAIR are exact
    dyadic numbers of few bits, and so is every partial sum of them in any order"""
    rng = np.random.default_rng(seed)
    w = n + 2
    x = (rng.integers(-512, 513, (members, w, w)) / 64.0).astype(F32)
    y = (rng.integers(-512, 513, (w, w)) / 64.0).astype(F32)
    return x, y


def recursive_sums(t):
    """forward, reverse and pairwise recursive summation of a vector in float64"""
    t = np.asarray(t, F64).ravel()
    fwd = F64(0.0)
    for v in t:
        fwd = fwd + v
    rev = F64(0.0)
    for v in t[::-1]:
        rev = rev + v

    def pair(a):
        return a[0] if a.size == 1 else pair(a[:a.size // 2]) + pair(a[a.size // 2:])
    return float(fwd), float(rev), float(pair(t))
