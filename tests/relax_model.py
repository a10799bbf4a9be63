"""The reference model of relaxation to prior spread (include/fluid_amd.h, "relaxation to prior spread"), in numpy float64,
shared by tests/test_relax_abi.py (CPU) and tests/test_gpu_relax.py (GPU).  numpy's double operations are IEEE and unfused
and np.sqrt is correctly rounded, so every line below is one rounding, in the order the header gives."""
import numpy as np

F32 = np.float32
F64 = np.float64


def narrow(y, storage):
    """what a store keeps: fp16 storage rounds once more, to nearest even"""
    with np.errstate(all="ignore"):
        return np.asarray(y, F32).astype(np.float16).astype(F32) if storage else np.asarray(y, F32)


def moments(x):
    """x: (M, W, W) float32, what the pack shows.  (mean_d, d, q) of fluid_ensemble_stats: both chains start from member
    0's term and run in member order."""
    xd = np.asarray(x, F32).astype(F64)
    members = xd.shape[0]
    with np.errstate(all="ignore"):
        s = xd[0].copy()
        for m in range(1, members):
            s = s + xd[m]
        mean = s / F64(members)
        d = xd - mean
        q = d[0] * d[0]
        for m in range(1, members):
            q = q + d[m] * d[m]
    return mean, d, q


def spread_model(x):
    """fluid_member_spread: (W, W) float32"""
    _, _, q = moments(x)
    with np.errstate(all="ignore"):
        return np.sqrt(q / F64(x.shape[0] - 1)).astype(F32)


def relax_model(x, prior, alpha, storage=0):
    """fluid_relax_spread on what the pack shows: (new members as the pack shows them, (W, W) bool of the cells stored).
    A cell with q == 0 or f == 1 is not stored and keeps what it held."""
    x = np.asarray(x, F32)
    mean, d, q = moments(x)
    with np.errstate(all="ignore"):
        sa = np.sqrt(q / F64(x.shape[0] - 1))
        sb = np.asarray(prior, F32).astype(F64)
        t = sb - sa
        t = F64(F32(alpha)) * t
        t = t / sa
        f = F64(1.0) + t
        stored = (q != 0) & (f != 1.0)                  # (a NaN q or f is stored: the cell becomes NaN)
        p = f * d
        y = narrow((mean + p).astype(F32), storage)
    return np.where(stored, y, x), stored


def property_inputs(n, members, storage, seed):
    """the property test's ensemble: values of order 1, spread of order 0.1, every cell and member different (fp16 storage:
    normal halves).  No cell's members lie within 2^-5 of each other all together: a cell must keep a spread when its
    anomalies are halved and rounded to halves -- a cell without one has nothing to relax (rule 3)."""
    rng = np.random.default_rng(seed)
    w = n + 2
    centre = rng.uniform(0.5, 1.5, (w, w)) * rng.choice([-1.0, 1.0], (w, w))
    x = narrow((centre + 0.1 * rng.standard_normal((members, w, w))).astype(F32), storage)
    while True:
        close = x.max(axis=0) - x.min(axis=0) < 2.0 ** -5
        if not close.any():
            return x
        x[:, close] = narrow((centre[close] + 0.1 * rng.standard_normal((members, int(close.sum())))).astype(F32), storage)


def property_bound(y, sd_b, storage):
    """|sd' - sd_b| <= eps * (max_m |y_m| + sd_b): eps = 2^-23 (fp16 storage: 2^-10), the issue's bound"""
    eps = 2.0 ** -10 if storage else 2.0 ** -23
    return eps * (np.abs(np.asarray(y, F32).astype(F64)).max(axis=0) + np.asarray(sd_b, F32).astype(F64))
