"""The reference model of screening observations (include/fluid_amd.h, "screening observations"), in numpy float64, shared by
tests/test_qc_abi.py (CPU) and tests/test_gpu_qc.py (GPU).  numpy's double operations are IEEE and unfused and np.sqrt is
correctly rounded, so every line below is one rounding, in the order the header gives."""
import numpy as np

F32 = np.float32
F64 = np.float64
CHUNK = 64          # points per chunk of the sums
LANES = 16          # lanes of the fold


def moments(h):
    """rule 2.  h: (M, P) float32.  (mean_d, var): both chains start from member 0's term and run in member order."""
    hd = np.asarray(h, F32).astype(F64)
    members = hd.shape[0]
    with np.errstate(all="ignore"):
        s = hd[0].copy()
        for m in range(1, members):
            s = s + hd[m]
        mean = s / F64(members)
        e = hd[0] - mean
        q = e * e
        for m in range(1, members):
            e = hd[m] - mean
            ee = e * e
            q = q + ee
        var = q / F64(members - 1)
    return mean, var


def chunk_sum(terms, keep):
    """one sum of the header: the kept terms of every chunk of 64 points in increasing point index, from the first one (-0.0
    for a chunk without one); lane j of 16 chains the chunks j, j + 16, .. from -0.0; the 16 sums in index order"""
    terms, keep = np.asarray(terms, F64), np.asarray(keep, bool)
    chunks = []
    with np.errstate(all="ignore"):
        for c in range(0, terms.size, CHUNK):
            s = F64(-0.0)
            for t in terms[c:c + CHUNK][keep[c:c + CHUNK]]:
                s = s + t                                   # (-0.0 + t has the bits of t: "from the first term")
            chunks.append(s)
        lanes = []
        for j in range(LANES):
            s = F64(-0.0)
            for v in chunks[j::LANES]:
                s = s + v
            lanes.append(s)
        s = lanes[0]
        for v in lanes[1:]:
            s = s + v
    return s


def screen(h, obs=None, inv_sigma=None, threshold=0.0):
    """fluid_observation_departures on the observations h (M, P): a dict of mean, spread (float32) and, with obs, departure
    (float32), rank, flag (uint8), sums (float64[3]), d and vs (float64, the terms of the sums)."""
    h = np.asarray(h, F32)
    members, points = h.shape
    mean, var = moments(h)
    with np.errstate(all="ignore"):
        out = {"mean": mean.astype(F32), "spread": np.sqrt(var).astype(F32)}
        if obs is None:
            return out
        y = np.asarray(obs, F32)
        sg = np.ones(points, F64) if inv_sigma is None else np.asarray(inv_sigma, F32).astype(F64)
        dep = y.astype(F64) - mean                          # rule 3
        d = dep * sg
        lhs = d * d                                         # rule 4
        vs = var * sg
        vs = vs * sg
        bound = F64(1.0) + vs
        t2 = F64(F32(threshold)) * F64(F32(threshold))
        lim = t2 * bound
        rejected = (lhs > lim) & (F32(threshold) != 0)      # (a comparison with a NaN is false)
        rank = (h < y[None, :]).sum(axis=0)                 # rule 5, as floats
    keep = ~rejected
    out.update(departure=dep.astype(F32), rank=rank.astype(np.uint8), flag=rejected.astype(np.uint8), d=d, vs=vs,
               sums=np.array([chunk_sum(np.ones(points), keep), chunk_sum(lhs, keep), chunk_sum(vs, keep)], F64))
    return out


def gated_inv_sigma(h, obs, inv_sigma, threshold):
    """what a gated call proceeds with: inv_sigma (all ones for None) with +0.0 at the rejected points; and the flags"""
    flag = screen(h, obs, inv_sigma, threshold)["flag"]
    s = np.ones(np.asarray(h).shape[1], F32) if inv_sigma is None else np.asarray(inv_sigma, F32).copy()
    s[flag != 0] = F32(0.0)
    return s, flag
