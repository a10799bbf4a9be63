#!/usr/bin/env python3
"""Localised updates (fluid_transform_members_local, fluid_taper_gaspari_cohn): what the tapered increment costs beside the
plain transform, and how its cost follows the box, measured in the same process.

Per (N, M) and storage type, uniform random values in every member of one field, by the method of
tools/ensemble_transform_timing.py (events on the stream the library shares with this tool -- the constructor's stream=;
the calls go to the C entry point directly, so nothing between the events waits --, one untimed call first, median over
--repeats, clocks as found).  The increments are D = Q - I with an orthogonal Q, none of them zero (the table where every
term is taken): with a taper in [0, 1] the values stay where they are over the repeats.
- (a) a null taper and a null box against fluid_transform_members with Q on the same context, the plain transform measured
  before and after so that a drift of the clocks shows.  The local kernel reads every member twice (the walk, and x_m again
  before its store) and writes it once: the expectation is a time within that of one more read of the field, that is at
  most 1.5 times the plain transform's; `over_transform` is the ratio against the faster of the two plain measurements.
- (b) the Gaspari-Cohn taper of half-width c = N / 32 about the middle of the grid, with the box the taper call returns:
  the expectation is a time that follows the box area (`box_share` of the array) and not the grid.
- (c) the same taper with a null box: every wave loads its taper values, the ones that find only zeros leave at once.
  What the early exit costs per cell outside the support.
Compulsory bytes: one read and one write of the stored cells of every member, plus the taper's floats where it is read.
Nothing is asserted.  Prints a table and writes JSON (--out).
    python tools/ensemble_local_timing.py [--cases 1024x8,4096x64] [--storage f32,f16] [--out profiles/ensemble_local_timing.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluidsimulationcuda_amd as F  # noqa: E402
from fluidsimulationcuda_amd import capi  # noqa: E402

DEFAULT_CASES = "1024x8,1024x32,1024x64,4096x8,4096x32,4096x64"


def device_ms(torch, stream, call, repeats):
    call()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def timed(torch, stream, call, repeats, nbytes):
    ms, lo, hi = device_ms(torch, stream, call, repeats)
    return {"device_ms": ms, "min_ms": lo, "max_ms": hi, "compulsory_bytes": nbytes, "gb_per_s": nbytes / (ms * 1e-3) / 1e9}


def run(n, members, storage, repeats):
    import torch
    w, esz = n + 2, 2 if storage else 4
    cells = members * w * w
    rng = np.random.default_rng(n + members)
    stream = torch.cuda.Stream()
    row = {"n": n, "grid": w, "members": members, "storage": "f16" if storage else "f32"}
    with torch.cuda.stream(stream), F.FluidSolver(n, members=members, storage=storage, stream=stream.cuda_stream) as s:
        base = rng.uniform(-1, 1, size=(w, w)).astype(np.float32)
        for m in range(members):                 # (member by member, each a shifted copy: no dense ensemble on the host)
            s.upload(member=m, u=np.roll(base, 17 * m + 1, axis=0))
        q = np.linalg.qr(rng.normal(size=(members, members)))[0].astype(np.float32)
        q[q == 0] = 1e-3
        d = (q - np.eye(members, dtype=np.float32)).astype(np.float32)
        d[d == 0] = 1e-3
        ids = (C.c_int * 1)(capi.U)
        dp = d.ctypes.data_as(capi._MF)
        L = capi.lib()

        def local(taper, box):
            capi.check(L.fluid_transform_members_local(s._h, ids, 1, dp, taper, box))

        def plain():
            s.transform(q, fields=("u",))

        taper, tbox = s.taper_gaspari_cohn((n + 1) / 2.0, (n + 1) / 2.0, n / 32.0)
        box = (C.c_int * 4)(*tbox)
        area = (tbox[1] - tbox[0]) * (tbox[3] - tbox[2])
        support = int((taper != 0).sum().item())
        stream.synchronize()
        row["box"] = list(tbox)
        row["box_share"] = area / float(w * w)
        row["support_cells"] = support
        row["transform"] = timed(torch, stream, plain, repeats, 2 * cells * esz)
        row["local_full"] = timed(torch, stream, lambda: local(None, None), repeats, 2 * cells * esz)
        row["transform_again"] = timed(torch, stream, plain, repeats, 2 * cells * esz)
        row["local_box"] = timed(torch, stream, lambda: local(taper.data_ptr(), box), repeats, 2 * members * support * esz + 4 * area)
        row["local_null_box"] = timed(torch, stream, lambda: local(taper.data_ptr(), None), repeats, 2 * members * support * esz + 4 * w * w)
    floor_ms = min(row["transform"]["device_ms"], row["transform_again"]["device_ms"])          # the faster: the stricter yardstick
    row["local_full"]["over_transform"] = row["local_full"]["device_ms"] / floor_ms
    row["local_box"]["over_local_full"] = row["local_box"]["device_ms"] / row["local_full"]["device_ms"]
    row["local_null_box"]["over_local_box"] = row["local_null_box"]["device_ms"] / row["local_box"]["device_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="NxM, comma separated")
    ap.add_argument("--storage", default="f32,f16")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    rows = []
    for storage in args.storage.split(","):
        for case in args.cases.split(","):
            n, members = (int(v) for v in case.split("x"))
            row = run(n, members, 1 if storage == "f16" else 0, args.repeats)
            rows.append(row)
            tr, tr2, a, b, c = (row[k] for k in ("transform", "transform_again", "local_full", "local_box", "local_null_box"))
            print("N=%5d M=%3d %s  transform %8.3f ms (again %8.3f ms) | (a) null taper, null box %8.3f ms [%7.3f .. %7.3f] %7.1f GB/s %5.2f x "
                  "transform | (b) taper, its box (%5.2f%% of the array) %8.3f ms %6.4f x (a) | (c) taper, null box %8.3f ms %5.2f x (b)" % (
                      n, members, storage, tr["device_ms"], tr2["device_ms"], a["device_ms"], a["min_ms"], a["max_ms"], a["gb_per_s"],
                      a["over_transform"], 100 * row["box_share"], b["device_ms"], b["over_local_full"], c["device_ms"],
                      c["over_local_box"]), flush=True)
    out = {"tool": "tools/ensemble_local_timing.py", "commit": args.commit, "repeats": args.repeats, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
