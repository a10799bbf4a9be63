#!/usr/bin/env python3
"""Block-averaged ensemble snapshots (fluid_pack_members_coarse, fluid_download_members_coarse): what the coarse pack costs
beside the dense pack of the same field, measured in the same process.

Per (N, M), storage type and coarse factor r, uniform random fields in every member, by the method of
tools/ensemble_io_timing.py (events on the stream the library shares with this tool -- the constructor's stream=,
wait=False --, one untimed call first, median over --repeats, clocks as found):
- device time of the coarse pack of one field, and its effective bandwidth against the compulsory bytes,
  sizeof(S) + 4 / r^2 per cell (one stored element read, one float written per r x r cells);
- device time of the dense fluid_pack_members of the same field -- the yardstick -- against its sizeof(S) + 4 per cell;
  the dense pack is timed again after the factors, so that a drift of the clocks during the case shows;
- wall time of download_members(coarse=r) beside download_members, median over --host-repeats.
The condition the coarse pack is held to follows from the bytes: fp32 storage, N = 4094, M = 4, every r >= 4 -- no longer than
the dense pack measured beside it; `condition_met` of those rows says so.

Prints a table and writes JSON (--out).
    python tools/ensemble_coarse_timing.py [--cases 1024x16,4094x4] [--storage f32,f16] [--out profiles/ensemble_coarse_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluidsimulationcuda_amd as F  # noqa: E402
from fluidsimulationcuda_amd import capi  # noqa: E402

DEFAULT_CASES = "1024x16,4094x4"


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


def wall_ms(s, call, repeats):
    call()
    out = []
    for _ in range(repeats):
        s.synchronize()
        t0 = time.perf_counter()
        call()
        s.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def timed(torch, stream, call, repeats, nbytes):
    ms, lo, hi = device_ms(torch, stream, call, repeats)
    return {"device_ms": ms, "min_ms": lo, "max_ms": hi, "compulsory_bytes": nbytes, "gb_per_s": nbytes / (ms * 1e-3) / 1e9}


def run(n, members, storage, repeats, host_repeats):
    import torch
    w, esz = n + 2, 2 if storage else 4
    cells = members * w * w
    rng = np.random.default_rng(n + members)
    stream = torch.cuda.Stream()
    row = {"n": n, "grid": w, "members": members, "storage": "f16" if storage else "f32", "factors": []}
    with torch.cuda.stream(stream), F.FluidSolver(n, members=members, storage=storage, stream=stream.cuda_stream) as s:
        host = rng.uniform(-1, 1, size=(members, w, w)).astype(np.float32)
        s.upload_members(u=host)
        dense = torch.empty((members, w, w), dtype=torch.float32, device="cuda")
        row["dense_pack"] = timed(torch, stream, lambda: s.pack("u", out=dense, wait=False), repeats, cells * (esz + 4))
        row["download_members_ms"] = wall_ms(s, lambda: s.download_members("u", out=host), host_repeats)
        for r in capi.COARSE_FACTORS:
            if w % r:
                continue
            c = w // r
            out = torch.empty((members, c, c), dtype=torch.float32, device="cuda")
            f = timed(torch, stream, lambda: s.pack("u", out=out, wait=False, coarse=r), repeats, cells * esz + members * c * c * 4)
            f["factor"] = r
            f["over_dense"] = f["device_ms"] / row["dense_pack"]["device_ms"]
            small = np.empty((members, c, c), np.float32)
            f["download_members_ms"] = wall_ms(s, lambda: s.download_members("u", out=small, coarse=r), host_repeats)
            row["factors"].append(f)
        row["dense_pack_again"] = timed(torch, stream, lambda: s.pack("u", out=dense, wait=False), repeats, cells * (esz + 4))
    dense_ms = min(row["dense_pack"]["device_ms"], row["dense_pack_again"]["device_ms"])       # the faster of the two: the stricter yardstick
    for f in row["factors"]:
        if not storage and n == 4094 and members == 4 and f["factor"] >= 4:
            f["condition_met"] = f["device_ms"] <= dense_ms
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="NxM, comma separated")
    ap.add_argument("--storage", default="f32,f16")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    rows = []
    for storage in args.storage.split(","):
        for case in args.cases.split(","):
            n, members = (int(v) for v in case.split("x"))
            row = run(n, members, 1 if storage == "f16" else 0, args.repeats, args.host_repeats)
            rows.append(row)
            d, d2 = row["dense_pack"], row["dense_pack_again"]
            print("N=%5d M=%3d %s  dense pack %8.3f ms %7.1f GB/s (again %8.3f ms)  download_members %9.2f ms" % (
                n, members, storage, d["device_ms"], d["gb_per_s"], d2["device_ms"], row["download_members_ms"]), flush=True)
            for f in row["factors"]:
                print("    r=%2d  coarse pack %8.3f ms [%7.3f .. %7.3f] %7.1f GB/s  %5.2f x dense  download_members %9.2f ms%s" % (
                    f["factor"], f["device_ms"], f["min_ms"], f["max_ms"], f["gb_per_s"], f["over_dense"], f["download_members_ms"],
                    "" if "condition_met" not in f else "  condition %s" % ("met" if f["condition_met"] else "MISSED")), flush=True)
    out = {"tool": "tools/ensemble_coarse_timing.py", "commit": args.commit, "repeats": args.repeats, "host_repeats": args.host_repeats, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
