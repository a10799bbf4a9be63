#!/usr/bin/env python3
"""Ensemble products (fluid_member_quantiles, fluid_member_exceedance): what one call costs beside one read of the members by
unchanged code, and beside the route a caller had before them -- pack, torch.sort, the interpolation in torch on the device --
measured in the same process.

Per row (N, M, storage): one field (dens), uniform random values on a mean of 50 in every member, made on the device and
unpacked.  The library and torch share one stream; what is measured is the time between two events on it, around work that
nothing waits inside of; the median over the repeats after one untimed call, the sides alternating.
- (a) quantiles:   quantiles("dens", levels, out=q, wait=False) with 3 levels (5 %, median, 95 %) and with 9;
- (b) exceedance:  exceedance("dens", thresholds, out=e, wait=False) with 1 threshold and with 4;
- (c) route:       pack -> torch.sort over the members -> the 3 levels by the same positions, interpolated in float32: what a
                   caller would write, NOT the double arithmetic of the call (no defined bits).  `route_peak_extra_bytes`:
                   torch's peak allocation above what was allocated before the route began.
- (d) spread:      spread(("dens",), out=sd, wait=False): fluid_member_spread, code these calls do not touch, which reads the
                   same members once and writes one float per cell -- the yardstick for "one read of the members" (M >= 2).
Recorded, not gated: `ratio_quantiles_to_spread` = (a, 3 levels) / (d), `ratio_exceedance_to_spread` = (b, 1 threshold) / (d),
`ratio_route_to_quantiles` = (c) / (a, 3 levels); and the calls' bytes per second against the traffic of the definition, per
cell esz * M bytes read and 4 bytes written per level (`moved`: esz is 2 with fp16 storage).
Every row runs in a child process under a time limit of its own (--limit seconds).

    python tools/ensemble_quantile_timing.py [--out profiles/ensemble_quantile_timing.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_CASES = "1022x8,1022x16,1022x64,4094x8,4094x16,4094x64"
FIELD = "dens"
LEVELS3 = (0.05, 0.5, 0.95)
LEVELS9 = (0.05, 0.1, 0.25, 1.0 / 3.0, 0.5, 2.0 / 3.0, 0.75, 0.9, 0.95)
THRESHOLDS1 = (50.5,)
THRESHOLDS4 = (50.1, 50.25, 50.5, 50.9)


def run(n, members, storage, repeats):
    import torch
    import fluidsimulationcuda_amd as F
    w = n + 2
    stream = torch.cuda.Stream()
    row = {"n": n, "members": members, "storage": "f16" if storage else "f32", "fields": 1}
    with torch.cuda.stream(stream), F.FluidSolver(n, members=members, storage=storage, stream=stream.cuda_stream) as s:
        for m in range(members):                             # (member by member: no M * W * W temporary beside the arena)
            s.unpack(FIELD, torch.rand((1, w, w), dtype=torch.float32, device="cuda") + 50.0, first=m, count=1, wait=False)
        q3 = torch.zeros((3, w, w), dtype=torch.float32, device="cuda")
        q9 = torch.zeros((9, w, w), dtype=torch.float32, device="cuda")
        e1 = torch.zeros((1, w, w), dtype=torch.float32, device="cuda")
        e4 = torch.zeros((4, w, w), dtype=torch.float32, device="cuda")
        sd = torch.zeros((1, w, w), dtype=torch.float32, device="cuda")
        positions = [F.quantile_position(members, level) for level in LEVELS3]
        kept = {}

        def route():
            x = s.pack(FIELD, wait=False)
            xs, _ = torch.sort(x, dim=0)
            kept["q"] = torch.stack([xs[lo] if frac == 0.0 else torch.lerp(xs[lo], xs[lo + 1], frac) for lo, frac in positions])

        def timed(call):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            call()
            t1.record(stream)
            t1.synchronize()
            return t0.elapsed_time(t1)

        sides = {"quantiles3": lambda: s.quantiles(FIELD, LEVELS3, out=q3, wait=False),
                 "quantiles9": lambda: s.quantiles(FIELD, LEVELS9, out=q9, wait=False),
                 "exceedance1": lambda: s.exceedance(FIELD, THRESHOLDS1, out=e1, wait=False),
                 "exceedance4": lambda: s.exceedance(FIELD, THRESHOLDS4, out=e4, wait=False),
                 "spread": lambda: s.spread((FIELD,), out=sd, wait=False),
                 "route": route}
        times = {k: [] for k in sides}
        for k, call in sides.items():
            timed(call)                                  # untimed: code objects, torch's allocator
        for _ in range(repeats):
            for k, call in sides.items():                # alternating
                times[k].append(timed(call))
        for k, v in times.items():
            row[k] = {"ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
        # the route's peak extra memory
        stream.synchronize()
        kept.clear()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        route()
        stream.synchronize()
        row["route_peak_extra_bytes"] = int(torch.cuda.max_memory_allocated() - base)
        # the call gives what the route gives (float algebra against double: no bits, a tolerance of float rounding)
        sides["quantiles3"]()
        sides["exceedance1"]()
        stream.synchronize()
        row["max_abs_difference_to_route"] = float((q3 - kept["q"]).abs().max())
        row["median_of_cell_0_0"] = float(q3[1, 0, 0])
        row["mean_exceedance"] = float(e1.mean())
    esz = 2 if storage else 4
    for k, levels in (("quantiles3", 3), ("quantiles9", 9), ("exceedance1", 1), ("exceedance4", 4)):
        row[k]["moved_bytes"] = w * w * (esz * members + 4 * levels)
        row[k]["moved_gb_per_s"] = row[k]["moved_bytes"] / row[k]["ms"] * 1e-6
    row["ratio_quantiles_to_spread"] = row["quantiles3"]["ms"] / row["spread"]["ms"]
    row["ratio_exceedance_to_spread"] = row["exceedance1"]["ms"] / row["spread"]["ms"]
    row["ratio_route_to_quantiles"] = row["route"]["ms"] / row["quantiles3"]["ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="NxM, comma separated; each with fp32 and fp16 storage")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--limit", type=int, default=120, help="seconds one row may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="")
    ap.add_argument("--date", default="")
    ap.add_argument("--row", default="", help="(internal) N,M,storage: measure one row and print it as JSON")
    args = ap.parse_args()
    if args.row:
        n, members, storage = (int(v) for v in args.row.split(","))
        print("ROW " + json.dumps(run(n, members, storage, args.repeats)), flush=True)
        return 0
    rows = []
    for case in args.cases.split(","):
        n, members = (int(v) for v in case.split("x"))
        for storage in (0, 1):
            # a fresh child per row, under its own time limit; a row that fails or runs out of time ends the tool
            cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--row", "%d,%d,%d" % (n, members, storage)]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
            if done.returncode != 0:
                print("N=%d M=%d storage=%d: the row ended with status %d; stopping" % (n, members, storage, done.returncode))
                return 1
            for line in done.stdout.splitlines():
                if not line.startswith("ROW "):
                    continue
                row = json.loads(line[4:])
                rows.append(row)
                print("N=%4d M=%2d %s | quantiles %7.3f ms (9 levels %7.3f) %5.0f GB/s moved | exceedance %7.3f ms (4 thresholds %7.3f) | "
                      "spread %7.3f ms | route %8.3f ms, %7.1f MiB extra | q/spread %5.2f | e/spread %5.2f | route/q %6.2f | off the route by %.3g"
                      % (n, members, row["storage"], row["quantiles3"]["ms"], row["quantiles9"]["ms"], row["quantiles3"]["moved_gb_per_s"],
                         row["exceedance1"]["ms"], row["exceedance4"]["ms"], row["spread"]["ms"], row["route"]["ms"],
                         row["route_peak_extra_bytes"] / 2.0 ** 20, row["ratio_quantiles_to_spread"], row["ratio_exceedance_to_spread"],
                         row["ratio_route_to_quantiles"], row["max_abs_difference_to_route"]), flush=True)
    out = {"tool": "tools/ensemble_quantile_timing.py", "commit": args.commit, "date": args.date, "repeats": args.repeats,
           "levels": {"quantiles3": LEVELS3, "quantiles9": LEVELS9, "exceedance1": THRESHOLDS1, "exceedance4": THRESHOLDS4},
           "recorded_not_gated": ["ratio_quantiles_to_spread", "ratio_exceedance_to_spread", "ratio_route_to_quantiles"],
           "quantiles_slower_than_route_somewhere": any(r["ratio_route_to_quantiles"] < 1.0 for r in rows), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
