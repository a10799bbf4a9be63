#!/usr/bin/env python3
"""Relaxation to prior spread (fluid_member_spread + fluid_relax_spread): what the two calls cost beside the route a caller
had before them -- pack, torch algebra on the device, unpack -- measured in the same process.

Per row (N, M, storage): three fields (dens, u, v), uniform random values on a mean of 50 in every member, made on the device
and unpacked.  The prior is 1.5 times the spread the ensemble has, so every cell of every member is stored.  Before every
measured call the three fields are put back from device copies (not timed), so every call relaxes the same ensemble.  The
library and torch share one stream; what is measured is the time between two events on it, around work that nothing waits
inside of; the median over the repeats after one untimed call, the two sides alternating.
- calls:  spread(fields, wait=False), then relax_spread(prior, alpha, fields, wait=False);
- route:  per field pack -> std over the members;  then per field pack -> mean, std, the factor, mean + f * (x - mean) ->
          unpack.  float32 torch algebra: what a caller would write, NOT the double arithmetic of the calls (no defined bits).
The condition, per row (`condition_met`): the calls are no slower than the route.  No ratio was fixed in advance.
Also recorded: the two calls timed on their own, and their bytes per second against the traffic of the definition -- per
cell and field the spread reads 4 M bytes and writes 4, the relaxation reads 4 M + 4 and writes 4 M (`model`, the header's
count for float fields); with fp16 storage the fields themselves are half of that (`moved`).
Every row runs in a child process under a time limit of its own (--limit seconds).

    python tools/ensemble_relax_timing.py [--out profiles/ensemble_relax_timing.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_CASES = "254x16,1022x16,1022x64"
FIELDS = ("dens", "u", "v")
ALPHA = 0.9


def run(n, members, storage, repeats):
    import torch
    import fluidsimulationcuda_amd as F
    w = n + 2
    stream = torch.cuda.Stream()
    row = {"n": n, "members": members, "storage": "f16" if storage else "f32", "fields": len(FIELDS), "alpha": ALPHA}
    with torch.cuda.stream(stream), F.FluidSolver(n, members=members, storage=storage, stream=stream.cuda_stream) as s:
        saved = {name: torch.rand((members, w, w), dtype=torch.float32, device="cuda") + 50.0 for name in FIELDS}

        def restore():
            for name in FIELDS:
                s.unpack(name, saved[name], wait=False)

        restore()
        prior = s.spread(FIELDS, wait=False) * 1.5
        out = torch.empty_like(prior)

        def spread():
            s.spread(FIELDS, out=out, wait=False)

        def relax():
            s.relax_spread(prior, ALPHA, fields=FIELDS, wait=False)

        def calls():
            spread()
            relax()

        def route():
            sd_b = [s.pack(name, wait=False).std(dim=0, unbiased=True) for name in FIELDS]
            for name, sb in zip(FIELDS, sd_b):
                x = s.pack(name, wait=False)
                mean = x.mean(dim=0)
                sa = x.std(dim=0, unbiased=True)
                f = torch.where(sa > 0, 1.0 + ALPHA * (sb * 1.5 - sa) / sa, torch.ones_like(sa))
                s.unpack(name, mean + f * (x - mean), wait=False)

        def timed(call):
            restore()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            call()
            t1.record(stream)
            t1.synchronize()
            return t0.elapsed_time(t1)

        sides = {"calls": calls, "route": route, "spread": spread, "relax": relax}
        times = {k: [] for k in sides}
        for k, call in sides.items():
            timed(call)                                  # untimed: code objects, torch's allocator
        for _ in range(repeats):
            for k, call in sides.items():                # alternating
                times[k].append(timed(call))
        for k, v in times.items():
            row[k] = {"ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
        # the relaxation did what the route does (float algebra against double: no bits, a tolerance of float rounding)
        restore()
        calls()
        mine = {name: s.pack(name, wait=False) for name in FIELDS}
        restore()
        route()
        worst = max(float(((mine[name] - s.pack(name, wait=False)).abs() / mine[name].abs()).max()) for name in FIELDS)
        s.synchronize()
        row["largest_relative_difference_to_route"] = worst
    cells = len(FIELDS) * w * w
    esz = 2 if storage else 4
    for k, model, moved in (("spread", 4 * members + 4, esz * members + 4), ("relax", 8 * members + 4, 2 * esz * members + 4)):
        row[k]["model_bytes"], row[k]["moved_bytes"] = cells * model, cells * moved
        row[k]["model_gb_per_s"] = cells * model / row[k]["ms"] * 1e-6
        row[k]["moved_gb_per_s"] = cells * moved / row[k]["ms"] * 1e-6
    row["ratio_calls_to_route"] = row["calls"]["ms"] / row["route"]["ms"]
    row["condition_met"] = bool(row["ratio_calls_to_route"] <= 1.0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="NxM, comma separated; each with fp32 and fp16 storage")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--limit", type=int, default=180, help="seconds one row may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="")
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
                print("N=%4d M=%2d %s | calls %8.3f ms (spread %7.3f, relax %7.3f) | route %8.3f ms | calls/route %6.3f | spread %6.0f GB/s, "
                      "relax %6.0f GB/s by the model (%.0f, %.0f moved) | diff %.2g | condition %s"
                      % (n, members, row["storage"], row["calls"]["ms"], row["spread"]["ms"], row["relax"]["ms"], row["route"]["ms"],
                         row["ratio_calls_to_route"], row["spread"]["model_gb_per_s"], row["relax"]["model_gb_per_s"],
                         row["spread"]["moved_gb_per_s"], row["relax"]["moved_gb_per_s"], row["largest_relative_difference_to_route"],
                         "met" if row["condition_met"] else "MISSED"), flush=True)
    out = {"tool": "tools/ensemble_relax_timing.py", "commit": args.commit, "repeats": args.repeats,
           "condition": "the two calls' ms <= the route's, every row",
           "condition_met_everywhere": all(r["condition_met"] for r in rows), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
