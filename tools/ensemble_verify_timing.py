#!/usr/bin/env python3
"""Verifying ensembles (fluid_verify_members): what one call costs beside one read of the members by unchanged code, and
beside the route a caller had before it -- pack, torch.sort, the formulas in torch on the device -- measured in the same
process.

Per row (N, M, storage): one field (dens), uniform random values on a mean of 50 in every member, made on the device and
unpacked; the truth is one more such array.  The box is the interior.  The library and torch share one stream; what is
measured is the time between two events on it, around work that nothing waits inside of; the median over the repeats after
one untimed call, the sides alternating.
- (a) verify:      verify(truth, ("dens",), out=row, wait=False), and the same with crps_map= (`verify_map`);
- (b) spread:      spread(("dens",), out=sd, wait=False): fluid_member_spread, code this call does not touch, which reads the same
                   members once and writes one float per cell -- the yardstick for "one read of the members";
- (c) route:       pack -> torch.sort over the members -> mean, unbiased variance, the sorted-form CRPS and the ranks in float32
                   per cell, the four sums in float64 and torch.bincount over the interior: what a caller would write, NOT the
                   double arithmetic of the call (no defined bits).  `route_peak_extra_bytes`: torch's peak allocation above
                   what was allocated before the route began.
Recorded, not gated: `ratio_verify_to_spread` = (a) / (b), `ratio_route_to_verify` = (c) / (a); and (a)'s bytes per second against
the traffic of the definition, per cell esz * M + 4 bytes read (`moved`: esz is 2 with fp16 storage).
Every row runs in a child process under a time limit of its own (--limit seconds).

    python tools/ensemble_verify_timing.py [--out profiles/ensemble_verify_timing.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_CASES = "254x8,254x32,254x64,1022x8,1022x32,1022x64"
FIELD = "dens"


def run(n, members, storage, repeats):
    import torch
    import fluidsimulationcuda_amd as F
    from fluidsimulationcuda_amd import capi
    w = n + 2
    stream = torch.cuda.Stream()
    row = {"n": n, "members": members, "storage": "f16" if storage else "f32", "fields": 1}
    with torch.cuda.stream(stream), F.FluidSolver(n, members=members, storage=storage, stream=stream.cuda_stream) as s:
        s.unpack(FIELD, torch.rand((members, w, w), dtype=torch.float32, device="cuda") + 50.0, wait=False)
        truth = torch.rand((1, w, w), dtype=torch.float32, device="cuda") + 50.0
        scores = torch.zeros((1, capi.VERIFY_ROW), dtype=torch.float64, device="cuda")
        crps_map = torch.zeros((1, w, w), dtype=torch.float32, device="cuda")
        sd = torch.zeros((1, w, w), dtype=torch.float32, device="cuda")
        coef = (2.0 * torch.arange(1, members + 1, dtype=torch.float32, device="cuda") - members - 1.0).view(members, 1, 1)
        kept = {}

        def verify():
            s.verify(truth, (FIELD,), out=scores, wait=False)

        def verify_map():
            s.verify(truth, (FIELD,), crps_map=crps_map, out=scores, wait=False)

        def spread():
            s.spread((FIELD,), out=sd, wait=False)

        def route():
            x = s.pack(FIELD, wait=False)
            y = truth[0]
            xs, _ = torch.sort(x, dim=0)
            mean = x.mean(dim=0)
            var = x.var(dim=0, unbiased=True)
            e = mean - y
            crps = (xs - y).abs().mean(dim=0) - (coef * xs).sum(dim=0) / float(members * members)
            rank = (x < y).sum(dim=0)
            inner = (slice(1, n + 1), slice(1, n + 1))
            kept["sums"] = torch.stack([t[inner].double().sum() for t in (e, e * e, var, crps)])
            kept["hist"] = torch.bincount(rank[inner].flatten(), minlength=members + 1)

        def timed(call):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            call()
            t1.record(stream)
            t1.synchronize()
            return t0.elapsed_time(t1)

        sides = {"verify": verify, "verify_map": verify_map, "spread": spread, "route": route}
        times = {k: [] for k in sides}
        for k, call in sides.items():
            timed(call)                                  # untimed: code objects, torch's allocator, the call's scratch
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
        # the call scores what the route scores (float algebra against double: no bits, a tolerance of float rounding)
        verify()
        got = s.verify_scores(scores)[0]
        cells = float(n * n)
        want = (kept["sums"] / cells).cpu().numpy()
        row["scores"] = {k: got[k] for k in ("bias", "rmse", "spread", "crps")}
        row["route_scores"] = {"bias": float(want[0]), "rmse": float(np.sqrt(want[1])), "spread": float(np.sqrt(want[2])), "crps": float(want[3])}
        row["rank_histograms_equal"] = bool(np.array_equal(got["rank_hist"], kept["hist"].cpu().numpy()))
    esz = 2 if storage else 4
    moved = n * n * (esz * members + 4)
    for k in ("verify", "verify_map"):
        row[k]["moved_bytes"] = moved + (4 * n * n if k == "verify_map" else 0)
        row[k]["moved_gb_per_s"] = row[k]["moved_bytes"] / row[k]["ms"] * 1e-6
    row["ratio_verify_to_spread"] = row["verify"]["ms"] / row["spread"]["ms"]
    row["ratio_route_to_verify"] = row["route"]["ms"] / row["verify"]["ms"]
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
                print("N=%4d M=%2d %s | verify %7.3f ms (with map %7.3f) %5.0f GB/s moved | spread %7.3f ms | route %8.3f ms, %6.1f MiB extra | "
                      "verify/spread %6.2f | route/verify %6.2f | crps %.6g (route %.6g) | histograms %s"
                      % (n, members, row["storage"], row["verify"]["ms"], row["verify_map"]["ms"], row["verify"]["moved_gb_per_s"],
                         row["spread"]["ms"], row["route"]["ms"], row["route_peak_extra_bytes"] / 2.0 ** 20, row["ratio_verify_to_spread"],
                         row["ratio_route_to_verify"], row["scores"]["crps"], row["route_scores"]["crps"],
                         "equal" if row["rank_histograms_equal"] else "DIFFER"), flush=True)
    out = {"tool": "tools/ensemble_verify_timing.py", "commit": args.commit, "date": args.date, "repeats": args.repeats,
           "recorded_not_gated": ["ratio_verify_to_spread", "ratio_route_to_verify"],
           "verify_slower_than_route_somewhere": any(r["ratio_route_to_verify"] < 1.0 for r in rows), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
