#!/usr/bin/env python3
"""Screening observations (fluid_set_observation_qc, fluid_observation_departures): what the gate costs an analysis, and what
the departures call saves over the route a caller had before, measured in the same process against the calls they stand
beside.

Per (N, M, P, storage): uniform random fields on a mean in every member (made on the device, unpacked), P uniform random
points, the clocks as found.
- `analysis`: fluid_analyse_lattice of dens, u and v on a lattice of step 16 from cell (8, 8), c = step, with obs and
  inv_sigma, the lists cached, threshold 0 against threshold 5 in the same context: device time between two events on the
  context's stream around the one call, nothing waited for in between.  The fields are uploaded anew before every call, so
  every call analyses the same state.
- `departures`: fluid_observation_departures with every output against fluid_observe_members_host (M P floats and a wait)
  followed by the same rules in vectorised numpy (the sums with np.sum: the order is not the library's): both are
  synchronous, so the WALL time (time.perf_counter); `same_flags` says that the two agree on every flag and rank.
The median over --repeats after one untimed call, the two sides in turns, each measured twice and the slower median kept.
No threshold is set: nobody had measured either before; the numbers are written down.
Every row runs in a child process under a time limit of its own (--limit seconds).

    python tools/ensemble_qc_timing.py [--out profiles/ensemble_qc_timing.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, STEP, ORIGIN, SIDE = 1022, 16, (8, 8), 64
DEFAULT_CASES = "16x65536,64x65536"
THRESHOLD = 5.0


def median_ms(samples):
    return {"ms": float(np.median(samples)), "min_ms": float(np.min(samples)), "max_ms": float(np.max(samples))}


def host_screen(h, y, inv_sigma, threshold):
    """rules 2 - 5 of the header on the host, vectorised over the points"""
    hd = h.astype(np.float64)
    members = hd.shape[0]
    s = hd[0].copy()
    for m in range(1, members):
        s += hd[m]
    mean = s / members
    q = np.zeros_like(mean)
    for m in range(members):
        e = hd[m] - mean
        q += e * e
    var = q / (members - 1)
    sg = inv_sigma.astype(np.float64)
    dep = y.astype(np.float64) - mean
    d = dep * sg
    vs = var * sg * sg
    flag = d * d > (threshold * threshold) * (1.0 + vs)
    rank = (h < y[None, :]).sum(axis=0).astype(np.uint8)
    keep = ~flag
    sums = np.array([keep.sum(), (d * d)[keep].sum(), vs[keep].sum()])
    return {"mean": mean.astype(np.float32), "spread": np.sqrt(var).astype(np.float32), "departure": dep.astype(np.float32),
            "rank": rank, "flag": flag.astype(np.uint8), "sums": sums}


def run(members, points, storage, repeats):
    import torch
    import fluidsimulationcuda_amd as F
    n, w, c = N, N + 2, float(STEP)
    rng = np.random.default_rng(members + points)
    stream = torch.cuda.Stream()
    row = {"n": n, "members": members, "points": points, "storage": "f16" if storage else "f32", "lattice": [SIDE, SIDE], "step": STEP, "c": c,
           "threshold": THRESHOLD}
    with torch.cuda.stream(stream), F.FluidSolver(n, members=members, storage=storage, stream=stream.cuda_stream) as s:
        start = {name: torch.rand((members, w, w), dtype=torch.float32, device="cuda") * 0.1 + (50.0 if name == "dens" else 0.0)
                 for name in ("u", "v", "dens")}

        def reset():
            for name, t in start.items():
                s.unpack(name, t, wait=True)

        reset()
        cols = rng.uniform(0.5, n + 0.5, points).astype(np.float32)
        rows = rng.uniform(0.5, n + 0.5, points).astype(np.float32)
        y = (50.05 + 0.01 * rng.normal(size=points)).astype(np.float32)
        y[::97] += np.float32(5.0)                            # gross errors: about one point in a hundred
        inv_sigma = rng.uniform(5.0, 20.0, points).astype(np.float32)
        s.set_observation_points(cols, rows)
        lat = ((SIDE, SIDE), ORIGIN, STEP, c)

        def analysis(threshold):
            reset()
            s.set_observation_qc(threshold)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            s.analyse_lattice("dens", *lat, y, inv_sigma=inv_sigma, fields=("dens", "u", "v"), wait=False)
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        sides = {"threshold_0": [], "threshold_5": []}
        for _ in range(2):                                    # in turns: a drift of the clocks reaches both sides
            for name, threshold in (("threshold_0", 0.0), ("threshold_5", THRESHOLD)):
                analysis(threshold)
                sides[name].append(median_ms([analysis(threshold) for _ in range(repeats)]))
        row["analysis"] = {name: max(v, key=lambda m: m["ms"]) for name, v in sides.items()}
        row["analysis"]["unit"] = "device ms per fluid_analyse_lattice, lists cached"
        row["analysis"]["rejected"] = int(s.observation_qc_result()[2])
        row["analysis"]["status"] = s.analyse_status()
        row["analysis"]["ratio_gated_to_ungated"] = row["analysis"]["threshold_5"]["ms"] / row["analysis"]["threshold_0"]["ms"]
        s.set_observation_qc(0.0)
        reset()

        kept = {}

        def device():
            kept["device"] = s.observation_departures("dens", obs=y, inv_sigma=inv_sigma, threshold=THRESHOLD)

        def host():
            kept["host"] = host_screen(s.observe("dens"), y, inv_sigma, THRESHOLD)

        def wall(call):
            t0 = time.perf_counter()
            call()
            return (time.perf_counter() - t0) * 1e3

        sides = {"fluid_observation_departures": [], "observe_members_host_and_numpy": []}
        for _ in range(2):
            for name, call in (("fluid_observation_departures", device), ("observe_members_host_and_numpy", host)):
                call()
                sides[name].append(median_ms([wall(call) for _ in range(repeats)]))
        row["departures"] = {name: max(v, key=lambda m: m["ms"]) for name, v in sides.items()}
        row["departures"]["unit"] = "wall ms per call"
        row["departures"]["same_flags"] = bool(np.array_equal(kept["device"]["flag"], kept["host"]["flag"]) and
                                               np.array_equal(kept["device"]["rank"], kept["host"]["rank"]))
        row["departures"]["rejected"] = int(kept["device"]["flag"].sum())
        row["departures"]["inflation_estimate"] = float((kept["device"]["sums"][1] - kept["device"]["sums"][0]) / kept["device"]["sums"][2])
        row["departures"]["ratio_device_to_host"] = (row["departures"]["fluid_observation_departures"]["ms"] /
                                                     row["departures"]["observe_members_host_and_numpy"]["ms"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="MxP, comma separated")
    ap.add_argument("--storage", default="f32,f16")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--limit", type=int, default=240, help="seconds one case may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="")
    ap.add_argument("--row", default="", help="(internal) M,P,storage: measure one case and print it as JSON")
    args = ap.parse_args()
    if args.row:
        members, points, storage = (int(v) for v in args.row.split(","))
        print("ROW " + json.dumps(run(members, points, storage, args.repeats)), flush=True)
        return 0
    rows = []
    for storage in args.storage.split(","):
        for case in args.cases.split(","):
            members, points = (int(v) for v in case.split("x"))
            # a fresh child per case, under its own time limit; a case that fails or runs out of time ends the tool
            cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--row",
                   "%d,%d,%d" % (members, points, 1 if storage == "f16" else 0)]
            try:
                done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print("M=%d P=%d %s: the case ran out of its %d s; stopping" % (members, points, storage, args.limit))
                return 1
            if done.returncode != 0:
                print("M=%d P=%d %s: the case ended with status %d; stopping" % (members, points, storage, done.returncode))
                return 1
            for line in done.stdout.splitlines():
                if not line.startswith("ROW "):
                    continue
                row = json.loads(line[4:])
                rows.append(row)
                a, d = row["analysis"], row["departures"]
                print("M=%3d P=%6d %s | analysis: gate off %8.3f ms  gate on %8.3f ms  ratio %6.4f  rejected %d | departures: device %8.3f ms  "
                      "host route %8.3f ms  ratio %6.4f  same flags %s"
                      % (members, points, storage, a["threshold_0"]["ms"], a["threshold_5"]["ms"], a["ratio_gated_to_ungated"], a["rejected"],
                         d["fluid_observation_departures"]["ms"], d["observe_members_host_and_numpy"]["ms"], d["ratio_device_to_host"],
                         d["same_flags"]), flush=True)
    out = {"tool": "tools/ensemble_qc_timing.py", "commit": args.commit, "repeats": args.repeats,
           "condition": "none: the numbers are written down", "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
