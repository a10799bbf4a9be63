#!/usr/bin/env python3
"""Asynchronous observations (fluid_run_window and the recorded lattice Gram): what recording costs a run, and what reading
a record saves a Gram call, measured in the same process against the calls they stand beside.

Per (N, M, P, storage): uniform random fields on a mean in every member (made on the device, unpacked), P uniform random
points, the clocks as found.
- `run`: fluid_run_members over --steps steps (iters sweeps, no snapshots) against fluid_run_window on the same plan with one
  slot per step, slot s the points [s P / steps, (s + 1) P / steps) observed after step s + 1: device time between two
  events on the context's stream around the one call, nothing waited for in between, per step; the median over --repeats
  after one untimed call, each side measured twice in turns and the slower median kept.
- `gram`: fluid_observation_gram_lattice (sampling dens) against fluid_observation_gram_lattice_recorded (reading the record
  fluid_observe_members wrote from the same state), a lattice of step 16 from cell (8, 8), c = step, with obs, inv_sigma and
  centre, the lists cached: both calls are synchronous, so the WALL time of a call (time.perf_counter around it), the median
  over --repeats after one untimed call; `same_bits` says that the two results agree bit for bit.
No threshold is set: nobody had measured either before; the numbers are written down.  This change touches neither the
fluid_run_members path nor the sampled Gram, so both comparisons are like for like.
Every row runs in a child process under a time limit of its own (--limit seconds).

    python tools/ensemble_window_timing.py [--out profiles/ensemble_window_timing.json]"""
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


def median_ms(samples):
    return {"ms": float(np.median(samples)), "min_ms": float(np.min(samples)), "max_ms": float(np.max(samples))}


def run(members, points, storage, steps, iters, repeats):
    import torch
    import fluidsimulationcuda_amd as F
    from fluidsimulationcuda_amd.solver import DT
    n, w, c = N, N + 2, float(STEP)
    rng = np.random.default_rng(members + points)
    stream = torch.cuda.Stream()
    row = {"n": n, "members": members, "points": points, "storage": "f16" if storage else "f32", "steps": steps, "iters": iters,
           "lattice": [SIDE, SIDE], "step": STEP, "c": c}
    with torch.cuda.stream(stream), F.FluidSolver(n, members=members, storage=storage, stream=stream.cuda_stream) as s:
        for name in ("u", "v", "dens"):
            s.unpack(name, torch.rand((members, w, w), dtype=torch.float32, device="cuda") * 0.1 + (50.0 if name == "dens" else 0.0), wait=True)
        cols = rng.uniform(0.5, n + 0.5, points).astype(np.float32)
        rows = rng.uniform(0.5, n + 0.5, points).astype(np.float32)
        y = (50.05 + 0.01 * rng.normal(size=points)).astype(np.float32)
        inv_sigma = rng.uniform(5.0, 20.0, points).astype(np.float32)
        s.set_observation_points(cols, rows)
        record = torch.zeros((members, points), dtype=torch.float32, device="cuda")
        first = [k * points // steps for k in range(steps + 1)]
        due = list(range(1, steps + 1))

        def timed(call):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / steps

        def plain():
            s.run(steps, dt=np.full(members, DT, np.float32), iters=iters, wait=False)

        def windowed():
            s.run_window(steps, first, due, record=record, field="dens", iters=iters, wait=False)

        sides = {"fluid_run_members": [], "fluid_run_window": []}
        for _ in range(2):                                    # in turns: a drift of the clocks reaches both sides
            for name, call in (("fluid_run_members", plain), ("fluid_run_window", windowed)):
                timed(call)
                sides[name].append(median_ms([timed(call) for _ in range(repeats)]))
        row["run"] = {name: max(v, key=lambda m: m["ms"]) for name, v in sides.items()}
        row["run"]["unit"] = "device ms per step"
        row["run"]["ratio_window_to_members"] = row["run"]["fluid_run_window"]["ms"] / row["run"]["fluid_run_members"]["ms"]

        kept = {}
        s.observe_device("dens", out=record, wait=True)
        lat = ((SIDE, SIDE), ORIGIN, STEP, c)

        def sampled():
            kept["sampled"] = s.observation_gram_lattice("dens", *lat, obs=y, inv_sigma=inv_sigma, centre=True)

        def recorded():
            kept["recorded"] = s.observation_gram_lattice_recorded(record, *lat, obs=y, inv_sigma=inv_sigma, centre=True)

        def wall(call):
            t0 = time.perf_counter()
            call()
            return (time.perf_counter() - t0) * 1e3

        sides = {"fluid_observation_gram_lattice": [], "fluid_observation_gram_lattice_recorded": []}
        for _ in range(2):
            for name, call in (("fluid_observation_gram_lattice", sampled), ("fluid_observation_gram_lattice_recorded", recorded)):
                call()
                sides[name].append(median_ms([wall(call) for _ in range(repeats)]))
        row["gram"] = {name: max(v, key=lambda m: m["ms"]) for name, v in sides.items()}
        row["gram"]["unit"] = "wall ms per call, lists cached"
        row["gram"]["pairs"] = int(kept["sampled"][3].sum())
        row["gram"]["same_bits"] = bool(all(np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)
                                            for a, b in zip(kept["sampled"], kept["recorded"])))
        row["gram"]["ratio_recorded_to_sampled"] = (row["gram"]["fluid_observation_gram_lattice_recorded"]["ms"] /
                                                    row["gram"]["fluid_observation_gram_lattice"]["ms"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="MxP, comma separated")
    ap.add_argument("--storage", default="f32,f16")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--limit", type=int, default=240, help="seconds one case may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="")
    ap.add_argument("--row", default="", help="(internal) M,P,storage: measure one case and print it as JSON")
    args = ap.parse_args()
    if args.row:
        members, points, storage = (int(v) for v in args.row.split(","))
        print("ROW " + json.dumps(run(members, points, storage, args.steps, args.iters, args.repeats)), flush=True)
        return 0
    rows = []
    for storage in args.storage.split(","):
        for case in args.cases.split(","):
            members, points = (int(v) for v in case.split("x"))
            # a fresh child per case, under its own time limit; a case that fails or runs out of time ends the tool
            cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--iters", str(args.iters), "--repeats", str(args.repeats),
                   "--row", "%d,%d,%d" % (members, points, 1 if storage == "f16" else 0)]
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
                r, g = row["run"], row["gram"]
                print("M=%3d P=%6d %s | per step: run_members %8.3f ms  run_window %8.3f ms  ratio %6.4f | lattice Gram: sampled %8.3f ms  "
                      "recorded %8.3f ms  ratio %6.4f  same bits %s"
                      % (members, points, storage, r["fluid_run_members"]["ms"], r["fluid_run_window"]["ms"], r["ratio_window_to_members"],
                         g["fluid_observation_gram_lattice"]["ms"], g["fluid_observation_gram_lattice_recorded"]["ms"],
                         g["ratio_recorded_to_sampled"], g["same_bits"]), flush=True)
    out = {"tool": "tools/ensemble_window_timing.py", "commit": args.commit, "repeats": args.repeats,
           "condition": "none: the numbers are written down", "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
