#!/usr/bin/env python3
"""The one-call analysis (fluid_analyse_lattice): what the call costs beside the route a caller had before it, measured in
the same process.

Per (M, lattice): N = 1022, uniform random fields on a mean in every member (made on the device, unpacked), P uniform random
points, a lattice of step 16 from cell (8, 8), c = step, rho = 1, observed field dens, updated fields dens, u, v.  Before
every measured call the three fields are put back from device copies (not timed), so every call analyses the same
background.  What is measured is WALL time (time.perf_counter), the median over the repeats after one untimed call:
- fused: analyse_lattice(wait=False) + synchronize;
- route: observation_gram_lattice, then per node that sees a point numpy.linalg.eigh and INTEGRATION.md's host algebra, then
  transform_lattice + synchronize -- with the three parts timed on their own (`gram_ms`, `host_ms`, `lattice_ms`).
The condition, per row (`condition_met`): the fused call is no slower than the route.  No ratio was fixed in advance.
Also recorded: `solve_ms`, fluid_etkf_increments alone on the row's matrices (upload, one launch, download, wait); the
status counts; and `largest_difference_units`: the largest difference between the device's increments and the host
algebra's (float64, the definition's D = W - I + w 1^T), the float term 2^-23 |D| taken off, in units of
M 2^-53 kappa (sqrt(rho) + max |w|) -- the tolerance of tests/test_gpu_etkf.py allows 64 of them.
Every row runs in a child process under a time limit of its own (--limit seconds).

    python tools/ensemble_etkf_timing.py [--out profiles/ensemble_etkf_timing.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, STEP, ORIGIN, POINTS = 1022, 16, (8, 8), 65536
DEFAULT_CASES = ",".join("%dx%d" % (m, side) for m in (16, 64) for side in (16, 64))
U = 2.0 ** -53
FIELDS = ("dens", "u", "v")


def host_increment(gram, rhs, members):
    """what a caller computed per node before the call existed"""
    lam, v = np.linalg.eigh((members - 1) * np.eye(members) + gram)
    w = v @ ((v.T @ rhs) / lam)
    big = v @ np.diag(np.sqrt((members - 1) / lam)) @ v.T
    a = np.eye(members) - np.ones((members, members)) / members
    return np.ones((members, members)) / members + a @ (big + w[:, None]) - np.eye(members)


def run(members, side, repeats, route_repeats):
    import torch
    import fluidsimulationcuda_amd as F
    n, w, c = N, N + 2, float(STEP)
    rng = np.random.default_rng(members + side)
    stream = torch.cuda.Stream()
    shape = (side, side)
    row = {"n": n, "members": members, "points": POINTS, "lattice": [side, side], "nodes": side * side, "step": STEP, "c": c, "rho": 1.0}
    with torch.cuda.stream(stream), F.FluidSolver(n, members=members, stream=stream.cuda_stream) as s:
        saved = {name: torch.rand((members, w, w), dtype=torch.float32, device="cuda") + 50.0 for name in FIELDS}
        cols = rng.uniform(0.5, n + 0.5, POINTS).astype(np.float32)
        rows = rng.uniform(0.5, n + 0.5, POINTS).astype(np.float32)
        y = (50.5 + 0.1 * rng.normal(size=POINTS)).astype(np.float32)
        inv_sigma = rng.uniform(5.0, 20.0, POINTS).astype(np.float32)
        s.set_observation_points(cols, rows)

        def restore():
            for name in FIELDS:
                s.unpack(name, saved[name], wait=True)
            s.synchronize()

        def fused():
            s.analyse_lattice("dens", shape, ORIGIN, STEP, c, y, inv_sigma=inv_sigma, fields=FIELDS, wait=False)
            s.synchronize()

        parts = {"gram_ms": [], "host_ms": [], "lattice_ms": []}
        kept = {}

        def route():
            t0 = time.perf_counter()
            gram, rhs, _, counts = s.observation_gram_lattice("dens", shape, ORIGIN, STEP, c, obs=y, inv_sigma=inv_sigma, centre=True)
            t1 = time.perf_counter()
            d = np.zeros(shape + (members, members), np.float32)
            for a, b in zip(*np.nonzero(counts)):
                d[a, b] = host_increment(gram[a, b], rhs[a, b], members)
            t2 = time.perf_counter()
            s.transform_lattice(d, ORIGIN, STEP, fields=FIELDS)
            s.synchronize()
            t3 = time.perf_counter()
            for key, v in zip(("gram_ms", "host_ms", "lattice_ms"), (t1 - t0, t2 - t1, t3 - t2)):
                parts[key].append(v * 1e3)
            kept["operands"] = (gram, rhs, counts)

        def wall(call, count):
            restore()
            call()
            out = []
            for _ in range(count):
                restore()
                t0 = time.perf_counter()
                call()
                out.append((time.perf_counter() - t0) * 1e3)
            return {"wall_ms": float(np.median(out)), "min_ms": float(np.min(out)), "max_ms": float(np.max(out))}

        row["fused"] = wall(fused, repeats)
        row["status"] = s.analyse_status()
        row["route"] = wall(route, route_repeats)
        row["route"]["repeats"] = route_repeats
        for key, v in parts.items():
            row["route"][key] = float(np.median(v[1:]))
        gram, rhs, counts = kept["operands"]
        got = {}

        def solve():
            got["d"], got["status"] = s.etkf_increments(gram, rhs, counts=counts)

        row["solve_ms"] = wall(solve, repeats)["wall_ms"]
        worst = 0.0
        for a, b in zip(*np.nonzero(counts)):
            lam, v = np.linalg.eigh((members - 1) * np.eye(members) + gram[a, b])
            wv = v @ ((v.T @ rhs[a, b]) / lam)
            want = v @ np.diag(np.sqrt((members - 1) / lam)) @ v.T - np.eye(members) + wv[:, None]
            kappa = 1.0 + np.linalg.norm(gram[a, b], 2) / (members - 1)
            unit = members * U * kappa * (1.0 + np.abs(wv).max())
            worst = max(worst, float(((np.abs(got["d"][a, b] - want) - 2.0 ** -23 * np.abs(want)) / unit).max()))
        row["largest_difference_units"] = worst
        row["solve_status"] = {"solved": int((got["status"] == 0).sum()), "empty": int((got["status"] == 1).sum()),
                               "failed": int((got["status"] == 2).sum())}
    row["ratio_fused_to_route"] = row["fused"]["wall_ms"] / row["route"]["wall_ms"]
    row["condition_met"] = bool(row["ratio_fused_to_route"] <= 1.0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="MxSIDE (a SIDE x SIDE lattice), comma separated")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--route-repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds one case may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="")
    ap.add_argument("--row", default="", help="(internal) M,SIDE: measure one case and print it as JSON")
    args = ap.parse_args()
    if args.row:
        members, side = (int(v) for v in args.row.split(","))
        print("ROW " + json.dumps(run(members, side, args.repeats, args.route_repeats)), flush=True)
        return 0
    rows = []
    for case in args.cases.split(","):
        members, side = (int(v) for v in case.split("x"))
        # a fresh child per case, under its own time limit; a case that fails or runs out of time ends the tool
        cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--route-repeats", str(args.route_repeats),
               "--row", "%d,%d" % (members, side)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
        if done.returncode != 0:
            print("M=%d %dx%d: the case ended with status %d; stopping" % (members, side, side, done.returncode))
            return 1
        for line in done.stdout.splitlines():
            if not line.startswith("ROW "):
                continue
            row = json.loads(line[4:])
            rows.append(row)
            print("M=%3d %2dx%-2d | fused %9.3f ms | route %10.3f ms (gram %8.3f, host %10.3f, lattice %8.3f) | solve alone %8.3f ms | "
                  "fused/route %7.4f  diff %6.3f units  %s  condition %s"
                  % (members, side, side, row["fused"]["wall_ms"], row["route"]["wall_ms"], row["route"]["gram_ms"], row["route"]["host_ms"],
                     row["route"]["lattice_ms"], row["solve_ms"], row["ratio_fused_to_route"], row["largest_difference_units"],
                     row["status"], "met" if row["condition_met"] else "MISSED"), flush=True)
    out = {"tool": "tools/ensemble_etkf_timing.py", "commit": args.commit, "repeats": args.repeats,
           "condition": "the fused call's wall_ms <= the route's, every row",
           "condition_met_everywhere": all(r["condition_met"] for r in rows), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
