#!/usr/bin/env python3
"""Typed observation networks (fluid_set_observation_network, FLUID_FIELD_OF_POINT): what the joint analysis of a mixed network
costs beside the route a caller had before it, what typing itself costs, and whether the untyped calls kept their speed.

Per (M, lattice): N = 1022, uniform random fields on a mean in every member (made on the device, unpacked), P = 65536 uniform
random points whose fields cycle u, v, dens, a lattice of step 16 from cell (8, 8), c = step, rho = 1, updated fields dens, u,
v.  Everything is WALL time (time.perf_counter), the median over the repeats after one untimed call; every row runs in a child
process under a time limit of its own (--limit seconds).

- joint: `fused`, analyse_lattice(field=None) on the typed network + synchronize, against `route`, the same joint analysis
  without typed networks: per variable set_observation_points on the sub-network + observation_gram_lattice, the matrices
  added in numpy, then etkf_increments and transform_lattice + synchronize.  Before every measured call the three fields are
  put back from device copies (not timed).  The condition, per row (`condition_met`): fused <= route.  No ratio was fixed in
  advance.  `largest_field_difference`: the route's and the fused call's joint Gram matrices differ in the order of their
  additions, so the two analyses are compared by what they leave in the updated fields, not by bits.
- typing: every point naming ONE field (dens), the typed call (field=None) against the untyped call on the same points, for
  observation_gram and for observation_gram_lattice with its lists cached.  `kernel_ms`: the device time of each call's
  kernels, each from a run of its own under rocprofv3 --kernel-trace --stats (a further child per row and variant).
- untyped: observation_gram, the cached observation_gram_lattice and analyse_lattice on an untyped network, on this build and --
  `--parent TREE`, a tree with the parent commit's package built -- on the parent's build, which is run twice with this build
  in between: this build's faster run is held against the parent's slower run plus the difference of the parent's two
  (`inside_parent_spread`); the untyped kernels' device times are taken on both builds as well.

    python tools/ensemble_network_timing.py [--parent TREE] [--out profiles/ensemble_network_timing.json]"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, STEP, ORIGIN, POINTS = 1022, 16, (8, 8), 65536
DEFAULT_CASES = ",".join("%dx%d" % (m, side) for m in (16, 64) for side in (16, 64))
FIELDS = ("dens", "u", "v")
CYCLE = ("u", "v", "dens")
KERNELS = ("k_observation_gram", "k_fold_observation_gram", "k_observation_operands", "k_lattice_gram")


def wall(call, count, before=None):
    if before:
        before()
    call()
    out = []
    for _ in range(count):
        if before:
            before()
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"wall_ms": float(np.median(out)), "min_ms": float(np.min(out)), "max_ms": float(np.max(out))}


def setup(members, side):
    import torch
    import fluidsimulationcuda_amd as F
    rng = np.random.default_rng(members + side)
    stream = torch.cuda.Stream()
    ctx = torch.cuda.stream(stream)
    ctx.__enter__()
    s = F.FluidSolver(N, members=members, stream=stream.cuda_stream)
    w = N + 2
    saved = {name: torch.rand((members, w, w), dtype=torch.float32, device="cuda") + 50.0 for name in FIELDS}
    cols = rng.uniform(0.5, N + 0.5, POINTS).astype(np.float32)
    rows = rng.uniform(0.5, N + 0.5, POINTS).astype(np.float32)
    y = (50.5 + 0.1 * rng.normal(size=POINTS)).astype(np.float32)
    inv_sigma = rng.uniform(5.0, 20.0, POINTS).astype(np.float32)

    def restore():
        for name in FIELDS:
            s.unpack(name, saved[name], wait=True)
        s.synchronize()

    restore()
    return s, cols, rows, y, inv_sigma, restore, (ctx, stream, saved)


def run_joint(members, side, repeats, route_repeats):
    s, cols, rows, y, inv_sigma, restore, keep = setup(members, side)
    shape, c = (side, side), float(STEP)
    names = np.array([CYCLE[k % 3] for k in range(POINTS)])
    sub = {f: np.nonzero(names == f)[0] for f in CYCLE}
    row = {"what": "joint", "n": N, "members": members, "points": POINTS, "lattice": [side, side], "nodes": side * side, "step": STEP, "c": c}
    with s:
        s.set_observation_network(cols, rows, list(names))

        def fused():
            s.analyse_lattice(None, shape, ORIGIN, STEP, c, y, inv_sigma=inv_sigma, fields=FIELDS, wait=False)
            s.synchronize()

        parts = {"grams_ms": [], "sum_ms": [], "solve_ms": [], "lattice_ms": []}

        def route():
            t0 = time.perf_counter()
            got = []
            for f in CYCLE:
                s.set_observation_points(cols[sub[f]], rows[sub[f]])
                got.append(s.observation_gram_lattice(f, shape, ORIGIN, STEP, c, obs=y[sub[f]], inv_sigma=inv_sigma[sub[f]], centre=True))
            t1 = time.perf_counter()
            gram = got[0][0] + got[1][0] + got[2][0]
            rhs = got[0][1] + got[1][1] + got[2][1]
            counts = got[0][3] + got[1][3] + got[2][3]
            t2 = time.perf_counter()
            d, _ = s.etkf_increments(gram, rhs, counts=counts)
            t3 = time.perf_counter()
            s.transform_lattice(d, ORIGIN, STEP, fields=FIELDS)
            s.synchronize()
            t4 = time.perf_counter()
            for key, v in zip(("grams_ms", "sum_ms", "solve_ms", "lattice_ms"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                parts[key].append(v * 1e3)

        row["fused"] = wall(fused, repeats, restore)
        row["status"] = s.analyse_status()
        after_fused = {f: s.download_members(f) for f in FIELDS}
        row["route"] = wall(route, route_repeats, restore)
        row["route"]["repeats"] = route_repeats
        for key, v in parts.items():
            row["route"][key] = float(np.median(v[1:]))
        worst = 0.0
        for f in FIELDS:
            worst = max(worst, float(np.abs(s.download_members(f).astype(np.float64) - after_fused[f]).max()))
        row["largest_field_difference"] = worst
    row["ratio_fused_to_route"] = row["fused"]["wall_ms"] / row["route"]["wall_ms"]
    row["condition_met"] = bool(row["ratio_fused_to_route"] <= 1.0)
    return row


def calls_of(s, typed, side, y, inv_sigma):
    """the three measured calls on the network in place: every point observes dens, by its type or by the call's field"""
    field, shape, c = (None if typed else "dens"), (side, side), float(STEP)
    return {
        "observation_gram": lambda: s.observation_gram(field, obs=y, inv_sigma=inv_sigma, centre=True),
        "observation_gram_lattice_cached": lambda: s.observation_gram_lattice(field, shape, ORIGIN, STEP, c, obs=y, inv_sigma=inv_sigma, centre=True),
        "analyse_lattice": lambda: (s.analyse_lattice(field, shape, ORIGIN, STEP, c, y, inv_sigma=inv_sigma, fields=FIELDS, wait=False),
                                    s.synchronize()),
    }


def run_single(members, side, repeats, typed, kernels_only):
    s, cols, rows, y, inv_sigma, restore, keep = setup(members, side)
    row = {"what": "typed" if typed else "untyped", "members": members, "lattice": [side, side]}
    with s:
        if typed:
            s.set_observation_network(cols, rows, ["dens"] * POINTS)
        else:
            s.set_observation_points(cols, rows)
        calls = calls_of(s, typed, side, y, inv_sigma)
        if kernels_only:                       # under the profiler: the two Gram calls and nothing else
            for name in ("observation_gram", "observation_gram_lattice_cached"):
                for _ in range(repeats + 1):
                    calls[name]()
            return row
        for name, call in calls.items():
            row[name] = wall(call, repeats, restore if name == "analyse_lattice" else None)
    return row


def child(args, what, case, tree="", profile=False):
    """one row in a fresh child under the time limit; `tree`: the package is imported from there"""
    cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--route-repeats", str(args.route_repeats), "--row", case,
           "--what", what] + (["--tree", tree] if tree else []) + (["--kernels-only"] if profile else [])
    if not profile:
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
        if done.returncode != 0:
            raise RuntimeError("%s %s ended with status %d" % (what, case, done.returncode))
        return [json.loads(line[4:]) for line in done.stdout.splitlines() if line.startswith("ROW ")][0]
    with tempfile.TemporaryDirectory() as d:
        done = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + cmd, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True, timeout=args.limit)
        if done.returncode != 0:
            raise RuntimeError("rocprofv3: %s %s ended with status %d" % (what, case, done.returncode))
        spans = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for rec in csv.DictReader(open(path)):
                for name in KERNELS:
                    if re.search(r"\b%s\b" % name, rec.get("Kernel_Name", "")):
                        spans.setdefault(name, []).append(int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"]))
        return {name: {"calls": len(v), "median_ms": float(np.median(v)) * 1e-6} for name, v in spans.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="MxSIDE (a SIDE x SIDE lattice), comma separated")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--route-repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds one child may take")
    ap.add_argument("--parent", default="", help="a tree with the parent commit's package built: the untyped calls are measured there too, twice")
    ap.add_argument("--no-kernel-times", action="store_true", help="no children under rocprofv3")
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="")
    ap.add_argument("--row", default="", help="(internal) M,SIDE: measure one case and print it as JSON")
    ap.add_argument("--what", default="joint", help="(internal) joint, typed or untyped")
    ap.add_argument("--tree", default="", help="(internal) import the package from this tree")
    ap.add_argument("--kernels-only", action="store_true", help="(internal) the Gram calls alone, for the profiler")
    args = ap.parse_args()
    if args.row:
        sys.path.insert(0, os.path.abspath(args.tree) if args.tree else ROOT)
        members, side = (int(v) for v in args.row.split(","))
        if args.what == "joint":
            row = run_joint(members, side, args.repeats, args.route_repeats)
        else:
            row = run_single(members, side, args.repeats, args.what == "typed", args.kernels_only)
        print("ROW " + json.dumps(row), flush=True)
        return 0
    rows = []
    names = ("observation_gram", "observation_gram_lattice_cached", "analyse_lattice")
    for case in args.cases.split(","):
        members, side = (int(v) for v in case.split("x"))
        arg = "%d,%d" % (members, side)
        row = {"members": members, "lattice": [side, side]}
        row["joint"] = child(args, "joint", arg)
        j = row["joint"]
        print("M=%3d %2dx%-2d | joint: fused %9.3f ms | route %10.3f ms (grams %9.3f, sum %7.3f, solve %8.3f, lattice %8.3f) | fused/route %7.4f  %s  "
              "condition %s" % (members, side, side, j["fused"]["wall_ms"], j["route"]["wall_ms"], j["route"]["grams_ms"], j["route"]["sum_ms"],
                                j["route"]["solve_ms"], j["route"]["lattice_ms"], j["ratio_fused_to_route"], j["status"],
                                "met" if j["condition_met"] else "MISSED"), flush=True)
        row["typed"] = child(args, "typed", arg)
        row["untyped"] = child(args, "untyped", arg)
        if not args.no_kernel_times:
            row["typed"]["kernel_ms"] = child(args, "typed", arg, profile=True)
            row["untyped"]["kernel_ms"] = child(args, "untyped", arg, profile=True)
        for name in names:
            row["typed_to_untyped_" + name] = row["typed"][name]["wall_ms"] / row["untyped"][name]["wall_ms"]
        print("             | typing: " + " | ".join("%s %8.3f / %8.3f ms" % (name, row["typed"][name]["wall_ms"], row["untyped"][name]["wall_ms"])
                                                     for name in names), flush=True)
        if not args.no_kernel_times:
            print("             | kernels, typed / untyped ms: " + ", ".join(
                "%s %.4f / %.4f" % (k, row["typed"]["kernel_ms"].get(k, {}).get("median_ms", float("nan")),
                                    row["untyped"]["kernel_ms"].get(k, {}).get("median_ms", float("nan"))) for k in KERNELS), flush=True)
        if args.parent:                        # parent, this build once more, parent: the builds alternate
            row["parent"] = [child(args, "untyped", arg, tree=args.parent)]
            row["untyped_again"] = child(args, "untyped", arg)
            row["parent"].append(child(args, "untyped", arg, tree=args.parent))
            if not args.no_kernel_times:
                row["parent"][0]["kernel_ms"] = child(args, "untyped", arg, tree=args.parent, profile=True)
            row["inside_parent_spread"] = {}
            for name in names:
                a, b = (r[name]["wall_ms"] for r in row["parent"])
                now = min(row["untyped"][name]["wall_ms"], row["untyped_again"][name]["wall_ms"])
                # no slower than the parent's slower run by more than the parent's own two runs differ
                row["inside_parent_spread"][name] = bool(now <= max(a, b) + abs(a - b))
                print("             | untyped %s: this build %8.3f and %8.3f ms, the parent's %8.3f and %8.3f ms: %s" % (
                    name, row["untyped"][name]["wall_ms"], row["untyped_again"][name]["wall_ms"], a, b,
                    "inside" if row["inside_parent_spread"][name] else "OUTSIDE"), flush=True)
            if not args.no_kernel_times:
                print("             | untyped kernels, this build / the parent's ms: " + ", ".join(
                    "%s %.4f / %.4f" % (k, row["untyped"]["kernel_ms"].get(k, {}).get("median_ms", float("nan")),
                                        row["parent"][0]["kernel_ms"].get(k, {}).get("median_ms", float("nan"))) for k in KERNELS), flush=True)
        rows.append(row)
    out = {"tool": "tools/ensemble_network_timing.py", "commit": args.commit, "repeats": args.repeats,
           "condition": "the typed fused call's wall_ms <= the per-variable route's, every row",
           "condition_met_everywhere": all(r["joint"]["condition_met"] for r in rows), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
