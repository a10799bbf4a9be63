#!/usr/bin/env python3
"""Lattice observations (fluid_observation_gram_lattice): what the one call costs beside the route a caller had before it,
measured in the same process.

Per (N, M, P, lattice, storage): uniform random fields on a mean in every member (made on the device, unpacked), P uniform
random points, a lattice of step 16 from cell (8, 8), c = step, with `obs`, `inv_sigma` and `centre`.  The calls are
synchronous, so what is measured is the WALL time of a call (time.perf_counter around it), the median over --repeats after
one untimed call, clocks as found:
- cold: the call right after fluid_set_observation_points (which is not timed): the point lists are built and uploaded;
- cached: a repeat call with the same network, lattice and c;
  each measured twice, the slower of the two medians kept -- the stricter reading;
- route: what a caller had before: per node that sees a point, one fluid_observation_gram call with inv_sigma * sqrt(w), w
  the node's taper at the points.  The weights of every node are worked out before the clock starts; per node the clock sees
  a buffer of P floats zeroed and the node's values scattered into it, and the call.  --route-repeats (3) passes over all
  nodes, their median: the route takes seconds at 4096 nodes, and it is not the side the condition is strict about.
The condition, per row (`condition_met`): the cached call is no slower than the route.  No ratio was fixed in advance.
Also recorded: `kernel_ms`, the device time of the call's two kernels alone, from a run of their own under rocprofv3
--kernel-trace --stats (a second child per row: the network, then calls and nothing else; the average over the calls;
--no-kernel-times leaves it out); `result_copy_ms`, a pinned copy of as many bytes as the call's results on its own (at 4096
nodes and 64 members 136 MB); and the largest difference from the route relative to (gamma(P_b + 3) + 2^-22) sqrt(G_kk G_mm): the summation bound of both sides plus the one thing the route does
differently, rounding sqrt(w) / sigma to float (2^-24 per operand and twice per product, doubled for the two sides).
Every row runs in a child process under a time limit of its own (--limit seconds).

    python tools/ensemble_lattice_gram_timing.py [--out profiles/ensemble_lattice_gram_timing.json]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, STEP, ORIGIN = 1022, 16, (8, 8)
DEFAULT_CASES = ",".join("%dx%dx%d" % (m, p, side) for m in (16, 64) for p in (4096, 65536) for side in (16, 64))
U = 2.0 ** -53


def taper(r):
    """fluid_taper_gaspari_cohn's value at r, float64, Horner's rule"""
    with np.errstate(all="ignore"):
        g = -0.25 * r + 0.5
        g = g * r + 0.625
        g = g * r - 5.0 / 3.0
        g = g * r
        near = g * r + 1.0
        g = (1.0 / 12.0) * r - 0.5
        g = g * r + 0.625
        g = g * r + 5.0 / 3.0
        g = g * r - 5.0
        g = g * r + 4.0
        far = g - (2.0 / 3.0) / r
    return np.clip(np.where(r <= 1.0, near, np.where(r < 2.0, far, 0.0)), 0.0, 1.0).astype(np.float32)


def node_lists(cols, rows, side, c):
    """per node (row-major): the indices of the points with w != 0 and sqrt(w) there"""
    x, y = cols.astype(np.float64), rows.astype(np.float64)
    out = []
    for a in range(side):
        dy = y - (ORIGIN[0] + a * STEP)
        band = np.nonzero(np.abs(dy) < 2.0 * c)[0]
        for b in range(side):
            dx = x[band] - (ORIGIN[1] + b * STEP)
            w = taper(np.sqrt(dx * dx + dy[band] * dy[band]) / np.float64(c))
            keep = np.nonzero(w)[0]
            out.append((band[keep], np.sqrt(w[keep].astype(np.float64))))
    return out


def wall_ms(call, repeats, before=None):
    if before:
        before()
    call()
    out = []
    for _ in range(repeats):
        if before:
            before()
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"wall_ms": float(np.median(out)), "min_ms": float(np.min(out)), "max_ms": float(np.max(out))}


def kernel_times(row_arg, limit):
    """the average device time of each of the call's kernels, ms, from rocprofv3's kernel statistics of a run of its own"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--row", row_arg, "--kernels-only"]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
        if done.returncode != 0:
            return {"error": "rocprofv3 ended with status %d" % done.returncode}
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for rec in csv.DictReader(open(path)):
                for name in ("k_observation_operands", "k_lattice_gram"):
                    if name in rec.get("Name", ""):
                        out[name] = {"calls": int(rec["Calls"]), "average_ms": float(rec["AverageNs"]) * 1e-6}
        if len(out) != 2:                     # no statistics file: the same average from the trace itself
            spans = {}
            for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                for rec in csv.DictReader(open(path)):
                    for name in ("k_observation_operands", "k_lattice_gram"):
                        if name in rec.get("Kernel_Name", ""):
                            spans.setdefault(name, []).append(int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"]))
            out = {name: {"calls": len(v), "average_ms": float(np.mean(v)) * 1e-6} for name, v in spans.items()}
        if len(out) != 2:
            return {"error": "no statistics of the two kernels were found"}
        out["sum_ms"] = out["k_observation_operands"]["average_ms"] + out["k_lattice_gram"]["average_ms"]
        return out


def run(members, points, side, storage, repeats, route_repeats, kernels_only=False):
    import torch
    import fluidsimulationcuda_amd as F
    n, w, c = N, N + 2, float(STEP)
    rng = np.random.default_rng(members + points + side)
    stream = torch.cuda.Stream()
    row = {"n": n, "members": members, "points": points, "lattice": [side, side], "step": STEP, "c": c, "storage": "f16" if storage else "f32"}
    with torch.cuda.stream(stream), F.FluidSolver(n, members=members, storage=storage, stream=stream.cuda_stream) as s:
        dense = torch.rand((members, w, w), dtype=torch.float32, device="cuda") + 50.0          # a spread on a mean
        s.unpack("u", dense, wait=True)
        cols = rng.uniform(0.5, n + 0.5, points).astype(np.float32)
        rows = rng.uniform(0.5, n + 0.5, points).astype(np.float32)
        y = (50.5 + 0.1 * rng.normal(size=points)).astype(np.float32)
        inv_sigma = rng.uniform(5.0, 20.0, points).astype(np.float32)
        kept = {}

        def network():
            s.set_observation_points(cols, rows)

        def lattice():
            kept["got"] = s.observation_gram_lattice("u", (side, side), ORIGIN, STEP, c, obs=y, inv_sigma=inv_sigma, centre=True)

        network()
        lattice()
        if kernels_only:
            for _ in range(9):
                lattice()
            return {}
        counts = kept["got"][3]
        row["pairs"] = int(counts.sum())
        row["nodes_with_points"] = int((counts > 0).sum())
        row["largest_count"] = int(counts.max())
        lists = node_lists(cols, rows, side, c)
        row["lists_agree"] = bool([len(i) for i, _ in lists] == counts.ravel().tolist())      # the tool's lists are the library's
        scaled = [(idx, (inv_sigma[idx].astype(np.float64) * sw).astype(np.float32)) for idx, sw in lists]
        buf = np.zeros(points, np.float32)

        def route():
            res = []
            for idx, vals in scaled:
                if len(idx) == 0:
                    res.append(None)
                    continue
                buf[:] = 0.0
                buf[idx] = vals
                res.append(s.observation_gram("u", obs=y, inv_sigma=buf, centre=True))
            kept["route"] = res

        cold = [wall_ms(lattice, repeats, before=network) for _ in range(2)]
        cached = [wall_ms(lattice, repeats) for _ in range(2)]
        row["cold"] = max(cold, key=lambda v: v["wall_ms"])
        row["cached"] = max(cached, key=lambda v: v["wall_ms"])
        row["route"] = wall_ms(route, route_repeats)
        row["route"]["repeats"] = route_repeats
        mp = 8 if members <= 8 else 1 << (members - 1).bit_length()
        nbytes = side * side * (mp * mp + mp + 1) * 8
        src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        copies = []
        for _ in range(repeats + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            dst.copy_(src, non_blocking=True)
            b.record(stream)
            b.synchronize()
            copies.append(a.elapsed_time(b))
        row["result_bytes"] = nbytes
        row["result_copy_ms"] = float(np.median(copies[1:]))
        # against the route: every node that sees a point
        gram, rhs, dd, _ = kept["got"]
        worst = 0.0
        for node, ref in enumerate(kept["route"]):
            if ref is None:
                continue
            a_, b_ = divmod(node, side)
            got = np.block([[gram[a_, b_], rhs[a_, b_][:, None]], [rhs[a_, b_][None, :], np.array([[dd[a_, b_]]])]])
            want = np.block([[ref[0], ref[1][:, None]], [ref[1][None, :], np.array([[ref[2]]])]])
            diag = np.sqrt(np.abs(np.diag(want)))
            pb = counts[a_, b_] + 3
            bound = (pb * U / (1 - pb * U) + 2.0 ** -22) * np.outer(diag, diag)
            worst = max(worst, float((np.abs(got - want) / np.maximum(bound, 1e-300)).max()))
        row["largest_difference_from_route_over_bound"] = worst
    row["ratio_cached_to_route"] = row["cached"]["wall_ms"] / row["route"]["wall_ms"]
    row["ratio_cold_to_route"] = row["cold"]["wall_ms"] / row["route"]["wall_ms"]
    row["condition_met"] = bool(row["ratio_cached_to_route"] <= 1.0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="MxPxSIDE (a SIDE x SIDE lattice), comma separated")
    ap.add_argument("--storage", default="f32,f16")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--route-repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds one case may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="")
    ap.add_argument("--no-kernel-times", action="store_true", help="no second child per row under rocprofv3")
    ap.add_argument("--row", default="", help="(internal) M,P,SIDE,storage: measure one case and print it as JSON")
    ap.add_argument("--kernels-only", action="store_true", help="(internal) with --row: the network and ten calls, nothing else")
    args = ap.parse_args()
    if args.row:
        members, points, side, storage = (int(v) for v in args.row.split(","))
        print("ROW " + json.dumps(run(members, points, side, storage, args.repeats, args.route_repeats, args.kernels_only)), flush=True)
        return 0
    rows = []
    for storage in args.storage.split(","):
        for case in args.cases.split(","):
            members, points, side = (int(v) for v in case.split("x"))
            # a fresh child per case, under its own time limit; a case that fails or runs out of time ends the tool
            row_arg = "%d,%d,%d,%d" % (members, points, side, 1 if storage == "f16" else 0)
            cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--route-repeats", str(args.route_repeats),
                   "--row", row_arg]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
            if done.returncode != 0:
                print("M=%d P=%d %dx%d %s: the case ended with status %d; stopping" % (members, points, side, side, storage, done.returncode))
                return 1
            for line in done.stdout.splitlines():
                if not line.startswith("ROW "):
                    continue
                row = json.loads(line[4:])
                if not args.no_kernel_times:
                    row["kernel_ms"] = kernel_times(row_arg, args.limit)
                rows.append(row)
                print("M=%3d P=%6d %2dx%-2d %s  pairs %8d | cold %9.3f ms  cached %9.3f ms (kernels %9.4f, copy %7.3f) | route %10.3f ms | "
                      "cached/route %7.4f  diff/bound %6.3f  condition %s"
                      % (members, points, side, side, storage, row["pairs"], row["cold"]["wall_ms"], row["cached"]["wall_ms"],
                         row.get("kernel_ms", {}).get("sum_ms", float("nan")), row["result_copy_ms"], row["route"]["wall_ms"], row["ratio_cached_to_route"],
                         row["largest_difference_from_route_over_bound"], "met" if row["condition_met"] else "MISSED"), flush=True)
    out = {"tool": "tools/ensemble_lattice_gram_timing.py", "commit": args.commit, "repeats": args.repeats,
           "condition": "the cached call's wall_ms (the slower of two measurements) <= the route's, every row",
           "condition_met_everywhere": all(r["condition_met"] for r in rows), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
