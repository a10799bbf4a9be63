#!/usr/bin/env python3
"""Observing ensembles (fluid_observe_members, fluid_observation_gram): what the library calls cost beside the outside route
they replace, measured in the same process.

Per (N, M, P), uniform random fields in every member (made on the device, unpacked), P uniform random points, by the method
of tools/ensemble_gram_timing.py (events on the stream the library shares with this tool -- the constructor's stream= --,
one untimed call first, median over --repeats, clocks as found), one field:
- observe_device: the one launch of fluid_observe_members into a dense (M, P) device array, between two events; with the
  bytes it asks for, 4 taps of sizeof(S) bytes per member and point plus the 4 bytes it stores;
- observation_gram: fluid_observation_gram with `obs`, `inv_sigma` and `centre` -- the two copies of P floats, the two
  kernels, the copy of the result and the one wait the call ends in;
- the route a caller had before, for each: fluid_pack_members of ALL members into a dense float tensor, then in torch a gather
  of the four taps, the two lerps (float), and for the Gram matrix .double(), the mean over the members subtracted, the
  scaling, and [A; d] [A; d]^T by torch.matmul -- calls this library's observing kernels take no part in.
The condition set in advance, for every row: each call's device time is no more than its route's (ratio <= 1.0, no
margin); `condition_met` of each row says so.  Every step on the device runs under a time limit of its own (--limit
seconds): one child process per case.

Prints a table and writes JSON (--out).
    python tools/ensemble_observe_timing.py [--cases 4094x8x1000,4094x64x100000] [--out profiles/ensemble_observe_timing.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_CASES = ",".join("4094x%dx%d" % (m, p) for m in (8, 64) for p in (1000, 100000, 1000000))


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
    return {"device_ms": float(np.median(out)), "min_ms": float(np.min(out)), "max_ms": float(np.max(out))}


def run(n, members, points, storage, repeats):
    import torch
    import fluidsimulationcuda_amd as F
    w, esz = n + 2, 2 if storage else 4
    rng = np.random.default_rng(n + members + points)
    stream = torch.cuda.Stream()
    row = {"n": n, "grid": w, "members": members, "points": points, "storage": "f16" if storage else "f32"}
    with torch.cuda.stream(stream), F.FluidSolver(n, members=members, storage=storage, stream=stream.cuda_stream) as s:
        dense = torch.rand((members, w, w), dtype=torch.float32, device="cuda") + 50.0          # a spread on a mean
        s.unpack("u", dense, wait=False)
        cols = rng.uniform(0.5, n + 0.5, points).astype(np.float32)
        rows = rng.uniform(0.5, n + 0.5, points).astype(np.float32)
        y = (50.5 + 0.1 * rng.normal(size=points)).astype(np.float32)
        inv_sigma = rng.uniform(5.0, 20.0, points).astype(np.float32)
        s.set_observation_points(cols, rows)
        out = torch.empty((members, points), dtype=torch.float32, device="cuda")
        # the route's own resident network: tap indices and weights, made once like the library's table
        c, r = torch.from_numpy(cols).cuda(), torch.from_numpy(rows).cuda()
        j0, i0 = c.long(), r.long()
        s1, t1 = c - j0.float(), r - i0.float()
        s0, t0 = 1.0 - s1, 1.0 - t1
        tap = i0 * w + j0
        yd, sd = torch.from_numpy(y).cuda().double(), torch.from_numpy(inv_sigma).cuda().double()
        kept = {}

        def observe():
            s.observe_device("u", out=out, wait=False)

        def gram():
            kept["gram"] = s.observation_gram("u", obs=y, inv_sigma=inv_sigma, centre=True)

        def route_observe():
            s.pack("u", out=dense, wait=False)
            x = dense.view(members, w * w)
            a = t0 * x[:, tap] + t1 * x[:, tap + w]
            e = t0 * x[:, tap + 1] + t1 * x[:, tap + w + 1]
            kept["h"] = s0 * a + s1 * e

        def route_gram():
            route_observe()
            h = kept["h"].double()
            mean = h.mean(dim=0, keepdim=True)
            full = torch.cat([(h - mean) * sd, (yd - mean) * sd], dim=0)
            kept["route"] = full @ full.T

        o = row["observe_device"] = device_ms(torch, stream, observe, repeats)
        o["gathered_bytes"] = members * points * (4 * esz + 4)
        o["gb_per_s"] = o["gathered_bytes"] / (o["device_ms"] * 1e-3) / 1e9
        row["observation_gram"] = device_ms(torch, stream, gram, repeats)
        row["route_observe"] = device_ms(torch, stream, route_observe, repeats)
        row["route_gram"] = device_ms(torch, stream, route_gram, repeats)
        row["observe_device_again"] = device_ms(torch, stream, observe, repeats)
        row["observation_gram_again"] = device_ms(torch, stream, gram, repeats)
        stream.synchronize()
        ref = kept["route"].cpu().numpy()
        g, rhs, dd = kept["gram"]
        got = np.block([[g, rhs[:, None]], [rhs[None, :], np.array([[dd]])]])
        row["largest_difference_from_route"] = float(np.abs(got - ref).max() / np.abs(ref).max())
        row["observations_differ_from_route"] = int((out != kept["h"]).sum().item()) if not storage else None
    # the slower of a call's two measurements: the stricter reading
    row["observe_ratio"] = max(o["device_ms"], row["observe_device_again"]["device_ms"]) / row["route_observe"]["device_ms"]
    row["gram_ratio"] = max(row["observation_gram"]["device_ms"], row["observation_gram_again"]["device_ms"]) / row["route_gram"]["device_ms"]
    row["condition_met"] = bool(row["observe_ratio"] <= 1.0 and row["gram_ratio"] <= 1.0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="NxMxP, comma separated")
    ap.add_argument("--storage", default="f32")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--limit", type=int, default=120, help="seconds one case may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="")
    ap.add_argument("--row", default="", help="(internal) N,M,P,storage: measure one case and print it as JSON")
    args = ap.parse_args()
    if args.row:
        n, members, points, storage = (int(v) for v in args.row.split(","))
        print("ROW " + json.dumps(run(n, members, points, storage, args.repeats)), flush=True)
        return 0
    rows = []
    for storage in args.storage.split(","):
        for case in args.cases.split(","):
            n, members, points = (int(v) for v in case.split("x"))
            # a fresh child per case, under its own time limit; a case that fails or runs out of time ends the tool
            cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats),
                   "--row", "%d,%d,%d,%d" % (n, members, points, 1 if storage == "f16" else 0)]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
            if done.returncode != 0:
                print("N=%d M=%d P=%d %s: the case ended with status %d; stopping" % (n, members, points, storage, done.returncode))
                return 1
            for line in done.stdout.splitlines():
                if not line.startswith("ROW "):
                    continue
                row = json.loads(line[4:])
                rows.append(row)
                print("N=%5d M=%3d P=%8d %s  observe %8.3f ms (again %8.3f) %7.1f GB/s | route %8.3f ms | ratio %6.3f || gram %8.3f ms (again %8.3f) | "
                      "route %8.3f ms | ratio %6.3f  condition %s"
                      % (n, members, points, storage, row["observe_device"]["device_ms"], row["observe_device_again"]["device_ms"],
                         row["observe_device"]["gb_per_s"], row["route_observe"]["device_ms"], row["observe_ratio"],
                         row["observation_gram"]["device_ms"], row["observation_gram_again"]["device_ms"], row["route_gram"]["device_ms"],
                         row["gram_ratio"], "met" if row["condition_met"] else "MISSED"), flush=True)
    out = {"tool": "tools/ensemble_observe_timing.py", "commit": args.commit, "repeats": args.repeats,
           "condition": "observe_device and observation_gram device_ms (the slower of two measurements each) <= their route's, every row",
           "condition_met_everywhere": all(r["condition_met"] for r in rows), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
