#!/usr/bin/env python3
"""The ensemble Gram matrix (fluid_member_gram): what the library call costs beside the outside route it replaces, measured
in the same process.

Per (N, M), storage type and `centre`, uniform random fields in every member (offset by 50 for `centre`: a spread on a
mean), by the method of tools/ensemble_transform_timing.py (events on the stream the library shares with this tool -- the
constructor's stream= --, one untimed call first, median over --repeats, clocks as found), one field:
- fluid_member_gram: the two kernels, the copy of the M x M result and the one wait the call ends in, between two events;
  with its effective bandwidth against the compulsory bytes -- ONE read of the field, sizeof(S) bytes per interior cell
  and member -- and the double-precision FMA rate it reaches, counted as the kernel issues them: MP * MP per interior cell,
  MP = M rounded up to 8, 16, 32 or 64 (the lower triangle's lanes included);
- the route a caller had before: fluid_pack_members into a dense float tensor, .double(), the mean over the members
  subtracted first for `centre`, A^T A by torch.matmul over the interior cells -- calls this library's Gram kernels take no
  part in.
The condition set in advance, for every row: the call's device time is no more than the route's (ratio <= 1.0, no margin);
`condition_met` of each row says so.  Every step on the device runs under a time limit of its own (--limit seconds): one
child process per case.

Prints a table and writes JSON (--out).
    python tools/ensemble_gram_timing.py [--cases 1022x16,1022x64] [--storage f32,f16] [--out profiles/ensemble_gram_timing.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_CASES = "1022x16,1022x64,254x64,4094x8"


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


def run(n, members, storage, centre, repeats):
    import torch
    import fluidsimulationcuda_amd as F
    w, esz = n + 2, 2 if storage else 4
    padded = max(8, 1 << (members - 1).bit_length())
    rng = np.random.default_rng(n + members)
    stream = torch.cuda.Stream()
    row = {"n": n, "grid": w, "members": members, "padded_members": padded, "storage": "f16" if storage else "f32", "centre": bool(centre)}
    with torch.cuda.stream(stream), F.FluidSolver(n, members=members, storage=storage, stream=stream.cuda_stream) as s:
        host = rng.uniform(-1, 1, size=(members, w, w)).astype(np.float32)
        if centre:
            host += 50
        s.upload_members(u=host)
        dense = torch.empty((members, w, w), dtype=torch.float32, device="cuda")
        kept = {}

        def call():
            kept["gram"] = s.member_gram("u", centre=centre)

        def route():
            s.pack("u", out=dense, wait=False)
            a = dense[:, 1:-1, 1:-1].double().reshape(members, n * n)
            if centre:
                a = a - a.mean(dim=0, keepdim=True)
            kept["route"] = a @ a.T

        nbytes = members * n * n * esz
        g = row["gram"] = device_ms(torch, stream, call, repeats)
        g["compulsory_bytes"] = nbytes
        g["gb_per_s"] = nbytes / (g["device_ms"] * 1e-3) / 1e9
        g["fma_f64_per_s"] = n * n * padded * padded / (g["device_ms"] * 1e-3)
        row["torch_route"] = device_ms(torch, stream, route, repeats)
        row["gram_again"] = device_ms(torch, stream, call, repeats)
        stream.synchronize()
        ref = kept["route"].cpu().numpy()
        row["largest_difference_from_route"] = float(np.abs(kept["gram"] - ref).max() / np.abs(ref).max())
    ms = max(g["device_ms"], row["gram_again"]["device_ms"])           # the slower of its two measurements: the stricter reading
    row["ratio"] = ms / row["torch_route"]["device_ms"]
    row["condition_met"] = bool(row["ratio"] <= 1.0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="NxM, comma separated")
    ap.add_argument("--storage", default="f32,f16")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--limit", type=int, default=120, help="seconds one case (its two rows) may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="")
    ap.add_argument("--rows", default="", help="(internal) N,M,storage: measure the two rows of a case and print them as JSON")
    args = ap.parse_args()
    if args.rows:
        n, members, storage = (int(v) for v in args.rows.split(","))
        for centre in (0, 1):
            print("ROW " + json.dumps(run(n, members, storage, centre, args.repeats)), flush=True)
        return 0
    rows = []
    for storage in args.storage.split(","):
        for case in args.cases.split(","):
            n, members = (int(v) for v in case.split("x"))
            # a fresh child per case (its two rows: centre 0 and 1), under its own time limit; a case that fails or runs out
            # of time ends the tool
            cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats),
                   "--rows", "%d,%d,%d" % (n, members, 1 if storage == "f16" else 0)]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
            if done.returncode != 0:
                print("N=%d M=%d %s: the case ended with status %d; stopping" % (n, members, storage, done.returncode))
                return 1
            for line in done.stdout.splitlines():
                if not line.startswith("ROW "):
                    continue
                row = json.loads(line[4:])
                rows.append(row)
                g, to = row["gram"], row["torch_route"]
                print("N=%5d M=%3d %s centre=%d  gram %8.3f ms [%7.3f .. %7.3f] (again %8.3f) %7.1f GB/s %6.2f Tfma/s | torch route %8.3f ms | "
                      "ratio %5.2f  condition %s" % (n, members, storage, row["centre"], g["device_ms"], g["min_ms"], g["max_ms"],
                                                     row["gram_again"]["device_ms"], g["gb_per_s"], g["fma_f64_per_s"] / 1e12, to["device_ms"],
                                                     row["ratio"], "met" if row["condition_met"] else "MISSED"), flush=True)
    out = {"tool": "tools/ensemble_gram_timing.py", "commit": args.commit, "repeats": args.repeats,
           "condition": "gram device_ms (the slower of two measurements) <= torch_route device_ms, every row",
           "condition_met_everywhere": all(r["condition_met"] for r in rows), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
