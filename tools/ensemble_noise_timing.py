#!/usr/bin/env python3
"""Ensemble noise (fluid_noise_members): what a call costs beside the route a caller had before it -- torch.randn on the
device and an unpack (SET), pack, add and unpack (ADD) -- measured in the same process.

Per row (N, M, storage): three fields (dens, u, v), one amplitude per member, none of them zero, so every cell of every
member is stored.  The library and torch share one stream; what is measured is the time between two events on it, around
work that nothing waits inside of; the median over the repeats after one untimed call, the sides alternating.
- set:        noise(fields, amplitude, seed, sequence, SET): one launch per field;
- route_set:  per field torch.randn((M, W, W)) * amplitude -> unpack;
- add:        noise(fields, amplitude, seed, sequence, ADD);
- route_add:  per field pack -> + torch.randn(..) * amplitude -> unpack.
The routes draw true Gaussians with torch's generator, whose bits depend on the torch build: they are what a caller would
write, not the definition of the calls.  The condition, per row and mode (`condition_met`): the call is no slower than its
route.  No ratio was fixed in advance.
Also recorded: the bytes the call stores per second -- the field's own bytes, 4 (fp16 storage: 2) per cell and member --,
and the cells per second: the kernel makes ten rounds of two 32 x 32 -> 64 multiplies per cell and may be bound by them
rather than by memory.
Every row runs in a child process under a time limit of its own (--limit seconds).

    python tools/ensemble_noise_timing.py [--out profiles/ensemble_noise_timing.json]"""
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
SEED = 0x0123456789ABCDEF


def run(n, members, storage, repeats):
    import torch
    import fluidsimulationcuda_amd as F
    from fluidsimulationcuda_amd import capi
    w = n + 2
    stream = torch.cuda.Stream()
    row = {"n": n, "members": members, "storage": "f16" if storage else "f32", "fields": len(FIELDS)}
    with torch.cuda.stream(stream), F.FluidSolver(n, members=members, storage=storage, stream=stream.cuda_stream) as s:
        amp = np.linspace(0.5, 1.5, members).astype(np.float32)
        amp_dev = torch.from_numpy(amp).cuda().view(members, 1, 1)
        state = {"sequence": 0}
        for name in FIELDS:
            s.unpack(name, torch.zeros((members, w, w), dtype=torch.float32, device="cuda"), wait=False)

        def noise(mode):
            state["sequence"] += 1
            s.noise(FIELDS, amp, SEED, state["sequence"], mode)

        def route_set():
            for name in FIELDS:
                s.unpack(name, torch.randn((members, w, w), dtype=torch.float32, device="cuda") * amp_dev, wait=False)

        def route_add():
            for name in FIELDS:
                x = s.pack(name, wait=False)
                s.unpack(name, x + torch.randn((members, w, w), dtype=torch.float32, device="cuda") * amp_dev, wait=False)

        def timed(call):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            call()
            t1.record(stream)
            t1.synchronize()
            return t0.elapsed_time(t1)

        sides = {"set": lambda: noise(capi.NOISE_SET), "route_set": route_set, "add": lambda: noise(capi.NOISE_ADD), "route_add": route_add}
        times = {k: [] for k in sides}
        for k, call in sides.items():
            timed(call)                                  # untimed: code objects, torch's allocator, the table ring
        for _ in range(repeats):
            for k, call in sides.items():                # alternating
                times[k].append(timed(call))
        for k, v in times.items():
            row[k] = {"ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
        # the call did what the route does, as far as moments can say: a SET field has the members' amplitudes as spread
        noise(capi.NOISE_SET)
        sd = s.pack("u", wait=False).std(dim=(1, 2)).cpu().numpy()
        s.synchronize()
        row["largest_relative_error_of_member_spread"] = float(np.abs(sd / amp - 1.0).max())
    values = len(FIELDS) * w * w * members
    esz = 2 if storage else 4
    for k in ("set", "add"):
        row[k]["stored_bytes"] = values * esz
        row[k]["stored_gb_per_s"] = values * esz / row[k]["ms"] * 1e-6
        row[k]["gcells_per_s"] = values / row[k]["ms"] * 1e-6
        row["ratio_%s_to_route" % k] = row[k]["ms"] / row["route_" + k]["ms"]
    row["condition_met"] = bool(row["ratio_set_to_route"] <= 1.0 and row["ratio_add_to_route"] <= 1.0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="NxM, comma separated; each with fp32 and fp16 storage")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--limit", type=int, default=120, help="seconds one row may take")
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
            try:
                done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print("N=%d M=%d storage=%d: the row ran out of its %d s; stopping" % (n, members, storage, args.limit))
                return 1
            if done.returncode != 0:
                print("N=%d M=%d storage=%d: the row ended with status %d; stopping" % (n, members, storage, done.returncode))
                return 1
            for line in done.stdout.splitlines():
                if not line.startswith("ROW "):
                    continue
                row = json.loads(line[4:])
                rows.append(row)
                print("N=%4d M=%2d %s | set %7.3f ms, route %7.3f ms, ratio %6.3f | add %7.3f ms, route %7.3f ms, ratio %6.3f | stored %6.0f / "
                      "%6.0f GB/s, %6.1f / %6.1f Gcells/s | spread error %.2g | condition %s"
                      % (n, members, row["storage"], row["set"]["ms"], row["route_set"]["ms"], row["ratio_set_to_route"], row["add"]["ms"],
                         row["route_add"]["ms"], row["ratio_add_to_route"], row["set"]["stored_gb_per_s"], row["add"]["stored_gb_per_s"],
                         row["set"]["gcells_per_s"], row["add"]["gcells_per_s"], row["largest_relative_error_of_member_spread"],
                         "met" if row["condition_met"] else "MISSED"), flush=True)
    out = {"tool": "tools/ensemble_noise_timing.py", "commit": args.commit, "repeats": args.repeats,
           "condition": "the call's ms <= its route's, both modes, every row",
           "condition_met_everywhere": all(r["condition_met"] for r in rows), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
