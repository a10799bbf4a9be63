#!/usr/bin/env python3
"""Lattice updates (fluid_transform_members_lattice): what the blended update costs beside the local call it generalises,
measured in the same process.

Per (N, M) and storage type, uniform random values in every member of one field, by the method of
tools/ensemble_local_timing.py (events on the stream the library shares with this tool -- the constructor's stream=; the
calls go to the C entry point directly --, one untimed call first, median over --repeats, clocks as found).  Every node's
increments are D = Q - I with an orthogonal Q, scaled per node, none of them zero (the tables where every term is taken).
- (a) fluid_transform_members_local with a null taper and a null box: the yardstick, measured before and after.
- (b) the lattice call with a 1 x 1 lattice: one corner, the walk of (a) in chunks of 16 new members.  Expectation: about (a).
- (c) the lattice call with step 64 and as many nodes as cover the array (at most 64 x 64 = FLUID_LATTICE_MAX_NODES,
  centred), dense matrices: four node sums per cell against one, and 4 M blend operations against M * M.  Expectation: at
  most 4 x (a).  The events enclose the whole call: the host widens and stages nodes * M * MP doubles before it enqueues
  the copy and the launch, and the stream waits for that; `host_call_ms` is the host clock around the same call, and
  `table_bytes` what travels.
- (d) for context: the launch floor of the chained-local route for (c)'s node count, nodes x 0.014 ms, one field.
Nothing is asserted.  Prints a table and writes JSON (--out).
    python tools/ensemble_lattice_timing.py [--cases 1022x8,4094x64] [--storage f32,f16] [--out profiles/ensemble_lattice_timing.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluidsimulationcuda_amd as F  # noqa: E402
from fluidsimulationcuda_amd import capi  # noqa: E402

DEFAULT_CASES = "1022x8,1022x32,1022x64,4094x8,4094x32,4094x64"
LAUNCH_MS = 0.014


def device_ms(torch, stream, call, repeats):
    call()
    out, host = [], []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t = time.perf_counter()
        call()
        host.append((time.perf_counter() - t) * 1e3)
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"device_ms": float(np.median(out)), "min_ms": float(np.min(out)), "max_ms": float(np.max(out)),
            "host_call_ms": float(np.median(host))}


def run(n, members, storage, repeats):
    import torch
    w = n + 2
    step = 64
    side = min(64, (w + step - 1) // step + 1)
    origin = (w - 1 - (side - 1) * step) // 2
    rng = np.random.default_rng(n + members)
    stream = torch.cuda.Stream()
    row = {"n": n, "grid": w, "members": members, "storage": "f16" if storage else "f32", "step": step, "nodes": side * side,
           "origin": origin, "table_bytes": side * side * members * (capi_padded(members) * 8 + 8) + side * side * 8}
    with torch.cuda.stream(stream), F.FluidSolver(n, members=members, storage=storage, stream=stream.cuda_stream) as s:
        base = rng.uniform(-1, 1, size=(w, w)).astype(np.float32)
        for m in range(members):                 # (member by member, each a shifted copy: no dense ensemble on the host)
            s.upload(member=m, u=np.roll(base, 17 * m + 1, axis=0))
        q = np.linalg.qr(rng.normal(size=(members, members)))[0].astype(np.float32)
        d = (q - np.eye(members, dtype=np.float32)).astype(np.float32)
        d[d == 0] = 1e-3
        d *= np.float32(0.01)                    # small increments: the values stay where they are over the repeats
        many = (d[None, None] * rng.uniform(0.5, 1.0, (side, side, 1, 1)).astype(np.float32)).astype(np.float32)
        many = np.ascontiguousarray(many)
        ids = (C.c_int * 1)(capi.U)
        L = capi.lib()

        def local():
            capi.check(L.fluid_transform_members_local(s._h, ids, 1, d.ctypes.data_as(capi._MF), None, None))

        def one_node():
            capi.check(L.fluid_transform_members_lattice(s._h, ids, 1, d.ctypes.data_as(capi._MF), 1, 1, w // 2, w // 2, 8))

        def lattice():
            capi.check(L.fluid_transform_members_lattice(s._h, ids, 1, many.ctypes.data_as(capi._MF), side, side, origin, origin, step))

        stream.synchronize()
        row["local_full"] = device_ms(torch, stream, local, repeats)
        row["lattice_1x1"] = device_ms(torch, stream, one_node, repeats)
        row["lattice_cover"] = device_ms(torch, stream, lattice, repeats)
        row["local_full_again"] = device_ms(torch, stream, local, repeats)
    floor_ms = min(row["local_full"]["device_ms"], row["local_full_again"]["device_ms"])          # the faster: the stricter yardstick
    row["lattice_1x1"]["over_local"] = row["lattice_1x1"]["device_ms"] / floor_ms
    row["lattice_cover"]["over_local"] = row["lattice_cover"]["device_ms"] / floor_ms
    row["chained_local_launch_floor_ms"] = side * side * LAUNCH_MS
    return row


def capi_padded(members):
    mp = 1
    while mp < members:
        mp <<= 1
    return mp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="NxM, comma separated")
    ap.add_argument("--storage", default="f32,f16")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    rows = []
    for storage in args.storage.split(","):
        for case in args.cases.split(","):
            n, members = (int(v) for v in case.split("x"))
            row = run(n, members, 1 if storage == "f16" else 0, args.repeats)
            rows.append(row)
            a, a2, b, c = (row[k] for k in ("local_full", "local_full_again", "lattice_1x1", "lattice_cover"))
            print("N=%5d M=%3d %s  (a) local, null taper and box %8.3f ms (again %8.3f ms) | (b) 1 x 1 lattice %8.3f ms %5.2f x (a) | "
                  "(c) %d nodes, step %d %8.3f ms [%7.3f .. %7.3f] %5.2f x (a), host %8.3f ms, tables %.1f MiB | (d) chained launches %7.3f ms" % (
                      n, members, storage, a["device_ms"], a2["device_ms"], b["device_ms"], b["over_local"], row["nodes"], row["step"],
                      c["device_ms"], c["min_ms"], c["max_ms"], c["over_local"], c["host_call_ms"], row["table_bytes"] / 2.0 ** 20,
                      row["chained_local_launch_floor_ms"]), flush=True)
    out = {"tool": "tools/ensemble_lattice_timing.py", "commit": args.commit, "repeats": args.repeats, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
