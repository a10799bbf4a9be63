#!/usr/bin/env python3
"""Recombining ensembles (fluid_transform_members, fluid_select_members): what the in-place transform costs beside the
outside route it replaces, measured in the same process.

Per (N, M) and storage type, uniform random fields in every member, by the method of tools/ensemble_io_timing.py (events
on the stream the library shares with this tool -- the constructor's stream=, wait=False --, one untimed call first, median
over --repeats, clocks as found), one field:
- a dense random transform (no zero weight: the table where every term is taken), with its effective bandwidth against the
  compulsory 2 * sizeof(S) bytes per cell and member (one read, one write) and the double-precision FMA rate it reaches,
  counted as the kernel issues them: MP fmas per old member and cell, MP = M rounded up to a power of two;
- a selection with a random `source` (the table with a mask: M fmas per cell);
- fluid_pack_members + fluid_unpack_members of the same field, two launches timed together -- the floor of any outside
  route: 2 * (sizeof(S) + 4) bytes per cell and member and no arithmetic -- before and after the other measurements, so that
  a drift of the clocks during the case shows;
- where torch is importable, the full outside route: pack -> X.double() @ T -> float -> unpack.
The condition set in advance: fp32 storage, N = 1022, M = 16 -- the dense transform takes no longer than the pack + unpack
pair measured beside it (the faster of its two measurements); `condition_met` of that row says so.

Prints a table and writes JSON (--out).
    python tools/ensemble_transform_timing.py [--cases 1022x16,1022x64] [--storage f32,f16] [--out profiles/ensemble_transform_timing.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluidsimulationcuda_amd as F  # noqa: E402

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
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def timed(torch, stream, call, repeats, nbytes):
    ms, lo, hi = device_ms(torch, stream, call, repeats)
    return {"device_ms": ms, "min_ms": lo, "max_ms": hi, "compulsory_bytes": nbytes, "gb_per_s": nbytes / (ms * 1e-3) / 1e9}


def run(n, members, storage, repeats):
    import torch
    w, esz = n + 2, 2 if storage else 4
    cells = members * w * w
    padded = 1 << (members - 1).bit_length()
    rng = np.random.default_rng(n + members)
    stream = torch.cuda.Stream()
    row = {"n": n, "grid": w, "members": members, "padded_members": padded, "storage": "f16" if storage else "f32"}
    with torch.cuda.stream(stream), F.FluidSolver(n, members=members, storage=storage, stream=stream.cuda_stream) as s:
        host = rng.uniform(-1, 1, size=(members, w, w)).astype(np.float32)
        s.upload_members(u=host)
        dense = torch.empty((members, w, w), dtype=torch.float32, device="cuda")
        # an orthogonal matrix keeps the values where they are over the repeats; none of its entries is zero
        t = np.linalg.qr(rng.normal(size=(members, members)))[0].astype(np.float32)
        t[t == 0] = 1e-3
        source = rng.integers(0, members, members)

        def pair():
            s.pack("u", out=dense, wait=False)
            s.unpack("u", dense, wait=False)

        def outside():
            s.pack("u", out=dense, wait=False)
            y = (tt @ dense.view(members, w * w).double()).float()
            s.unpack("u", y, wait=False)

        row["pack_unpack"] = timed(torch, stream, pair, repeats, 2 * cells * (esz + 4))
        row["transform"] = timed(torch, stream, lambda: s.transform(t, fields=("u",)), repeats, 2 * cells * esz)
        row["transform"]["fma_f64_per_s"] = w * w * members * padded / (row["transform"]["device_ms"] * 1e-3)
        row["select"] = timed(torch, stream, lambda: s.select(source, fields=("u",)), repeats, 2 * cells * esz)
        s.upload_members(u=host)
        tt = torch.from_numpy(t.T.copy()).double().cuda()          # new[m] = sum over k of t[k][m] * old[k]
        stream.synchronize()
        row["torch_route"] = timed(torch, stream, outside, repeats, 2 * cells * (esz + 4))
        row["pack_unpack_again"] = timed(torch, stream, pair, repeats, 2 * cells * (esz + 4))
    floor_ms = min(row["pack_unpack"]["device_ms"], row["pack_unpack_again"]["device_ms"])       # the faster: the stricter yardstick
    row["transform"]["over_pack_unpack"] = row["transform"]["device_ms"] / floor_ms
    row["select"]["over_pack_unpack"] = row["select"]["device_ms"] / floor_ms
    if not storage and n == 1022 and members == 16:
        row["condition_met"] = row["transform"]["device_ms"] <= floor_ms
    return row


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
            tr, se, pu, pu2, to = (row[k] for k in ("transform", "select", "pack_unpack", "pack_unpack_again", "torch_route"))
            print("N=%5d M=%3d %s  transform %8.3f ms [%7.3f .. %7.3f] %7.1f GB/s %6.2f Tfma/s %5.2f x pair | select %8.3f ms %7.1f GB/s | "
                  "pack + unpack %8.3f ms %7.1f GB/s (again %8.3f ms) | torch route %8.3f ms%s" % (
                      n, members, storage, tr["device_ms"], tr["min_ms"], tr["max_ms"], tr["gb_per_s"], tr["fma_f64_per_s"] / 1e12,
                      tr["over_pack_unpack"], se["device_ms"], se["gb_per_s"], pu["device_ms"], pu["gb_per_s"], pu2["device_ms"], to["device_ms"],
                      "" if "condition_met" not in row else "  condition %s" % ("met" if row["condition_met"] else "MISSED")), flush=True)
    out = {"tool": "tools/ensemble_transform_timing.py", "commit": args.commit, "repeats": args.repeats, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
