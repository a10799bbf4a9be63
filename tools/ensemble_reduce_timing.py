#!/usr/bin/env python3
"""Ensemble diagnostics (fluid_residual_members, fluid_absmax_velocity_members, fluid_member_moments,
fluid_ensemble_stats): wall time of each call beside the only other way to the same numbers -- one fluid_download_member
per member and field the quantity needs, then numpy on the host.

Per (N, M): uniform random fields in every member; per call the median over --repeats of the wall time between
fluid_synchronize pairs (the calls that return values are synchronous themselves; the statistics are timed "computed only",
both pointers null, and once more with both fields copied to the host).  The host way is timed in two parts: the
downloads, and the numpy arithmetic on the downloaded arrays.  For the moments and the statistics also compulsory bytes /
time: each member's field read once (the statistics read every member twice; how much of the second pass comes from
cache is what a counter run of this tool under a profiler shows, not this table).

Prints a table and writes JSON (--out).
    python tools/ensemble_reduce_timing.py [--cases 256x16,1024x64] [--repeats 9] [--out profiles/ensemble_reduce_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluidsimulationcuda_amd as F  # noqa: E402

DEFAULT_CASES = "256x16,256x64,1024x16,1024x64,4094x4,64x4096"


def median_ms(s, call, repeats):
    call()                                     # first call: allocations, table upload
    out = []
    for _ in range(repeats):
        s.synchronize()
        t0 = time.perf_counter()
        call()
        s.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def residual_host(x, x0, alpha, beta):
    nb = ((x[1:-1, :-2] + x[1:-1, 2:]) + x[:-2, 1:-1]) + x[2:, 1:-1]
    return np.fmax.reduce(np.abs((beta * x[1:-1, 1:-1] - alpha * nb) - x0[1:-1, 1:-1]).ravel(), initial=np.float32(0))


def host_way(s, members, fields, arithmetic, repeats):
    """median ms of the downloads of `fields` in every member, and of `arithmetic` on the arrays they return"""
    down, calc = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        arrays = {k: s.download_members(k) for k in fields}
        t1 = time.perf_counter()
        arithmetic(arrays)
        t2 = time.perf_counter()
        down.append((t1 - t0) * 1e3)
        calc.append((t2 - t1) * 1e3)
    return float(np.median(down)), float(np.median(calc))


def run(n, members, storage, repeats, host_repeats):
    rng = np.random.default_rng(n + members)
    alpha = np.linspace(0.3, 1.0, members).astype(np.float32)
    beta = (1 + 4 * alpha).astype(np.float32)
    esz = 2 if storage else 4
    field_bytes = members * (n + 2) * (n + 2) * esz
    with F.FluidSolver(n, members=members, storage=storage) as s:
        for m in range(members):
            s.upload(member=m, **{k: rng.uniform(-1, 1, size=(n + 2, n + 2)).astype(np.float32) for k in ("u", "v", "u_prev")})
        row = {"n": n, "grid": n + 2, "members": members, "storage": "f16" if storage else "f32", "field_bytes_all_members": field_bytes}
        calls = {
            "residual_members": (lambda: s.residual_members("u", "u_prev", alpha, beta), ("u", "u_prev"),
                                 lambda a: [residual_host(a["u"][m], a["u_prev"][m], alpha[m], beta[m]) for m in range(members)], 2),
            "absmax_velocity_members": (lambda: s.absmax_velocity_members("u", "v"), ("u", "v"),
                                        lambda a: [max(np.abs(a["u"][m, 1:-1, 1:-1]).max(), np.abs(a["v"][m, 1:-1, 1:-1]).max()) for m in range(members)], 2),
            "member_moments": (lambda: s.member_moments("u"), ("u",),
                               lambda a: [(x.sum(), (x * x).sum()) for x in (a["u"][m, 1:-1, 1:-1].astype(np.float64) for m in range(members))], 1),
            "ensemble_stats_device_only": (lambda: s.ensemble_stats("u", mean=False, variance=False), ("u",),
                                           lambda a: (a["u"].astype(np.float64).mean(axis=0), a["u"].astype(np.float64).var(axis=0)), 1),
            "ensemble_stats_to_host": (lambda: s.ensemble_stats("u"), None, None, 1),
        }
        for name, (call, fields, arithmetic, reads) in calls.items():
            ms = median_ms(s, call, repeats)
            r = {"ms": ms, "compulsory_bytes": reads * field_bytes, "gb_per_s": reads * field_bytes / (ms * 1e-3) / 1e9}
            if fields:
                r["host_download_ms"], r["host_numpy_ms"] = host_way(s, members, fields, arithmetic, host_repeats)
            row[name] = r
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="NxM, comma separated")
    ap.add_argument("--storage", default="f32", choices=["f32", "f16"])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    rows = []
    for case in args.cases.split(","):
        n, members = (int(v) for v in case.split("x"))
        row = run(n, members, 1 if args.storage == "f16" else 0, args.repeats, args.host_repeats)
        rows.append(row)
        for name in ("residual_members", "absmax_velocity_members", "member_moments", "ensemble_stats_device_only", "ensemble_stats_to_host"):
            r = row[name]
            host = "   host way: %9.3f ms downloads + %9.3f ms numpy" % (r["host_download_ms"], r["host_numpy_ms"]) if "host_download_ms" in r else ""
            print("N=%5d M=%5d %-28s %9.3f ms %8.1f GB/s of compulsory bytes%s" % (n, members, name, r["ms"], r["gb_per_s"], host), flush=True)
    out = {"tool": "tools/ensemble_reduce_timing.py", "commit": args.commit, "storage": args.storage, "repeats": args.repeats,
           "host_repeats": args.host_repeats, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
