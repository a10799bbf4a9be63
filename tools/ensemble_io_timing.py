#!/usr/bin/env python3
"""Moving whole ensembles (fluid_pack_members / fluid_unpack_members, fluid_download_members / fluid_upload_members,
fluid_run): what each costs beside the way to the same data without it.

Per (N, M) and storage type, uniform random fields in every member:
- pack and unpack of one field: device time between two events on the stream the library shares with this tool (the
  constructor's stream=, wait=False), median over --repeats; and the effective bandwidth against the compulsory bytes,
  4 + sizeof(S) per cell (one dense float and one stored element);
- the same rows moved by M hipMemcpy2DAsync device-to-device copies between the same events: for fp32 what a caller can do
  today through fluid_field_ptr; for fp16 the copies move the stored halves as they are (no widening: fewer bytes, and not
  the same result -- the line is there for the launch count alone);
- fluid_download_members / fluid_upload_members beside the loops of M fluid_download_member / fluid_upload_member calls
  they replace: wall time, median over --host-repeats;
- a forced, recorded run (--steps steps, sources before every step, three fields recorded after every second step)
  beside the same steps driven call by call from Python (3 unpacks, one step, 3 packs on the same shared stream, no wait
  in between): wall time between two synchronises.

Prints a table and writes JSON (--out).
    python tools/ensemble_io_timing.py [--cases 256x16,1024x16] [--storage f32,f16] [--out profiles/ensemble_io_timing.json]"""
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

DEFAULT_CASES = "256x16,256x64,1024x16,4094x4,64x4096"
RECORDED = ("u", "v", "dens")


def hip_runtime():
    """the HIP runtime this process already holds (the one libfluid_amd.so runs on)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            lib = C.CDLL(line.split()[-1])
            lib.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
            lib.hipMemcpy2DAsync.restype = C.c_int
            return lib
    raise RuntimeError("no HIP runtime is loaded")


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
    return float(np.median(out))


def wall_ms(s, call, repeats):
    call()
    out = []
    for _ in range(repeats):
        s.synchronize()
        t0 = time.perf_counter()
        call()
        s.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def run(n, members, storage, repeats, host_repeats, steps, iters):
    import torch
    hip = hip_runtime()
    w, esz = n + 2, 2 if storage else 4
    cells = w * w
    pitch, xoff, ff = C.c_int(), C.c_int(), C.c_size_t()
    capi.check(capi.lib().fluid_layout(n, C.byref(pitch), C.byref(xoff), C.byref(ff)))
    rng = np.random.default_rng(n + members)
    stream = torch.cuda.Stream()
    row = {"n": n, "grid": w, "members": members, "storage": "f16" if storage else "f32",
           "compulsory_bytes": members * cells * (4 + esz)}
    with torch.cuda.stream(stream), F.FluidSolver(n, members=members, storage=storage, stream=stream.cuda_stream) as s:
        host = rng.uniform(-1, 1, size=(members, w, w)).astype(np.float32)
        for k in ("u", "v", "dens"):
            s.upload_members(**{k: host})
        dense = torch.empty((members, w, w), dtype=torch.float32, device="cuda")
        for name, call in (("pack", lambda: s.pack("u", out=dense, wait=False)), ("unpack", lambda: s.unpack("u", dense, wait=False))):
            ms = device_ms(torch, stream, call, repeats)
            row[name] = {"device_ms": ms, "gb_per_s": row["compulsory_bytes"] / (ms * 1e-3) / 1e9}
        # the same rows as M two-dimensional copies out of the library's layout
        raw = torch.empty(members * cells * esz, dtype=torch.uint8, device="cuda")
        base = s.field_ptr("u") + xoff.value * esz

        def copies():
            for m in range(members):
                rc = hip.hipMemcpy2DAsync(raw.data_ptr() + m * cells * esz, w * esz, base + m * ff.value * esz, pitch.value * esz, w * esz, w,
                                          3, stream.cuda_stream)          # hipMemcpyDeviceToDevice
                assert rc == 0, rc

        ms = device_ms(torch, stream, copies, repeats)
        row["memcpy2d_per_member"] = {"device_ms": ms, "bytes": 2 * members * cells * esz, "gb_per_s": 2 * members * cells * esz / (ms * 1e-3) / 1e9}
        # bulk host copies beside the per-member loops
        out = np.empty_like(host)
        L, h = capi.lib(), s._h

        def loop_down():
            for m in range(members):
                capi.check(L.fluid_download_member(h, m, 0, out[m]))

        def loop_up():
            for m in range(members):
                capi.check(L.fluid_upload_member(h, m, 0, host[m]))

        row["download_members"] = {"ms": wall_ms(s, lambda: s.download_members("u", out=out), host_repeats), "loop_ms": wall_ms(s, loop_down, host_repeats)}
        row["upload_members"] = {"ms": wall_ms(s, lambda: s.upload_members(u=host), host_repeats), "loop_ms": wall_ms(s, loop_up, host_repeats)}
        # a forced, recorded run beside the same steps call by call
        sources = torch.from_numpy((rng.uniform(-1, 1, size=(3, members, w, w)) * 0.1).astype(np.float32)).cuda()
        snaps = torch.empty((steps // 2, len(RECORDED), members, w, w), dtype=torch.float32, device="cuda")

        def run_call():
            s.run(steps, every=2, fields=RECORDED, sources=sources, out=snaps, iters=iters, wait=False)

        def by_call():
            for z in range(steps):
                for k, name in enumerate(("u_prev", "v_prev", "dens_prev")):
                    s.unpack(name, sources[k], wait=False)
                s.step(1, use_sources=True, iters=iters)
                if z % 2 == 1:
                    for k, name in enumerate(RECORDED):
                        s.pack(name, out=snaps[z // 2, k], wait=False)

        for _ in range(40):                  # the strip-height tuner measures during the first steps of a shape
            if not s.autotune_pending():
                break
            run_call()
        row["run"] = {"steps": steps, "iters": iters, "ms": wall_ms(s, run_call, host_repeats), "call_by_call_ms": wall_ms(s, by_call, host_repeats)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="NxM, comma separated")
    ap.add_argument("--storage", default="f32,f16")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    rows = []
    for storage in args.storage.split(","):
        for case in args.cases.split(","):
            n, members = (int(v) for v in case.split("x"))
            r = run(n, members, 1 if storage == "f16" else 0, args.repeats, args.host_repeats, args.steps, args.iters)
            rows.append(r)
            print("N=%5d M=%5d %s  pack %8.3f ms %7.1f GB/s  unpack %8.3f ms %7.1f GB/s  %d x memcpy2D %8.3f ms | download %9.2f ms (loop %9.2f)  "
                  "upload %9.2f ms (loop %9.2f) | run %9.2f ms (call by call %9.2f)" % (
                      n, members, storage, r["pack"]["device_ms"], r["pack"]["gb_per_s"], r["unpack"]["device_ms"], r["unpack"]["gb_per_s"], members,
                      r["memcpy2d_per_member"]["device_ms"], r["download_members"]["ms"], r["download_members"]["loop_ms"], r["upload_members"]["ms"],
                      r["upload_members"]["loop_ms"], r["run"]["ms"], r["run"]["call_by_call_ms"]), flush=True)
    out = {"tool": "tools/ensemble_io_timing.py", "commit": args.commit, "repeats": args.repeats, "host_repeats": args.host_repeats, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
