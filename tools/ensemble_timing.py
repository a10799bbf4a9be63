#!/usr/bin/env python3
"""Ensembles (FluidSolver(n, members=M)): wall time per ensemble step over grid sizes and member counts, on the reference's
workload -- initialize_parameters per member with different seeds, one sourced step, then plain steps ("decay": what
bench.py runs, the fields shrink towards zero) -- and once more with the sources uploaded again before every step
("sourced": the fields keep their magnitude).

Per (N, M): untimed steps until the strip-height tuner has settled (fluid_autotune_pending == 0, or --max-tune steps), then
wall time between fluid_synchronize pairs, the median of --blocks blocks.  "decay": a block is --steps steps between one
pair.  "sourced": every step sits between its own pair, with the uploads outside it (a block is the sum of --steps such
steps), so it carries one host round trip per step that "decay" does not.  One process, one context at a time.

--member-params picks the kind of call: "scalar" (default) -- fluid_step with one dt, diff, visc for everybody; "constant" --
fluid_step_members with arrays that hold those same values; "ladder" -- fluid_step_members with member m's own visc and
diff, a geometric ladder around the defaults from x 1/2 to x 2 (dt shared; the ladder is written into the JSON).  The
division proofs of the ladder's betas (one per distinct beta and process) run in the untimed steps.

Prints a table and writes JSON (--out): ms per ensemble step, ms per member-step, member-steps per second, the gain over
M one-member steps (the M = 1 row of the same run), and the strip heights the tuner kept for each launch shape.
    python tools/ensemble_timing.py [--sizes 64,256] [--members 1,16] [--member-params ladder]
                                    [--out profiles/ensemble_timing.json] [--commit ID]"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluidsimulationcuda_amd as F  # noqa: E402
from fluidsimulationcuda_amd.harness import initialize_parameters  # noqa: E402

SOURCES = ("u_prev", "v_prev", "dens_prev")


class TunerLog:
    """the library reports each strip height it keeps on stderr (FLUID_TUNE_LOG): file descriptor 2 goes to a file while a
    configuration runs"""

    def __enter__(self):
        sys.stderr.flush()
        self.saved = os.dup(2)
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
        self.kept = [{"shape": m.group(1), "rows": int(m.group(2))}
                     for m in re.finditer(r"\[fluid tune\] key \w+ \[([^\]]*)\] -> (\d+) rows", text)]
        rest = "\n".join(line for line in text.splitlines() if "[fluid tune]" not in line)
        if rest.strip():
            sys.stderr.write(rest + "\n")


def ladder(members):
    """x 2^-1 ... x 2^+1 in equal ratios (one member: x 1)"""
    if members == 1:
        return np.ones(1)
    return 2.0 ** (2.0 * np.arange(members) / (members - 1) - 1.0)


def member_params(members, kind):
    """keyword arguments of FluidSolver.step for this kind of call, and what goes into the JSON"""
    if kind == "scalar":
        return {}, None
    factor = ladder(members) if kind == "ladder" else np.ones(members)
    kw = {"dt": np.full(members, F.solver.DT, np.float32), "diff": (F.solver.DIFF * factor).astype(np.float32),
          "visc": (F.solver.VIS * factor).astype(np.float32)}
    return kw, {k: [float(x) for x in v] for k, v in kw.items()}


def run(n, members, workload, args):
    fields = [initialize_parameters(n, seed=1 + m) for m in range(members)]
    sourced = workload == "sourced"
    kw, recorded = member_params(members, args.member_params)

    def inject(s):
        for m, f in enumerate(fields):
            s.upload(member=m, **{k: f[k] for k in SOURCES})

    with TunerLog() as log, F.FluidSolver(n, members=members) as s:
        for m, f in enumerate(fields):
            s.upload(member=m, **f)
        s.step(1, use_sources=True, **kw)
        tune_steps = 0
        while tune_steps < args.max_tune and (tune_steps < 2 or s.autotune_pending() > 0):
            if sourced:
                inject(s)
            s.step(1, use_sources=sourced, **kw)
            tune_steps += 1
        s.synchronize()
        pending = s.autotune_pending()
        blocks = []
        for _ in range(args.blocks):
            if sourced:
                t = 0.0
                for _ in range(args.steps):
                    inject(s)
                    s.synchronize()
                    t0 = time.perf_counter()
                    s.step(1, use_sources=True, **kw)
                    s.synchronize()
                    t += time.perf_counter() - t0
            else:
                s.synchronize()
                t0 = time.perf_counter()
                s.step(args.steps, **kw)
                s.synchronize()
                t = time.perf_counter() - t0
            blocks.append(t / args.steps * 1e3)
        absmax = s.absmax_velocity()
    ms = float(np.median(blocks))
    return {"n": n, "grid": n + 2, "members": members, "workload": workload, "member_params": args.member_params,
            "member_values": recorded, "ms_per_ensemble_step": ms,
            "ms_per_member_step": ms / members, "member_steps_per_s": members / (ms * 1e-3), "blocks_ms": blocks,
            "tune_steps": tune_steps, "shapes_still_open": pending, "absmax_velocity_after": absmax, "strip_heights": log.kept}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256,512,1024,2046,4094")
    ap.add_argument("--members", default="1,2,4,8,16,64")
    ap.add_argument("--workloads", default="sourced,decay")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--max-tune", type=int, default=80)
    ap.add_argument("--max-gib", type=float, default=24.0, help="largest arena (12 fields x members) that still counts as comfortable")
    ap.add_argument("--max-upload-gib", type=float, default=1.0, help="'sourced' uploads 3 fields x members per step: skipped beyond this")
    ap.add_argument("--member-params", default="scalar", choices=["scalar", "constant", "ladder"],
                    help="scalar: fluid_step; constant / ladder: fluid_step_members with the defaults / a x1/2..x2 ladder of visc and diff")
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    if args.blocks < 5:
        ap.error("--blocks: the median is taken over at least five")
    os.environ["FLUID_TUNE_LOG"] = "1"
    rows, skipped = [], []
    for n in [int(v) for v in args.sizes.split(",")]:
        base = {}
        for members in [int(v) for v in args.members.split(",")]:
            arena = F.capi.lib().fluid_arena_bytes_ensemble(n, F.capi.STORAGE_F32, members)
            if arena == 0 or arena > args.max_gib * 2 ** 30:
                skipped.append({"n": n, "members": members, "why": "arena of %.1f GiB" % (arena / 2 ** 30)})
                continue
            for workload in args.workloads.split(","):
                if workload == "sourced" and arena / 4 > args.max_upload_gib * 2 ** 30:
                    skipped.append({"n": n, "members": members, "workload": workload, "why": "uploads of %.1f GiB per step" % (arena / 4 / 2 ** 30)})
                    continue
                r = run(n, members, workload, args)
                if members == 1:
                    base[workload] = r["ms_per_ensemble_step"]
                if workload in base:
                    r["gain_over_one_member_steps"] = base[workload] * members / r["ms_per_ensemble_step"]
                rows.append(r)
                heights = sorted(set(h["rows"] for h in r["strip_heights"]))
                print("N=%5d M=%3d %-7s %9.3f ms/ensemble step %8.4f ms/member-step %10.0f member-steps/s  x%5.2f vs M one-member steps   "
                      "tuned in %2d steps (%d open), strip heights kept: %s"
                      % (n, members, workload, r["ms_per_ensemble_step"], r["ms_per_member_step"], r["member_steps_per_s"],
                         r.get("gain_over_one_member_steps", float("nan")), r["tune_steps"], r["shapes_still_open"], heights), flush=True)
    out = {"tool": "tools/ensemble_timing.py", "commit": args.commit, "member_params": args.member_params, "steps_per_block": args.steps, "blocks": args.blocks,
           "dt": F.solver.DT, "diff": F.solver.DIFF, "visc": F.solver.VIS, "iters": F.solver.ITERS, "rows": rows, "skipped": skipped}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
