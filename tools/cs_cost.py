#!/usr/bin/env python3
"""What the CIGAR and cs options cost on the device: one resident batch of synthetic 5 Mbp assemblies (the benchmark's generator)
aligned three ways -- options off, `cigar` only, `cs` -- each in a process of its own under `rocprofv3 --kernel-trace --stats`.

    python tools/cs_cost.py [--assemblies 1000] [--out-dir build/cs_cost]           # the three profiled runs, then the table
    python tools/cs_cost.py --mode cs                                               # one way, unprofiled (what the driver starts)

The table lists the per-launch durations of the CIGAR kernels (locate, count, emit) and of the cs kernels (count, emit) beside
kp_sw_traceback_kernel of the same trace, and the bytes per hit the cs strings needed.  Every profiled run has its own time limit;
the driver stops at the first one that fails.  DESIGN.md section 3 quotes the table (profiles/cs_cost_*.txt)."""

from __future__ import annotations

import argparse
import csv
import glob
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

MODES = {"off": dict(cigar=0, cs=0), "cigar": dict(cigar=1, cs=0), "cs": dict(cigar=0, cs=1)}
KERNELS = ("kp_sw_traceback_kernel", "kp_cigar_locate_tasks_kernel", "kp_cigar_locate_joins_kernel", "kp_cigar_walk_kernel<false>",
           "kp_cigar_walk_kernel<true>", "kp_cigar_scan_kernel", "kp_cs_walk_kernel<false>", "kp_cs_walk_kernel<true>")  # fmt: skip


def run_mode(mode: str, n_asm: int, seed0: int, passes: int) -> dict:
    import bench  # the generator (and the databases) of the flagship workload

    bench._load_dbs("kpsc")
    _, packed = bench.build_workload(n_asm, seed0, bench._WL["length"], workers=16)  # forked before any GPU state exists
    from kaptive_amd.engine import Engine

    dbs = [bench._DBS["main"]] + ([bench._DBS["also"]] if bench._DBS["also"] is not None else [])
    eng = Engine(dbs)
    for name, value in MODES[mode].items():
        eng.ctx.set_option(name, value)
    batch = eng.ctx.batch(packed)
    out = dict(mode=mode, assemblies=n_asm, passes=passes, wall_ms=[])
    for _ in range(passes):  # the first pass settles the buffer sizes
        t0 = time.perf_counter()
        hits, _ = batch.align()
        out["wall_ms"].append(round((time.perf_counter() - t0) * 1e3, 2))
    out["hits"] = len(hits)
    out["columns"] = int(hits["block_len"].sum())
    if MODES[mode]["cigar"] or MODES[mode]["cs"]:
        out["ops"] = int(batch.cigars()[1][-1])
    if MODES[mode]["cs"]:
        import numpy as np

        off = batch.cs()[1]
        per_hit = np.diff(off)
        out["cs_bytes"] = int(off[-1])
        out["cs_bytes_per_hit_mean"] = round(float(off[-1]) / max(len(hits), 1), 2)
        out["cs_bytes_per_hit_max"] = int(per_hit.max()) if len(per_hit) else 0
        # kp_caps_after_cs: the context keeps its first guess of 64 while the bytes fit with an eighth to spare
        need, hits_n = int(off[-1]), max(len(hits), 1)
        out["cs_bytes_per_hit_learnt"] = 64 if need + need // 8 <= 64 * hits_n else -(-(need + need // 4) // hits_n)
    batch.close()
    eng.close()
    return out


def kernel_rows(trace_dir: Path) -> dict:
    files = sorted(glob.glob(f"{trace_dir}/**/*kernel_stats.csv", recursive=True))
    rows = {}
    if not files:
        return rows
    for r in csv.DictReader(open(files[-1])):
        for k in KERNELS:
            if k in r["Name"]:
                rows[k] = dict(calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 1), min_us=round(float(r["MinNs"]) / 1e3, 1),
                               max_us=round(float(r["MaxNs"]) / 1e3, 1))  # fmt: skip
    return rows


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=sorted(MODES))
    ap.add_argument("--assemblies", type=int, default=1000)
    ap.add_argument("--seed0", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out-dir", default="build/cs_cost")
    ap.add_argument("--timeout", type=int, default=420, help="seconds per profiled run")
    args = ap.parse_args()
    if args.mode:
        print(json.dumps(run_mode(args.mode, args.assemblies, args.seed0, args.passes)), flush=True)
        return 0
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    report = {}
    for mode in ("off", "cigar", "cs"):
        cmd = ["timeout", "-k", "10", str(args.timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out_dir / mode),
               "--", sys.executable, str(Path(__file__).resolve()), "--mode", mode, "--assemblies", str(args.assemblies), "--seed0", str(args.seed0),
               "--passes", str(args.passes)]  # fmt: skip
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(ROOT))
        (out_dir / f"{mode}.log").write_text(r.stdout + "\n--- stderr ---\n" + r.stderr)
        if r.returncode != 0:  # nothing more is started on the device after a run that failed
            print(f"{mode}: exit status {r.returncode}; see {out_dir / (mode + '.log')}", file=sys.stderr)
            return 1
        line = next((ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{")), "{}")
        report[mode] = dict(run=json.loads(line), kernels=kernel_rows(out_dir / mode))
        print(f"# {mode}: {line}", flush=True)
        for k, v in report[mode]["kernels"].items():
            print(f"{mode:6s} {k:32s} calls {v['calls']:3d}  avg {v['avg_us']:9.1f} us  min {v['min_us']:9.1f}  max {v['max_us']:9.1f}", flush=True)
    (out_dir / "cs_cost.json").write_text(json.dumps(report, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
