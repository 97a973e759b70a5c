#!/usr/bin/env python3
"""What the `breakpoints` option costs on the device: one resident batch of synthetic 5 Mbp assemblies (the benchmark's generator,
the shape tools/variants_cost.py uses) aligned and typed with `variants` and `breakpoints` on, in a process of its own under
`rocprofv3 --kernel-trace --stats` (a kernel trace only: no counters in the same run).

    python tools/breakpoints_cost.py [--assemblies 1000] [--out-dir build/breakpoints_cost]   # the profiled run, then the table
    python tools/breakpoints_cost.py --run                                                     # unprofiled (what the driver starts)

The table lists the per-launch durations of the kernels of the pass (pairs, scan, compact) beside the variant pass's of the same
trace, the number of kept records and of breakpoint records by event and the bytes of the TSV.  DESIGN.md section 3 quotes it
(profiles/breakpoints_cost.txt)."""

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

KERNELS = ("kp_breakpoints_pair_kernel", "kp_breakpoints_compact_kernel", "kp_cigar_scan_kernel", "kp_variants_walk_kernel<false>",
           "kp_variants_walk_kernel<true>")  # fmt: skip (the scan serves the CIGARs, the variants and the breakpoints: its row is all of them)


def run(n_asm: int, seed0: int, passes: int) -> dict:
    import numpy as np

    import bench  # the generator (and the databases) of the flagship workload

    bench._load_dbs("kpsc")
    _, packed = bench.build_workload(n_asm, seed0, bench._WL["length"], workers=16)  # forked before any GPU state exists
    from kaptive_amd import _native
    from kaptive_amd.engine import Engine
    from kaptive_amd.serotyping.core import Serotyper

    dbs = [bench._DBS["main"]] + ([bench._DBS["also"]] if bench._DBS["also"] is not None else [])
    eng = Engine(dbs, variants=True, breakpoints=True)
    typers = [Serotyper(d) for d in dbs]
    ids = [f"asm{i}" for i in range(n_asm)]
    batch = eng.ctx.batch(packed)
    out = dict(assemblies=n_asm, passes=passes, wall_ms=[], groups=[])
    for _ in range(passes):  # the first pass settles the buffer sizes
        t0 = time.perf_counter()
        batch.align_async()
        typed = [eng.view(g).type_batch(t, batch, ids, aligned=True) for g, t in enumerate(typers)]
        out["wall_ms"].append(round((time.perf_counter() - t0) * 1e3, 2))
    out["hits"] = int(batch.hits()[1][-1])
    first = np.concatenate([[0], np.cumsum([len(pa.ctg_start) for pa in packed])]).astype(np.int64)
    names = [f"c{i}" for i in range(int(first[-1]))]
    for d, t, bt in zip(dbs, typers, typed):
        records, bp_off = bt.breakpoints()
        tsv = _native.format_breakpoints(d.genes.ids, ids, names, first, bt.kept, records, bp_off, t.partial_edge_tolerance)
        events: dict = {}
        for line in tsv.splitlines():
            e = line.split(b"\t")[2].decode()
            events[e] = events.get(e, 0) + 1
        out["groups"].append(dict(database=d.metadata.keyword, kept_records=int(bt.sums["n_kept"].sum()), variant_records=len(bt.variants()[0]),
                                  breakpoint_records=len(records), assemblies_with_a_record=int((np.diff(bp_off) > 0).sum()), events=events,
                                  tsv_bytes=len(tsv)))  # fmt: skip
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
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--assemblies", type=int, default=1000)
    ap.add_argument("--seed0", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out-dir", default="build/breakpoints_cost")
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the profiled run")
    args = ap.parse_args()
    if args.run:
        print(json.dumps(run(args.assemblies, args.seed0, args.passes)), flush=True)
        return 0
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(args.timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out_dir / "trace"),
           "--", sys.executable, str(Path(__file__).resolve()), "--run", "--assemblies", str(args.assemblies), "--seed0", str(args.seed0),
           "--passes", str(args.passes)]  # fmt: skip
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(ROOT))
    (out_dir / "run.log").write_text(r.stdout + "\n--- stderr ---\n" + r.stderr)
    if r.returncode != 0:
        print(f"exit status {r.returncode}; see {out_dir / 'run.log'}", file=sys.stderr)
        return 1
    line = next((ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{")), "{}")
    report = dict(run=json.loads(line), kernels=kernel_rows(out_dir / "trace"))
    print(f"# {line}", flush=True)
    for k, v in report["kernels"].items():
        print(f"{k:32s} calls {v['calls']:3d}  avg {v['avg_us']:9.1f} us  min {v['min_us']:9.1f}  max {v['max_us']:9.1f}", flush=True)
    (out_dir / "breakpoints_cost.json").write_text(json.dumps(report, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
