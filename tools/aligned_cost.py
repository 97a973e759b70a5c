#!/usr/bin/env python3
"""What the `aligned` option costs on the device: resident batches of synthetic 5 Mbp assemblies (the benchmark's generator, the shape
tools/alleles_cost.py uses), K + O typed in one pass through `Engine.type_stream_groups`.

    python tools/aligned_cost.py --ab [--assemblies 1000] [--repeats 6] [--steps 4]   # option on and off, alternating, one process
    python tools/aligned_cost.py [--out-dir build/aligned_cost]                        # the kernels under rocprofv3, then their table
    python tools/aligned_cost.py --run                                                 # unprofiled (what the driver starts)

`--ab` prints one JSON line: assemblies per second of every repeat with the option on and off (two engines over the same device
words, the repeats alternating) and their medians and spreads; the option-on leg also computes the CIGARs, as the option implies.
The profiled run (`rocprofv3 --kernel-trace --stats`, a kernel trace only: no counters in the same run) prints the per-launch
durations of the pass's kernels -- kp_kept_locate_kernel, kp_aligned_count_kernel, kp_aligned_emit_kernel -- and, per typing group,
the kept rows, the ops read and the blocks written.  DESIGN.md quotes both (profiles/aligned_cost.txt)."""

from __future__ import annotations

import argparse
import csv
import glob
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

KERNELS = ("kp_kept_locate_kernel", "kp_aligned_count_kernel", "kp_aligned_emit_kernel")


def _setup(n_asm: int, seed0: int):
    import bench  # the generator (and the databases) of the flagship workload

    bench._load_dbs("kpsc")
    _, packed = bench.build_workload(n_asm, seed0, bench._WL["length"], workers=16)  # forked before any GPU state exists
    dbs = [bench._DBS["main"]] + ([bench._DBS["also"]] if bench._DBS["also"] is not None else [])
    return dbs, packed


def _engine(dbs, aligned: bool):
    from kaptive_amd.engine import Engine
    from kaptive_amd.serotyping.core import Serotyper

    return Engine(dbs, aligned=aligned), [Serotyper(d) for d in dbs]


def run_ab(n_asm: int, seed0: int, repeats: int, steps: int) -> dict:
    from kaptive_amd import _native

    dbs, packed = _setup(n_asm, seed0)
    ids = [f"asm{i}" for i in range(n_asm)]
    legs = {}
    first = None
    for on in (True, False):  # two engines, one resident copy of the words; each with enough batch objects for the stream's window
        eng, typers = _engine(dbs, on)
        batches = []
        for _ in range(_native.WORK_SLOTS + 1):
            b = eng.ctx.batch(packed) if first is None else eng.ctx.batch(packed, device_words=first.device_words, after=first)
            first = b if first is None else first
            batches.append(b)
        legs[on] = (eng, typers, batches)

    def one(on: bool, n: int) -> float:
        eng, typers, batches = legs[on]
        t0 = time.perf_counter()
        done = 0
        for groups, _ in eng.type_stream_groups(typers, ((batches[i % len(batches)], ids, None) for i in range(n))):
            done += len(groups[0].tsv()) > 0
        assert done == n
        return n_asm * n / (time.perf_counter() - t0)

    for on in (True, False):  # buffer sizing, untimed
        one(on, len(legs[on][2]))
    rates = {True: [], False: []}
    for r in range(repeats):
        for on in ((True, False) if r % 2 == 0 else (False, True)):
            rates[on].append(round(one(on, steps), 1))
    out = dict(assemblies=n_asm, steps=steps, repeats=repeats, databases=[d.metadata.keyword for d in dbs])
    for on, key in ((True, "aligned_on"), (False, "aligned_off")):
        v = rates[on]
        out[key] = dict(assemblies_per_s=v, median=round(statistics.median(v), 1), min=min(v), max=max(v))
    out["median_on_over_off"] = round(out["aligned_on"]["median"] / out["aligned_off"]["median"], 4)
    for eng, _, batches in legs.values():
        for b in reversed(batches):
            if b is not first:
                b.close()
    first.close()
    for eng, _, _ in legs.values():
        eng.close()
    return out


def run(n_asm: int, seed0: int, passes: int) -> dict:
    dbs, packed = _setup(n_asm, seed0)
    eng, typers = _engine(dbs, True)
    ids = [f"asm{i}" for i in range(n_asm)]
    batch = eng.ctx.batch(packed)
    out = dict(assemblies=n_asm, passes=passes, wall_ms=[], groups=[])
    for _ in range(passes):  # the first pass settles the buffer sizes
        t0 = time.perf_counter()
        batch.align_async()
        typed = [eng.view(g).type_batch(t, batch, ids, aligned=True) for g, t in enumerate(typers)]
        out["wall_ms"].append(round((time.perf_counter() - t0) * 1e3, 2))
    ops, coff = batch.cigars()
    hits, hoff = batch.hits()
    for d, bt in zip(dbs, typed):
        rows, blocks = bt.aligned()
        nk = bt.sums["n_kept"]
        live = np.arange(rows.shape[1])[None, :] < nk[:, None]
        r = rows[live]
        out["groups"].append(dict(database=d.metadata.keyword, kept_rows=int(nk.sum()), blocks=int(len(blocks)), bytes_written=8 * int(len(blocks)) + 24 * int(nk.sum()),
                                  columns=int(r["gene_len"].sum()), covered=int(r["covered"].sum()), inserted=int(r["inserted"].sum()),
                                  rows_with_gaps_inside=int((r["covered"] < (bt.kept["q_end"] - bt.kept["q_start"])[live]).sum()),
                                  longest_gene=int(r["gene_len"].max()) if len(r) else 0))  # fmt: skip
    out["hits"], out["ops"] = int(len(hits)), int(len(ops))
    batch.close()
    eng.close()
    return out


def kernel_rows(trace_dir: Path) -> dict:
    files = sorted(glob.glob(f"{trace_dir}/**/*kernel_stats.csv", recursive=True))
    out = {}
    if not files:
        return out
    for r in csv.DictReader(open(files[-1])):
        for k in KERNELS:
            if k in r["Name"]:
                out[k] = dict(calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 1), min_us=round(float(r["MinNs"]) / 1e3, 1),
                              max_us=round(float(r["MaxNs"]) / 1e3, 1), total_us=round(float(r["TotalDurationNs"]) / 1e3, 1) if "TotalDurationNs" in r else None)  # fmt: skip
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--assemblies", type=int, default=1000)
    ap.add_argument("--seed0", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--out-dir", default="build/aligned_cost")
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the profiled run")
    args = ap.parse_args()
    if args.ab:
        print(json.dumps(run_ab(args.assemblies, args.seed0, args.repeats, args.steps)), flush=True)
        return 0
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
    for name, k in report["kernels"].items():
        print(f"{name:26s} calls {k['calls']:3d}  avg {k['avg_us']:9.1f} us  min {k['min_us']:9.1f}  max {k['max_us']:9.1f}", flush=True)
    for g in report["run"].get("groups", []):
        print(f"  {g['database']}: {g['kept_rows']} kept rows, {g['columns']} columns, {g['blocks']} blocks, {g['bytes_written']} bytes written", flush=True)
    (out_dir / "aligned_cost.json").write_text(json.dumps(report, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
