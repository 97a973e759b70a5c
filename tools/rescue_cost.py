#!/usr/bin/env python3
"""What the `rescue` option costs on the device: a resident batch of synthetic 5 Mbp assemblies against the headline's synthetic K
database, each assembly carrying its locus with ONE expected gene recoded codon by codon (kaptive_amd.synth.recode_orf: no shared
15-mer, a protein three quarters identical) -- the gene a nucleotide seed misses.

    python tools/rescue_cost.py [--out-dir build/rescue_cost]         # the kernels under rocprofv3 (a kernel trace only), then a table
    python tools/rescue_cost.py --run [--assemblies 512] [--passes 6]  # unprofiled (what the driver starts)

`--run` prints one JSON line: wall milliseconds of every typing pass (alignment, reduction, records) with the option on and off --
two engines over the same device words, the passes alternating --, their medians over the settled passes as ms per 1000 assemblies,
the missing genes, windows and cells of the score-only fill (rows of every frame text x residues of the protein), and those cells over
the time the option adds.  The profiled run adds the per-launch durations of the kernels of kp_rescue.hip and the score-only fill's
cells per second.  DESIGN.md quotes both (profiles/rescue_cost.txt)."""

from __future__ import annotations

import argparse
import csv
import glob
import json
import statistics
import subprocess
import sys
import time
from multiprocessing import get_context
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

KERNELS = ("kp_rescue_plan_kernel", "kp_rescue_fill_kernel<false>", "kp_rescue_pick_kernel", "kp_rescue_fill_kernel<true>")
_DB: dict = {}


def _make_one(job):
    """One assembly: an iid background with locus `li` planted in one piece, one of its forward-strand genes recoded."""
    import numpy as np

    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.synth import random_dna, recode_orf

    seed, length = job
    db = _DB["main"]
    rng = np.random.default_rng(seed)
    li = int(rng.integers(len(db.loci)))
    o, n = int(db.loci.offsets[li]), int(db.loci.lengths[li])
    locus = np.asarray(db.loci.seqs[o : o + n], np.uint8).copy()
    g0, ng = int(db.locus_gene_offsets[li]), int(db.locus_gene_lengths[li])
    fwd = [g for g in range(g0 + 4, g0 + ng - 4) if db.gene_intervals.strands[g] > 0]  # (a gene of the locus's own, not one of the shared families)
    g = fwd[int(rng.integers(len(fwd)))]
    s, e = int(db.gene_intervals.starts[g]), int(db.gene_intervals.ends[g])
    locus[s:e] = recode_orf(rng, locus[s:e])
    total = int(length)
    at = int(rng.integers(total // 4, total // 2))
    contigs = [np.concatenate([random_dna(rng, at, 0.57), locus, random_dna(rng, total // 2 - at, 0.57)]), random_dna(rng, total // 2, 0.57)]
    genome = GenomeAssembly(f"asm{seed}", Sequences.from_records([SeqRecord(f"c{i}", np.ascontiguousarray(c).tobytes()) for i, c in enumerate(contigs)]))
    return genome.id, genome.packed(), g


def _setup(n_asm: int, seed0: int, workers: int):
    import bench  # the databases of the flagship workload

    bench._load_dbs("kpsc")
    _DB["main"] = bench._DBS["main"]
    jobs = [(seed0 + i, bench._WL["length"]) for i in range(n_asm)]
    with get_context("fork").Pool(workers) as pool:  # forked before any GPU state exists
        rows = pool.map(_make_one, jobs, chunksize=4)
    return _DB["main"], [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]


def run(n_asm: int, seed0: int, passes: int, workers: int) -> dict:
    import numpy as np

    from kaptive_amd import _native
    from kaptive_amd.engine import Engine
    from kaptive_amd.serotyping.core import Serotyper

    db, ids, packed, edited = _setup(n_asm, seed0, workers)
    legs, first = {}, None
    for on in (True, False):  # two engines, one resident copy of the words
        eng = Engine(db, rescue=on)
        b = eng.ctx.batch(packed) if first is None else eng.ctx.batch(packed, device_words=first.device_words, after=first)
        first = b if first is None else first
        legs[on] = (eng, Serotyper(db, rescue=on), b)
    wall = {True: [], False: []}
    typed = {}
    for p in range(passes + 1):  # the first pass settles the buffer sizes
        for on in ((True, False) if p % 2 == 0 else (False, True)):
            eng, typer, b = legs[on]
            t0 = time.perf_counter()
            b.align_async()
            typed[on] = eng.type_batch(typer, b, ids, aligned=True)
            wall[on].append(round((time.perf_counter() - t0) * 1e3, 2))
    bt = typed[True]
    records, off = bt.rescue()
    prot_len = np.asarray(db.translations.lengths, np.int64)
    flank = _native.RESCUE_FLANK
    cells = windows = 0
    for a, pa in enumerate(packed):
        rows = 0
        for pc in bt.pieces[a, : int(bt.sums["n_pieces"][a])]:
            ws, we = max(0, int(pc["start"]) - flank), min(int(pa.ctg_len[int(pc["contig"])]), int(pc["end"]) + flank)
            rows += 2 * sum(max(0, (we - ws - f) // 3) for f in range(3))
            windows += 1
        cells += rows * int(prot_len[records["gene"][off[a] : off[a + 1]]].sum())
    found = sum(int(records["gene"][i]) == edited[a] and int(records["score"][i]) >= _native.RESCUE_MIN_SCORE
                for a in range(n_asm) for i in range(int(off[a]), int(off[a + 1])))  # fmt: skip
    med = {on: statistics.median(wall[on][1:]) for on in wall}
    out = dict(assemblies=n_asm, passes=passes, wall_ms_on=wall[True], wall_ms_off=wall[False],
               ms_per_1000_on=round(med[True] * 1000 / n_asm, 2), ms_per_1000_off=round(med[False] * 1000 / n_asm, 2),
               missing_genes=int(len(records)), windows=windows, edited_found=int(found), score_only_cells=int(cells),
               cells_per_s_of_added_time=round(cells / max(1e-9, (med[True] - med[False]) * 1e-3)), tsv_same=bt.tsv() == typed[False].tsv())  # fmt: skip
    legs[False][2].close()  # (it reads the first batch's device words: closed before it)
    first.close()
    for on in legs:
        legs[on][0].close()
    return out


def kernel_rows(trace_dir: Path) -> dict:
    files = sorted(glob.glob(f"{trace_dir}/**/*kernel_stats.csv", recursive=True))
    out = {}
    if files:
        for r in csv.DictReader(open(files[-1])):
            for k in KERNELS:
                if k in r["Name"]:
                    out[k] = dict(calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 1), min_us=round(float(r["MinNs"]) / 1e3, 1),
                                  max_us=round(float(r["MaxNs"]) / 1e3, 1))  # fmt: skip
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--assemblies", type=int, default=512)
    ap.add_argument("--seed0", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=6)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out-dir", default="build/rescue_cost")
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the profiled run")
    args = ap.parse_args()
    if args.run:
        print(json.dumps(run(args.assemblies, args.seed0, args.passes, args.workers)), flush=True)
        return 0
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(args.timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out_dir / "trace"),
           "--", sys.executable, str(Path(__file__).resolve()), "--run", "--assemblies", str(args.assemblies), "--seed0", str(args.seed0),
           "--passes", str(args.passes), "--workers", str(args.workers)]  # fmt: skip
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(ROOT))
    (out_dir / "run.log").write_text(r.stdout + "\n--- stderr ---\n" + r.stderr)
    if r.returncode != 0:
        print(f"exit status {r.returncode}; see {out_dir / 'run.log'}", file=sys.stderr)
        return 1
    line = next((ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{")), "{}")
    report = dict(run=json.loads(line), kernels=kernel_rows(out_dir / "trace"))
    print(f"# {line}", flush=True)
    for k, v in report["kernels"].items():
        print(f"{k:30s} calls {v['calls']:3d}  avg {v['avg_us']:10.1f} us  min {v['min_us']:10.1f}  max {v['max_us']:10.1f}", flush=True)
    fill = report["kernels"].get("kp_rescue_fill_kernel<false>")
    if fill and report["run"].get("score_only_cells"):
        print(f"score-only fill: {report['run']['score_only_cells'] / (fill['avg_us'] * 1e-6):.3e} cells/s", flush=True)
    (out_dir / "rescue_cost.json").write_text(json.dumps(report, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
