#!/usr/bin/env python3
"""What bootstrap support of the neighbour-joining tree costs on the device (include/kp_spec.h, BOOTSTRAP;
kaptive_amd/csrc/kp_dist_boot.hip), on the population of tools/distances_probe.py: synthetic locus rows of NB = 1 600 blocks (25 600
columns) without N or GAP, so every row is a taxon.

    python tools/experiments/nj_boot_probe.py [--taxa 256 1024 4096] [--blocks 1600] [--replicates 100] [--repeats 5]
    python tools/experiments/nj_boot_probe.py --once --taxa 1024        # one warm call of each kind, for a kernel trace

Per size, after one warm-up of each, `repeats` timed rounds that alternate
  (a) kp_dist_nj_bootstrap with `replicates` replicates, and
  (b) the yardstick: `replicates` sequential kp_dist_nj calls on the same handle -- what a loop without the batched call would cost,
      with no resampling at all.
Each call is timed by a host clock and ends in a synchronise.  One JSON line per size: the medians, the spread, the batch the
library chose and the launches of the join loops.  (c), the weighted matrix fill against kp_dist_nj's fill, is a ratio of kernel
times: run `--once` under `rocprofv3 --kernel-trace --stats` and compare kp_dist_boot_kernel (per replicate) with
kp_dist_nj_kernel (per call).  DESIGN.md quotes the lines; nothing is gated on them."""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from tools.distances_probe import population  # noqa: E402


def run(n: int, blocks: int, replicates: int, repeats: int, once: bool) -> dict:
    from kaptive_amd import _native

    m = population(n, blocks)
    ctx = _native.Context(0)
    try:
        with _native.Distances(ctx, m) as d:
            taxa, nodes = d.nj(1)  # (warm-up of the yardstick, and the tree to support)
            support = d.nj_support(1, nodes, replicates)  # (warm-up of the call)
            a_ms, b_ms = [], []
            for _ in range(1 if once else repeats):
                t0 = time.perf_counter()
                again = d.nj_support(1, nodes, replicates)
                a_ms.append(1e3 * (time.perf_counter() - t0))
                assert again.tobytes() == support.tobytes()
                t0 = time.perf_counter()
                for _ in range(1 if once else replicates):
                    d.nj(1)
                b_ms.append(1e3 * (time.perf_counter() - t0))
    finally:
        ctx.close()
    k = len(taxa)
    batch = max(1, min(replicates, _native.BOOT_MAX_BATCH, _native.BOOT_MATRIX_BYTES // (k * k * 8)))
    batches = -(-replicates // batch)
    held = support[: max(k - 3, 0)]
    return {"taxa": int(k), "blocks": blocks, "replicates": replicates, "batch": int(batch), "batches": int(batches), "joins": max(k - 3, 0),
            "launches_of_the_joins_bootstrap": 4 * max(k - 3, 0) * batches, "launches_of_the_joins_loop": 4 * max(k - 3, 0) * replicates,
            "bootstrap_ms_median": round(statistics.median(a_ms), 2), "bootstrap_ms": [round(x, 2) for x in a_ms],
            "nj_loop_ms_median": round(statistics.median(b_ms), 2), "nj_loop_ms": [round(x, 2) for x in b_ms], "nj_loop_calls": 1 if once else replicates,
            "support_mean": round(float(held.mean()), 2) if len(held) else None, "support_full": int((held == replicates).sum())}  # fmt: skip


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--taxa", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--blocks", type=int, default=1600)
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="one warm call of each kind per size: the run to trace")
    a = ap.parse_args()
    for n in a.taxa:
        print(json.dumps(run(n, a.blocks, a.replicates, a.repeats, a.once)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
