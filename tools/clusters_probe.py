#!/usr/bin/env python3
"""What clusters and nearest neighbours cost on the device beside the count pass of the same matrix (include/kp_spec.h, CLUSTERS;
kaptive_amd/csrc/kp_dist_graph.hip), at the shape of tools/distances_probe.py: R = 10 000 synthetic locus rows of NB = 1 600 blocks
(25 600 columns), 5e7 pairs.

    python tools/clusters_probe.py [--rows 10000] [--blocks 1600] [--repeats 5]           # clusters of 100 rows: 1 % of the pairs within 10
    python tools/clusters_probe.py --dense                                                  # every row drawn from one founder
    python tools/clusters_probe.py --lib PATH                                               # another build of the library (-DKP_CLUST_HALVE=0)

kp_dist_count (max_diff 10, min_compared 1: the same all-pairs work with the cheapest epilogue) and kp_dist_clusters (the default
levels, nearest on) are timed alone on one handle, each by a host clock around a call that ends in a device synchronise; the median
of ``--repeats`` runs after one warm-up.  ``--dense`` is the worst case for the union-find's atomics and for the depth of its
chains: every pair is an edge at the last level, most of them from lower ones.  The labels are checked against what the population
must give.  DESIGN.md quotes the lines; nothing is gated on them."""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.distances_probe import CLUSTER, population  # noqa: E402


def dense_population(rows: int, blocks: int, seed: int = 1) -> np.ndarray:
    """``population`` with a single founder: every pair lies within ten differences."""
    rng = np.random.default_rng(seed)
    m = np.tile(rng.integers(0, 1 << 32, blocks, dtype=np.uint64), (rows, 1))
    for _ in range(5):
        r = np.flatnonzero(rng.random(rows) < 0.8)
        col = rng.integers(0, 16 * blocks, len(r))
        m[r, col // 16] ^= rng.integers(1, 4, len(r)).astype(np.uint64) << (2 * (col % 16)).astype(np.uint64)
    return m


def run_device(rows: int, blocks: int, repeats: int, dense: bool, lib: "str | None") -> dict:
    from kaptive_amd import _native

    if lib:
        _native.LIB_PATH = Path(lib).resolve()
    m = dense_population(rows, blocks) if dense else population(rows, blocks)
    levels = _native.CLUSTER_LEVELS
    ctx = _native.Context(0)
    t = {"count": [], "clusters": []}
    first = None
    try:
        with _native.Distances(ctx, m) as d:
            for rep in range(repeats + 1):  # the first is the warm-up
                t0 = time.perf_counter()
                n = d.count(levels[-1], 1)
                t1 = time.perf_counter()
                labels, near = d.clusters(levels, 1)
                t2 = time.perf_counter()
                if rep:
                    t["count"].append(t1 - t0); t["clusters"].append(t2 - t1)
                got = labels.tobytes() + near.tobytes()
                if first is None:
                    first = got
                elif got != first:
                    raise SystemExit("two runs gave different clusters")
    finally:
        ctx.close()
    n_clusters = 1 if dense else max(1, rows // CLUSTER)
    want = np.arange(rows) % n_clusters  # the last level joins every founder's rows: the label is the founder's first row
    if labels[-1].tolist() != want.tolist() or (near["row"] < 0).any() or (near["row"] % n_clusters != want).any():
        raise SystemExit("the clusters are not the population's")
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"rows": rows, "blocks": blocks, "columns": 16 * blocks, "pairs": rows * (rows - 1) // 2, "dense": dense, "levels": list(levels),
            "edges_at_last_level": int(n), "clusters_per_level": [int((labels[k] == np.arange(rows)).sum()) for k in range(len(levels))],
            "lib": str(lib) if lib else None, "repeats": repeats, "ms": {k: round(1e3 * v, 3) for k, v in med.items()},
            "ms_all": {k: [round(1e3 * x, 3) for x in v] for k, v in t.items()}, "clusters_over_count": round(med["clusters"] / med["count"], 3)}  # fmt: skip


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--blocks", type=int, default=1600)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    print(json.dumps(run_device(a.rows, a.blocks, a.repeats, a.dense, a.lib)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
