#!/usr/bin/env python3
"""What the minimum spanning forest costs on the device beside the count pass of the same matrix (include/kp_spec.h, TREE;
kaptive_amd/csrc/kp_dist_graph.hip), at the shape of tools/distances_probe.py: R = 10 000 synthetic locus rows of NB = 1 600 blocks
(25 600 columns), 5e7 pairs.

    python tools/tree_probe.py [--rows 10000] [--blocks 1600] [--repeats 5]           # clusters of 100 rows around a founder each
    python tools/tree_probe.py --dense                                                  # every row drawn from one founder
    python tools/tree_probe.py --lib PATH                                               # another build of the library (-DKP_TREE_SKIP=0)

kp_dist_count (max_diff 10, min_compared 1: the same all-pairs work with the cheapest epilogue) and kp_dist_tree (min_compared 1) are
timed alone on one handle, each by a host clock around a call that ends in a device synchronise; the median of ``--repeats`` runs
after one warm-up.  The expectation to hold the tree against is rounds x the count pass: every round of Boruvka visits every tile
once.  The forest is checked against what the population must give.  DESIGN.md quotes the lines; nothing is gated on them."""

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

from tools.clusters_probe import dense_population  # noqa: E402
from tools.distances_probe import CLUSTER, population  # noqa: E402


def run_device(rows: int, blocks: int, repeats: int, dense: bool, lib: "str | None") -> dict:
    from kaptive_amd import _native

    if lib:
        _native.LIB_PATH = Path(lib).resolve()
    m = dense_population(rows, blocks) if dense else population(rows, blocks)
    ctx = _native.Context(0)
    t = {"count": [], "tree": []}
    first = None
    try:
        with _native.Distances(ctx, m) as d:
            for rep in range(repeats + 1):  # the first is the warm-up
                t0 = time.perf_counter()
                d.count(10, 1)
                t1 = time.perf_counter()
                edges, comp = d.tree(1)
                t2 = time.perf_counter()
                if rep:
                    t["count"].append(t1 - t0); t["tree"].append(t2 - t1)
                got = edges.tobytes() + comp.tobytes()
                if first is None:
                    first = got
                elif got != first:
                    raise SystemExit("two runs gave different forests")
            rounds = d.tree_rounds()
    finally:
        ctx.close()
    # one tree; inside a founder's rows (r % n_clusters) the edges are at most ten differences, between founders far more
    n_clusters = 1 if dense else max(1, rows // CLUSTER)
    near = edges["differences"] <= 10
    key = list(zip(edges["differences"].tolist(), edges["a"].tolist(), edges["b"].tolist()))
    if (len(edges) != rows - 1 or comp.any() or int(near.sum()) != rows - n_clusters or (edges["a"][near] % n_clusters != edges["b"][near] % n_clusters).any()
            or key != sorted(key)):  # fmt: skip
        raise SystemExit("the forest is not the population's")
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"rows": rows, "blocks": blocks, "columns": 16 * blocks, "pairs": rows * (rows - 1) // 2, "dense": dense, "edges": int(len(edges)),
            "edges_within_10": int(near.sum()), "heaviest_edge": int(edges["differences"].max()), "rounds": rounds,
            "lib": str(lib) if lib else None, "repeats": repeats, "ms": {k: round(1e3 * v, 3) for k, v in med.items()},
            "ms_all": {k: [round(1e3 * x, 3) for x in v] for k, v in t.items()}, "tree_over_count": round(med["tree"] / med["count"], 3),
            "tree_over_rounds_x_count": round(med["tree"] / (rounds * med["count"]), 3)}  # fmt: skip


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
