#!/usr/bin/env python3
"""What the pairwise locus distances cost on the device (include/kp_spec.h, DISTANCES; kaptive_amd/csrc/kp_dist.hip), at the
benchmark's own shape: R = 10 000 synthetic locus rows of NB = 1 600 blocks (25 600 columns), 5e7 pairs.

    python tools/distances_probe.py [--rows 10000] [--blocks 1600] [--repeats 5]   # on the device: one JSON line
    python tools/distances_probe.py --cpu [--rows 500]                              # the numpy restatement on the host, for context

The population: clusters of 100 rows around a founder each, every row up to five substitutions away from its founder -- so that with
max_diff = 10 the pairs inside a cluster qualify, about 1 % of all pairs.  kp_dist_create (upload and planes), kp_dist_count (the
pair kernel's count pass and the scan) and kp_dist_pairs (its fill pass and the read-back) are timed alone, each by a host clock
around a call that ends in a device synchronise; the median of ``--repeats`` runs after one warm-up.  column_pairs_per_s is
pairs x columns over the time of kp_dist_count.  DESIGN.md quotes the line; nothing is gated on it."""

from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CLUSTER = 100


def population(rows: int, blocks: int, seed: int = 1) -> np.ndarray:
    """uint64 [rows, blocks]: locus rows without N or GAP; row r belongs to cluster r % n_clusters."""
    rng = np.random.default_rng(seed)
    n_clusters = max(1, rows // CLUSTER)
    founders = rng.integers(0, 1 << 32, (n_clusters, blocks), dtype=np.uint64)  # sixteen random 2-bit codes a block, no mask bit
    m = founders[np.arange(rows) % n_clusters].copy()
    for _ in range(5):  # up to five substitutions a row: a code XOR 1..3 is another code
        hit = rng.random(rows) < 0.8
        r = np.flatnonzero(hit)
        col = rng.integers(0, 16 * blocks, len(r))
        m[r, col // 16] ^= rng.integers(1, 4, len(r)).astype(np.uint64) << (2 * (col % 16)).astype(np.uint64)
    return m


def run_device(rows: int, blocks: int, repeats: int, max_diff: int) -> dict:
    from kaptive_amd import _native

    m = population(rows, blocks)
    ctx = _native.Context(0)
    t = {"create": [], "count": [], "pairs": []}
    n_pairs = first = None
    try:
        for rep in range(repeats + 1):  # the first is the warm-up
            t0 = time.perf_counter()
            d = _native.Distances(ctx, m)
            t1 = time.perf_counter()
            n = d.count(max_diff, 1)
            t2 = time.perf_counter()
            out = np.zeros(n, _native.DIST_PAIR_DTYPE)
            t3 = time.perf_counter()
            ctx._check(_native.lib().kp_dist_pairs(ctx._h, d._h, out.ctypes.data_as(C.c_void_p), C.c_int64(len(out))), "kp_dist_pairs")
            t4 = time.perf_counter()
            d.close()
            if rep:
                t["create"].append(t1 - t0); t["count"].append(t2 - t1); t["pairs"].append(t4 - t3)
            if first is None:
                n_pairs, first = n, out.tobytes()
            elif out.tobytes() != first:
                raise SystemExit("two runs listed different pairs")
        same = (out["a"] % max(1, rows // CLUSTER)) == (out["b"] % max(1, rows // CLUSTER))
    finally:
        ctx.close()
    med = {k: statistics.median(v) for k, v in t.items()}
    all_pairs = rows * (rows - 1) // 2
    return {"rows": rows, "blocks": blocks, "columns": 16 * blocks, "pairs": all_pairs, "listed": int(n_pairs), "listed_share": n_pairs / max(all_pairs, 1),
            "listed_inside_a_cluster": int(same.sum()), "max_diff": max_diff, "repeats": repeats,
            "ms": {k: round(1e3 * v, 3) for k, v in med.items()}, "ms_all": {k: [round(1e3 * x, 3) for x in v] for k, v in t.items()},
            "column_pairs_per_s": all_pairs * 16 * blocks / med["count"]}  # fmt: skip


def run_cpu(rows: int, blocks: int, max_diff: int) -> dict:
    from tests import distances_util as D

    codes = D.unpack(population(rows, blocks))
    t0 = time.perf_counter()
    got = D.all_pairs(codes, max_diff, 1)
    dt = time.perf_counter() - t0
    all_pairs = rows * (rows - 1) // 2
    return {"cpu_restatement": True, "rows": rows, "blocks": blocks, "pairs": all_pairs, "listed": len(got), "ms": round(1e3 * dt, 1),
            "column_pairs_per_s": all_pairs * 16 * blocks / dt}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--blocks", type=int, default=1600)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-diff", type=int, default=10)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    if a.cpu:
        print(json.dumps(run_cpu(a.rows or 500, a.blocks, a.max_diff)))
    else:
        print(json.dumps(run_device(a.rows or 10000, a.blocks, a.repeats, a.max_diff)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
