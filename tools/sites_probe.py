#!/usr/bin/env python3
"""What the variable sites cost on the device beside the count pass of the same handle (include/kp_spec.h, SITES;
kaptive_amd/csrc/kp_dist_sites.hip): R = 4096 synthetic locus rows of the largest locus of the ``kpsc_k`` synthetic database.

    python tools/sites_probe.py [--rows 4096] [--repeats 5]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/sites_probe.py      # the kernels' own times, in a run of its own

Every repeat makes a handle of its own -- the profile is computed once per handle -- and calls ``count`` (max_diff 10, min_compared
1), ``sites`` and ``site_rows`` on it, each timed by a host clock around a call that ends in a device synchronise; the first handle
is the warm-up.  The rows are clusters of 100 around a founder each, ten substitutions and an N or GAP run per row, as
tools/distances_probe.py draws them; the sites are checked against a count on the host.  DESIGN.md quotes the lines; nothing is gated
on them."""

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

from tools.distances_probe import population  # noqa: E402


def largest_locus_blocks() -> tuple[str, int, int]:
    from kaptive_amd.synth import make_db

    db = make_db("kpsc_k")
    blocks = (np.asarray(db.genes.lengths, np.int64) + 15) // 16
    off, n = np.asarray(db.locus_gene_offsets, np.int64), np.asarray(db.locus_gene_lengths, np.int64)
    per = np.array([int(blocks[o : o + k].sum()) for o, k in zip(off, n)])
    L = int(per.argmax())
    return db.loci.ids[L], int(per[L]), int(np.asarray(db.genes.lengths, np.int64)[off[L] : off[L] + n[L]].sum())


def host_counts(m: np.ndarray) -> np.ndarray:
    """int64 [16 NB, 4]: the rows of ``m`` that hold a, c, g, t at every column, counted 256 rows at a time."""
    j = np.arange(16, dtype=np.uint64)
    n = np.zeros((16 * m.shape[1], 4), np.int64)
    for r0 in range(0, m.shape[0], 256):
        v = m[r0 : r0 + 256, :, None]
        code = ((v >> (2 * j)) & np.uint64(3)).astype(np.uint8)
        held = (((v >> (j + np.uint64(32))) | (v >> (j + np.uint64(48)))) & np.uint64(1)) == 0
        for k in range(4):
            n[:, k] += ((code == k) & held).sum(axis=0).ravel()
    return n


def run_device(rows: int, repeats: int) -> dict:
    from kaptive_amd import _native

    locus, blocks, columns = largest_locus_blocks()
    m = population(rows, blocks)
    ctx = _native.Context(0)
    t = {"count": [], "sites": [], "site_rows": []}
    try:
        for rep in range(repeats + 1):  # the first is the warm-up
            with _native.Distances(ctx, m) as d:
                t0 = time.perf_counter()
                n_pairs = d.count(10, 1)
                t1 = time.perf_counter()
                s = d.sites()
                t2 = time.perf_counter()
                r = d.site_rows()
                t3 = time.perf_counter()
                if rep:
                    t["count"].append(t1 - t0); t["sites"].append(t2 - t1); t["site_rows"].append(t3 - t2)
    finally:
        ctx.close()
    n = host_counts(m)
    want = np.flatnonzero((n > 0).sum(axis=1) >= 2)
    if s["column"].tolist() != want.tolist() or (s["n"] != n[want]).any() or r.shape != (rows, (len(s) + 15) // 16):
        raise SystemExit("the sites are not the population's")
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"locus": locus, "rows": rows, "blocks": blocks, "columns": columns, "pairs_listed": int(n_pairs), "sites": int(len(s)), "repeats": repeats,
            "ms": {k: round(1e3 * v, 3) for k, v in med.items()}, "ms_all": {k: [round(1e3 * x, 3) for x in v] for k, v in t.items()}}  # fmt: skip


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps(run_device(a.rows, a.repeats)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
