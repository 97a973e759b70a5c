#!/usr/bin/env python3
"""What small parsimony on the neighbour-joining tree costs on the device beside the tree itself (include/kp_spec.h, PARSIMONY;
kaptive_amd/csrc/kp_dist_pars.hip), on the population of tools/distances_probe.py: synthetic locus rows without N or GAP, so every
row is a taxon -- and, its founders being random, nearly every column a site with a change for every cluster: the longest lists.

    python tools/experiments/nj_parsimony_probe.py [--taxa 1024 8192] [--blocks 1600] [--repeats 3]
    python tools/experiments/nj_parsimony_probe.py --once --taxa 1024                          # one warm call of each kind, for a kernel trace

Per size, on one handle, after one warm-up of each: `repeats` timed rounds of
  (a) kp_dist_nj -- the tree,
  (b) kp_dist_nj_parsimony on its records -- both passes, the counts, the scans and the fills --, and
  (c) kp_dist_pars_sites and kp_dist_pars_changes -- the copies of the records to the host.
Each call is timed by a host clock and ends in a synchronise.  One JSON line per size: the medians, every run, the numbers of sites
and changes, and the pass as a share of the tree's time, b / a.  The kernels' own times: run `--once` under `rocprofv3 --kernel-trace
--stats`.  DESIGN.md quotes the lines; nothing is gated on them."""

from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from tools.distances_probe import population  # noqa: E402


def _timed(call) -> float:
    t0 = time.perf_counter()
    call()
    return 1e3 * (time.perf_counter() - t0)


def run(n: int, blocks: int, repeats: int, once: bool) -> dict:
    from kaptive_amd import _native

    m = population(n, blocks)
    ctx = _native.Context(0)
    lib = _native.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        with _native.Distances(ctx, m) as d:
            taxa, nodes = d.nj(1)  # (warm-up of every call)
            sites, changes = d.nj_parsimony(1, nodes)
            ns, nc = C.c_int64(0), C.c_int64(0)

            def passes():
                ctx._check(lib.kp_dist_nj_parsimony(ctx._h, d._h, C.c_int32(1), p(nodes), C.c_int64(len(nodes)), C.byref(ns), C.byref(nc)), "kp_dist_nj_parsimony")

            def fetch():
                ctx._check(lib.kp_dist_pars_sites(ctx._h, d._h, p(sites), C.c_int64(len(sites))), "kp_dist_pars_sites")
                ctx._check(lib.kp_dist_pars_changes(ctx._h, d._h, p(changes), C.c_int64(len(changes))), "kp_dist_pars_changes")

            a_ms, b_ms, c_ms = [], [], []
            for _ in range(1 if once else repeats):
                a_ms.append(_timed(lambda: d.nj(1)))
                b_ms.append(_timed(passes))
                c_ms.append(_timed(fetch))
            assert ns.value == len(sites) and nc.value == len(changes) and int(sites["steps"].sum()) == len(changes)
    finally:
        ctx.close()
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    held = np.array([bin(int(x)).count("1") for x in sites["alleles"][:100000]])
    return {"taxa": int(len(taxa)), "blocks": blocks, "plane_words": (blocks + 3) // 4, "nj_ms_median": round(a, 2), "nj_ms": [round(x, 2) for x in a_ms],
            "parsimony_ms_median": round(b, 2), "parsimony_ms": [round(x, 2) for x in b_ms], "fetch_ms_median": round(statistics.median(c_ms), 2),
            "parsimony_share_of_nj": round(b / a, 4), "sites": int(len(sites)), "changes": int(len(changes)),
            "homoplasic_of_first_100000_sites": int((sites["steps"][:100000] > held - 1).sum())}  # fmt: skip


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--taxa", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--blocks", type=int, default=1600)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="one warm call of each kind per size: the run to trace")
    a = ap.parse_args()
    for n in a.taxa:
        print(json.dumps(run(n, a.blocks, a.repeats, a.once)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
