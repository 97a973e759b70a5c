#!/usr/bin/env python3
"""What the neighbour-joining tree costs on the device and on the host (include/kp_spec.h, NJ; kaptive_amd/csrc/kp_dist_nj.hip,
kp_nj.h), on the population of tools/distances_probe.py: synthetic locus rows of NB = 1 600 blocks (25 600 columns) without N or
GAP, so every row is a taxon.

    python tools/nj_probe.py --device [--taxa 1024 4096] [--blocks 1600]      # kp_dist_nj: one cold and one warm call per size
    python tools/nj_probe.py --host   [--taxa 1024 4096] [--blocks 1600]      # kp_nj_matrix_host + kp_nj_host under g++ -O2, one thread

Each call is timed by a host clock; a device call ends in a synchronise.  Either mode prints one JSON line per size with the
SHA-256 of the taxa and the records: the two modes must print the same digest.  A kernel trace of the device mode gives the share
of the pick kernel.  DESIGN.md quotes the lines; nothing is gated on them."""

from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.distances_probe import population  # noqa: E402


def _digest(taxa, nodes) -> str:
    return hashlib.sha256(np.ascontiguousarray(taxa).tobytes() + np.ascontiguousarray(nodes).tobytes()).hexdigest()[:16]


def run_device(n: int, blocks: int) -> dict:
    from kaptive_amd import _native

    m = population(n, blocks)
    ctx = _native.Context(0)
    try:
        with _native.Distances(ctx, m) as d:
            ms = []
            for _ in range(2):  # cold, warm
                t0 = time.perf_counter()
                taxa, nodes = d.nj(1)
                ms.append(round(1e3 * (time.perf_counter() - t0), 3))
            t0 = time.perf_counter()
            d.count(10, 1)
            count_ms = round(1e3 * (time.perf_counter() - t0), 3)
    finally:
        ctx.close()
    joins = max(len(taxa) - 3, 0)
    return {"mode": "device", "taxa": int(len(taxa)), "blocks": blocks, "records": int(len(nodes)), "joins": joins, "launches_of_the_joins": 4 * joins,
            "cold_ms": ms[0], "warm_ms": ms[1], "count_pass_ms": count_ms, "total_length": float(nodes["la"].sum() + nodes["lb"].sum() + nodes["lc"].sum()),
            "digest": _digest(taxa, nodes)}  # fmt: skip


def run_host(n: int, blocks: int) -> dict:
    from tests import nj_util as NJ

    m = np.ascontiguousarray(population(n, blocks), np.uint64)
    h = NJ.harness()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    taxa = np.zeros(n, np.int32)
    t0 = time.perf_counter()
    k = h.kpy_nj_matrix_host(p(m), C.c_int32(n), C.c_int64(blocks), C.c_int32(1), p(taxa), None)
    dist = np.zeros((k, k), np.float64)
    h.kpy_nj_matrix_host(p(m), C.c_int32(n), C.c_int64(blocks), C.c_int32(1), p(taxa), p(dist))
    t1 = time.perf_counter()
    nodes = np.zeros(max(k - 2, 1), NJ.NODE_DTYPE)
    made = h.kpy_nj_host(p(dist), C.c_int32(k), p(nodes))
    t2 = time.perf_counter()
    return {"mode": "host", "taxa": int(k), "blocks": blocks, "records": int(made), "matrix_ms": round(1e3 * (t1 - t0), 1), "tree_ms": round(1e3 * (t2 - t1), 1),
            "digest": _digest(taxa[:k], nodes[:made])}  # fmt: skip


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--taxa", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--blocks", type=int, default=1600)
    a = ap.parse_args()
    if a.device == a.host:
        ap.error("one of --device and --host")
    for n in a.taxa:
        print(json.dumps((run_device if a.device else run_host)(n, a.blocks)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
