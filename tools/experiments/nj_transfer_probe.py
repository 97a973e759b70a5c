#!/usr/bin/env python3
"""What the transfer bootstrap of the neighbour-joining tree costs on the device (include/kp_spec.h, TRANSFER;
kaptive_amd/csrc/kp_dist_transfer.hip), on the population of tools/distances_probe.py: synthetic locus rows without N or GAP, so every
row is a taxon.

    python tools/experiments/nj_transfer_probe.py [--taxa 1024] [--blocks 1600] [--replicates 100] [--repeats 5] [--parent-lib FILE]
    python tools/experiments/nj_transfer_probe.py --taxa 8192 --replicates 1                   # the longest walk, the fewest lanes
    python tools/experiments/nj_transfer_probe.py --once --taxa 1024                           # one warm call of each kind, for a kernel trace

Per size, after one warm-up of each, `repeats` timed rounds that alternate -- every round starts one kind later than the one before --
  (p) kp_dist_nj_bootstrap of the library built from the parent commit (`--parent-lib`: its libkaptive_amd.so; left out without it),
  (a) kp_dist_nj_bootstrap of this tree's library, and
  (b) kp_dist_nj_transfer of this tree's library,
all with the same rows, seed and replicates.  Each call is timed by a host clock and ends in a synchronise.  One JSON line per size:
the medians, every run, the spread of the parent's runs -- the margin within which (a) must stay --, and the cost of the transfer pass
as a share of the bootstrap's time, (b - a) / a.  The kernels' own times: run `--once` under `rocprofv3 --kernel-trace --stats`.
DESIGN.md quotes the lines; nothing is gated on them."""

from __future__ import annotations

import argparse
import importlib.util
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from tools.distances_probe import population  # noqa: E402


def _binding_of(lib_path: Path):
    """A second copy of the binding module around another build of the library: its own globals, its own handle."""
    spec = importlib.util.spec_from_file_location("kaptive_amd_native_of_parent", ROOT / "kaptive_amd" / "_native.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    mod.LIB_PATH = lib_path
    return mod


def _timed(call) -> float:
    t0 = time.perf_counter()
    call()
    return 1e3 * (time.perf_counter() - t0)


def run(n: int, blocks: int, replicates: int, repeats: int, once: bool, parent_lib: "Path | None") -> dict:
    from kaptive_amd import _native

    m = population(n, blocks)
    ctx = _native.Context(0)
    old = _binding_of(parent_lib) if parent_lib else None
    old_ctx = old.Context(0) if old else None
    try:
        with _native.Distances(ctx, m) as d:
            taxa, nodes = d.nj(1)
            counted = d.nj_support(1, nodes, replicates)  # (warm-up of every call)
            support, transfer = d.nj_transfer(1, nodes, replicates)
            assert support.tobytes() == counted.tobytes()
            od = old.Distances(old_ctx, m) if old else None
            if od is not None:
                assert od.nj(1)[1].tobytes() == nodes.tobytes() and od.nj_support(1, nodes, replicates).tobytes() == counted.tobytes()
            p_ms, a_ms, b_ms = [], [], []
            kinds = [(a_ms, lambda: d.nj_support(1, nodes, replicates)), (b_ms, lambda: d.nj_transfer(1, nodes, replicates))]
            if od is not None:
                kinds.insert(0, (p_ms, lambda: od.nj_support(1, nodes, replicates)))
            for k in range(1 if once else repeats):
                for into, call in kinds[k % len(kinds) :] + kinds[: k % len(kinds)]:  # (a round starts one kind later than the one before: no kind is always first)
                    into.append(_timed(call))
            if od is not None:
                od.close()
    finally:
        if old_ctx is not None:
            old_ctx.close()
        ctx.close()
    k = len(taxa)
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    deep = transfer[: max(k - 3, 0)]
    out = {"taxa": int(k), "blocks": blocks, "replicates": replicates, "bootstrap_ms_median": round(a, 2), "bootstrap_ms": [round(x, 2) for x in a_ms],
           "transfer_ms_median": round(b, 2), "transfer_ms": [round(x, 2) for x in b_ms], "transfer_pass_share_of_bootstrap": round((b - a) / a, 4),
           "support_full": int((support[: max(k - 3, 0)] == replicates).sum()), "transfer_zero": int((deep == 0).sum()), "transfer_mean": round(float(deep.mean()), 2) if len(deep) else None}  # fmt: skip
    if p_ms:
        out.update({"parent_bootstrap_ms_median": round(statistics.median(p_ms), 2), "parent_bootstrap_ms": [round(x, 2) for x in p_ms],
                    "parent_spread_ms": round(max(p_ms) - min(p_ms), 2), "bootstrap_minus_parent_ms": round(a - statistics.median(p_ms), 2)})  # fmt: skip
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--taxa", type=int, nargs="+", default=[1024])
    ap.add_argument("--blocks", type=int, default=1600)
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", type=Path, default=None, help="libkaptive_amd.so built from the parent commit: the yardstick of the existing call")
    ap.add_argument("--once", action="store_true", help="one warm call of each kind per size: the run to trace")
    a = ap.parse_args()
    for n in a.taxa:
        print(json.dumps(run(n, a.blocks, a.replicates, a.repeats, a.once, a.parent_lib)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
