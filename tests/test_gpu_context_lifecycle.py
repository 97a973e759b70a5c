"""A context gives back what it owns when it is closed, cycle after cycle, and the process ends cleanly (run with -m gpu).

The context, its work sets, typing runs and batch inputs own their device buffers, streams, events and page-locked blocks
through their members: closing a context frees them in member order, and nothing of them is left for process teardown.
The cycles run in a process of their own, because its exit status is part of what is checked."""

import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu


def _cycles():
    """Three times: create a context, load the 9-locus database, align and type one batch of two 90 kb assemblies, close."""
    from kaptive_amd import _native
    from kaptive_amd.engine import Engine
    from kaptive_amd.serotyping.core import Serotyper
    from kaptive_amd.synth import make_assembly, make_db

    db = make_db("kpsc_k", seed=7, n_loci=9)
    asms = [make_assembly(db, seed=s, length=90_000, median_contigs=5, min_contig=200) for s in (11, 13)]
    packed, ids, typer = [a.packed() for a in asms], [a.id for a in asms], Serotyper(db)
    pinned_before = _native.pinned_bytes()
    results = []
    for cycle in range(3):
        eng = Engine(db)
        batch = eng.ctx.batch(packed)
        typed = eng.type_batch(typer, batch, ids)
        results.append((typed.rows(), typed.sums.tobytes()))
        batch.close()
        eng.close()
        assert _native.pinned_bytes() == pinned_before, (cycle, _native.pinned_bytes(), pinned_before)
    assert results[0][0]
    assert results[1] == results[0] and results[2] == results[0]
    print("three cycles equal")


def test_three_context_cycles_in_one_process():
    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_context_lifecycle import _cycles; _cycles()"], cwd=root,
                       capture_output=True, text=True, timeout=300)  # fmt: skip
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("three cycles equal")
