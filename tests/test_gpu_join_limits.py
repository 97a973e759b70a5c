"""The device on both sides of every limit of the join path (kp-align v5, include/kp_spec.h), against the CPU oracle, with
the assemblies of tests/join_limits_util.py (tests/test_join_limits_oracle.py pins which side of its limit the oracle lands
on): anchors, band tasks, join records and hits alone in a small batch, the same inside full-size assemblies of the 163-locus
K database, and the typed rows of the device's reduction against the host reduction of the oracle's hits."""

import os

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.core.genome import GenomeAssembly
from kaptive_amd.core.seq import SeqRecord, Sequences
from kaptive_amd.pack import PackedAssembly, pack_sequences_flat
from tests import join_limits_util as J
from tests.test_gpu_parity import _oracle_typer, _rows_of, _same_records
from tests.test_join_limits_oracle import EXPECT

pytestmark = pytest.mark.gpu

_TASK_ORDER = list(_native.TASK_DTYPE.names)


def _sorted_joins(j):
    return j[np.lexsort((j["lo"][:, 0], j["contig"], j["gs"]))] if len(j) else j


def _compare(label, got_anchors, got_tasks, got_joins, got_hits, want):
    """Device stages of one assembly against the oracle's (anchors, tasks, joins, hits); returns the oracle's joins."""
    anchors, tasks, joins, hits = want
    assert np.array_equal(got_anchors, anchors), f"{label}: anchors differ ({len(got_anchors)} vs {len(anchors)})"
    _same_records(np.sort(got_tasks, order=_TASK_ORDER), np.sort(tasks, order=_TASK_ORDER), f"{label}: tasks")
    want_j, got_j = _sorted_joins(joins), _sorted_joins(got_joins)
    assert len(got_j) == len(want_j), f"{label}: {len(got_j)} join records, the oracle has {len(want_j)}"
    for f in want_j.dtype.names:
        assert np.array_equal(got_j[f], want_j[f]), f"{label}: join field {f}: {got_j[f][:2]} vs {want_j[f][:2]}"
    _same_records(got_hits, hits, f"{label}: hits")
    return joins


def _align_and_compare(genes, labels, packed, want):
    codes, off = pack_sequences_flat(genes)
    ctx = _native.Context(0)
    ctx.load_genes(codes, off)
    batch = ctx.batch(packed)
    hits, hoff = batch.align()
    n_joined = 0
    for i, label in enumerate(labels):
        joins = _compare(label, batch.anchors(i), batch.tasks(i), batch.joins(i), hits[hoff[i] : hoff[i + 1]], want[i])
        n_joined += int((joins["piece"][:, :, 0] == 1).any(axis=1).sum())
    batch.close()
    ctx.close()
    return n_joined


# ---- the oracle in spawned workers (a process that holds a HIP context does not survive a fork) ----------------------------------
_ODB = None


def _oracle_init(codes, off):
    global _ODB
    from oracle import oracle as O

    _ODB = O.OracleDB(codes, off)


def _oracle_stages(fields):
    pa = PackedAssembly(*fields)
    return _ODB.anchors(pa), _ODB.tasks(pa), _ODB.joins(pa), _ODB.align(pa)


def _fields(pa):
    return (pa.words, pa.padded_len, pa.ctg_start, pa.ctg_len, pa.n_runs)


def test_join_limits_match_oracle(oracle):
    """All sides of all cases in one batch: anchors, sorted band tasks, every field of the join records, hits."""
    sides = J.join_limit_cases()
    genes = J.database().genes
    odb = oracle.OracleDB(*pack_sequences_flat(genes))
    packed = [s.asm.packed() for s in sides]
    want = [(odb.anchors(pa), odb.tasks(pa), odb.joins(pa), odb.align(pa)) for pa in packed]
    assert _align_and_compare(genes, [s.label for s in sides], packed, want) >= 20  # (the comparison was not vacuous)


def test_join_limits_inside_full_size_assemblies(oracle):
    """Every side again, its contigs appended to a full-size assembly of the 163-locus K database whose genes the limit's genes
    sit among: the gene/strand's anchors lie inside a long sorted list that kp_chain_kernel cuts into slices and hands on
    from one wave to the next."""
    import multiprocessing as mp

    from kaptive_amd.synth import make_assembly, make_db

    db_k = make_db("kpsc_k", seed=100)
    half = len(db_k.genes) // 2
    ours = J.database().genes
    k_recs = [SeqRecord(f"k{i}", db_k.genes[i].seq) for i in range(len(db_k.genes))]
    genes = Sequences.from_records(k_recs[:half] + [SeqRecord(f"j{i}", ours[i].seq) for i in range(len(ours))] + k_recs[half:])
    base = make_assembly(db_k, seed=9300)
    base_recs = [SeqRecord(f"b{i}", base.contigs[i].seq) for i in range(len(base.contigs))]
    sides = J.join_limit_cases()
    asms = [GenomeAssembly(s.label, Sequences.from_records(base_recs + [SeqRecord(f"x{i}", s.asm.contigs[i].seq) for i in range(len(s.asm.contigs))]))
            for s in sides]  # fmt: skip
    packed = [a.packed() for a in asms]
    codes, off = pack_sequences_flat(genes)
    with mp.get_context("spawn").Pool(min(16, max(2, (os.cpu_count() or 2) // 2)), _oracle_init, (codes, off)) as pool:
        want = pool.map(_oracle_stages, [_fields(pa) for pa in packed], chunksize=1)
    for s, w in zip(sides, want):  # the limit's gene is on the same side as alone (its index moved up by `half`)
        joins = w[2][w[2]["gs"] // 2 == half + s.gene]
        pieces = sorted(int(j["n_pieces"]) for j in joins if (j["piece"][:, 0] == 1).any())
        assert pieces == EXPECT[s.label][0], f"{s.label}: joins of {pieces} pieces inside the full-size assembly"
    assert _align_and_compare(genes, [f"{s.label}, inside a full-size assembly" for s in sides], packed, want) >= 20


def test_join_limits_typed_rows(oracle):
    """Cases a-e as typed rows against a database whose loci hold the genes: the device's reduction of the device's hits
    equals the host reduction of the oracle's hits, joined or not."""
    from kaptive_amd.engine import Engine
    from kaptive_amd.serotyping.core import Serotyper

    db = J.database()
    sides = [s for s in J.join_limit_cases() if s.gene != J.F]
    genomes = [s.asm for s in sides]
    _, cpu = _oracle_typer(db, oracle)
    want = _rows_of([cpu(g) for g in genomes])
    eng = Engine(db)
    typer = Serotyper(db)
    typer._engine = eng
    batch = eng.ctx.batch([g.packed() for g in genomes])
    batch.align()
    got = eng.type_batch(typer, batch, [g.id for g in genomes], aligned=True).rows()
    for s, g_row, w_row in zip(sides, got, want):
        assert g_row == w_row, f"{s.label}: typed row\n{g_row}\nvs\n{w_row}"
    assert len(set(want)) > 1
    batch.close()
    eng.close()
