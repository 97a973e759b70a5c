"""The device against the CPU oracle at the batch sizes the benchmark runs at and at the limits the library states for a
batch, with the compositions of tests/large_batch_util.py (tests/test_large_batch_oracle.py pins where they land):

a. the benchmark's shape: 1026 full-size assemblies, 5.2 Gbp, K and O on one device copy of the words; bases 2^31 and
   2^32 of the batch lie inside a hit (the second inside a joined one), so candidate positions use bits 31 and 32, the DP
   trace passes 4 GB and the per-assembly strides are multiplied by indices beyond 1000 -- once as it comes, once with
   hit_cap and tasks_per_asm started small, so that a grow-and-rerun happens at this size, once (report rows) through one
   pass over the genes of both databases, as bench.py runs it;
b. the same for 1100 assemblies of about 1500 contigs each: 1.7 M contigs in the batch's tables;
c. a batch of 2^33 - 64 bases, the most a batch may hold, with real sources at its highest positions;
d. the same batch 64 bases longer: refused with KP_EOVERFLOW before anything is launched, and the context works on;
e. per-assembly buffers the library could not index: anchor_cap * n_asm of 2^32 entries and prot_cap * n_asm of 2^31
   bytes are refused, and 63 * 2^25 bytes of protein buffer -- the largest int32 offset that path forms -- give the host
   reduction's rows.

Every comparison covers every entry of its batch: hit tables field for field, report rows byte for byte.  Three limits
are out of scope, because they cannot be reached without doing that much real work: 64 GB of DP trace, 2^24 hits in one
assembly and 65 536 occurrence tables.  Each refusal tested here is a checked return at the head of enqueue_align /
enqueue_reduce (kp_align.hip, kp_typing.hip), before the first reservation and the first launch of the pass."""

import json

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.pack import pack_sequences_flat
from kaptive_amd.serotyping.core import Serotyper
from kaptive_amd.synth import make_assembly, make_db
from tests import large_batch_util as L
from tests.test_gpu_parity import _oracle_typer, _rows_of, _same_records

pytestmark = pytest.mark.gpu


def _same_hits(what, keys, its, k, hits, off) -> int:
    """Hit table of every entry against its source's oracle table of database k; the label of a difference names the entry,
    its source and the batch-wide base it starts at.  Returns the number of records compared."""
    word_off = L.word_offsets(keys, its)
    for i, key in enumerate(keys):
        _same_records(hits[off[i] : off[i + 1]], its[key].hits[k], f"{what}, database {k}, entry {i} = {key} from base {16 * int(word_off[i])}")
    assert int(off[-1]) == sum(len(its[key].hits[k]) for key in keys)
    return int(off[-1])


def _same_rows(what, keys, its, k, engine, db, batch) -> None:
    typer = Serotyper(db)
    typer._engine = engine
    rows = engine.type_batch(typer, batch, [its[key].id for key in keys], aligned=True).rows()
    assert len(rows) == len(keys)
    for i, (key, row) in enumerate(zip(keys, rows)):
        assert row == its[key].rows[k], f"{what}, database {k}, row of entry {i} = {key}\n{row}\nvs\n{its[key].rows[k]}"


def _k_and_o(what, keys, its, rows: bool) -> dict:
    """One pass for K, one for O on the adopted device words (as the sweep and the benchmark do): every entry's hits, and
    with `rows` every entry's report row, equal the oracle's.  Returns the K pass's stats()."""
    from kaptive_amd.engine import Engine

    dbs = L.databases("kpsc")
    packed = [its[key].packed for key in keys]
    engines = [Engine(db) for db in dbs]
    first = engines[0].ctx.batch(packed)
    assert first.total_words * 16 == L.total_bases(keys, its)
    batches = [first, engines[1].ctx.batch(packed, device_words=first.device_words, after=first)]
    for b in batches:
        b.align_async()
    compared = 0
    for k, (db, e, b) in enumerate(zip(dbs, engines, batches)):
        b.wait()
        compared += _same_hits(what, keys, its, k, *b.hits())
        if rows:
            _same_rows(what, keys, its, k, e, db, b)
    stats = batches[0].stats()
    print(f"{what}: {len(keys)} entries, {first.total_words * 16} bases, {compared} hit records equal; stats of the K pass: {json.dumps(stats)}")
    for b in reversed(batches):
        b.close()
    for e in engines:
        e.close()
    return dict(stats, compared=compared)


# ---- a. the benchmark's shape ---------------------------------------------------------------------------------------------------
def test_benchmark_shape_k_and_o(oracle):
    from kaptive_amd.engine import Engine

    keys, its, _ = L.benchmark_shape_batch()
    assert len(keys) == 1026 and L.total_bases(keys, its) > 2**32
    first = _k_and_o("benchmark shape", keys, its, rows=True)
    assert first["compared"] > 1000 * len(keys), f"{first['compared']} hit records"
    assert first["hits"] == sum(len(its[key].hits[0]) for key in keys) and first["dp_cells"] > 0
    # ... and with the hit and task lists started far too small: the pass and the finalisation are repeated at this size
    db = L.databases("kpsc")[0]
    eng = Engine(db)
    eng.ctx.set_option("hit_cap", 512)
    eng.ctx.set_option("tasks_per_asm", 256)
    batch = eng.ctx.batch([its[key].packed for key in keys])
    assert batch.total_words * 16 > 2**32
    _same_hits("benchmark shape, grown buffers", keys, its, 0, *batch.align())
    stats = batch.stats()
    print(f"benchmark shape, hit_cap and tasks_per_asm started small: stats of the K pass: {json.dumps(stats)}")
    assert stats["retries"] >= 1
    assert (stats["anchors"], stats["tasks"], stats["hits"]) == (first["anchors"], first["tasks"], first["hits"])
    batch.close()
    eng.close()
    # ... and through one alignment pass over the genes of both databases, which is how bench.py types its batches of 1000
    dbs = L.databases("kpsc")
    both = Engine(list(dbs))
    batch = both.ctx.batch([its[key].packed for key in keys])
    batch.align_async()
    for k, db in enumerate(dbs):
        _same_rows("benchmark shape, shared pass", keys, its, k, both.view(k), db, batch)
    assert batch.stats()["hits"] == sum(len(h) for key in keys for h in its[key].hits)
    batch.close()
    both.close()


# ---- b. 1500 contigs per assembly ---------------------------------------------------------------------------------------------
def test_many_contigs_past_two_to_the_32(oracle):
    from kaptive_amd.engine import Engine

    keys, its = L.many_contigs_batch()
    db = L.databases("ab_k")[0]
    eng = Engine(db)
    batch = eng.ctx.batch([its[key].packed for key in keys])
    assert len(keys) == 1100 and batch.total_words * 16 > 2**32
    compared = _same_hits("1500 contigs", keys, its, 0, *batch.align())
    assert compared > 1000 * len(keys)
    _same_rows("1500 contigs", keys, its, 0, eng, db, batch)
    print(f"1500 contigs: {len(keys)} entries, {sum(len(its[key].packed.ctg_len) for key in keys)} contigs, {batch.total_words * 16} bases, "
          f"{compared} hit records equal; stats: {json.dumps(batch.stats())}")  # fmt: skip
    batch.close()
    eng.close()


# ---- c. just inside 2^33 bases -------------------------------------------------------------------------------------------------
def test_batch_of_two_to_the_33_minus_64_bases(oracle):
    keys, its, _ = L.inside_limit_batch()
    assert L.total_bases(keys, its) == 2**33 - 64
    got = _k_and_o("2^33 - 64 bases", keys, its, rows=False)
    assert got["compared"] > 1000 * 48  # (the 48 real sources; the fillers' counts: tests/test_large_batch_oracle.py)


# ---- d. just outside ------------------------------------------------------------------------------------------------------------
def test_batch_of_two_to_the_33_bases_is_refused_cleanly(oracle):
    keys, its, last = L.inside_limit_batch()
    packed = [its[key].packed for key in keys[:-1]] + [L.packed_of((*last[:2], last[2] + 64, last[3]))]
    db = L.databases("kpsc")[0]
    ctx = _native.Context(0)
    ctx.load_genes(*pack_sequences_flat(db.genes))
    batch = ctx.batch(packed)
    assert batch.total_words * 16 == 2**33
    with pytest.raises(_native.NativeError, match=r"at most 2\^33 bases"):
        batch.align_async()
    with pytest.raises(_native.NativeError):  # nothing was enqueued, so there is nothing to wait for
        batch.wait()
    batch.close()
    del packed
    two = keys[-3:-1]  # the same context goes on: two real sources
    small = ctx.batch([its[key].packed for key in two])
    assert _same_hits("after the refusal", two, its, 0, *small.align()) > 1000
    small.close()
    ctx.close()


# ---- e. buffers that cannot be indexed -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    db = make_db("kpsc_k", seed=7, n_loci=9)
    genomes = [make_assembly(db, seed=640 + i, length=60_000, median_contigs=4, min_contig=200) for i in range(64)]
    return db, genomes


def test_anchor_buffer_of_two_to_the_32_entries_is_refused(oracle, small):
    db, genomes = small
    codes, off = pack_sequences_flat(db.genes)
    odb = oracle.OracleDB(codes, off)
    packed = [g.packed() for g in genomes]
    ctx = _native.Context(0)
    ctx.load_genes(codes, off)
    batch = ctx.batch(packed)
    try:
        ctx.set_option("anchor_cap", 1 << 26)  # x 64 assemblies = 2^32 entries: one past what a 32-bit index reaches
        before = _native.device_allocations()
        with pytest.raises(_native.NativeError, match=r"anchor buffer would exceed 2\^32 entries"):
            batch.align_async()
        assert _native.device_allocations() == before, "the refused pass reserved device memory"
    finally:
        ctx.set_option("anchor_cap", 1 << 17)  # (the library's default)
    hits, hoff = batch.align()
    for i, pa in enumerate(packed):
        _same_records(hits[hoff[i] : hoff[i + 1]], odb.align(pa), f"hits of assembly {i} after the refusal")
    assert hoff[-1] > 10 * len(packed)
    batch.close()
    ctx.close()


def test_protein_buffer_of_two_to_the_31_bytes_is_refused_and_the_largest_below_works(oracle, small):
    from kaptive_amd.engine import Engine

    db, genomes = small
    _, cpu = _oracle_typer(db, oracle)
    eng = Engine(db)
    typer = Serotyper(db)
    typer._engine = eng
    try:
        eng.ctx.set_option("prot_cap", 1 << 25)  # x 64 assemblies = 2^31 bytes: one past the largest int32 offset
        batch = eng.ctx.batch([g.packed() for g in genomes])
        batch.align_async()
        with pytest.raises(_native.NativeError, match=r"protein buffer would exceed 2\^31 bytes"):
            eng.type_batch(typer, batch, [g.id for g in genomes], aligned=True)
        batch.close()
        batch = eng.ctx.batch([g.packed() for g in genomes[:63]])  # 63 x 2^25 = 2 113 929 216 bytes
        batch.align_async()
        got = eng.type_batch(typer, batch, [g.id for g in genomes[:63]], aligned=True).rows()
        want = _rows_of([cpu(g) for g in genomes[:63]])
        for i, (g_row, w_row) in enumerate(zip(got, want)):
            assert g_row == w_row, f"row of assembly {i} with a protein buffer of 63 x 2^25 bytes\n{g_row}\nvs\n{w_row}"
        assert len(got) == 63 and sum(b"Typeable" in r for r in want) >= 32
        batch.close()
    finally:
        eng.ctx.set_option("prot_cap", 32768)  # (the library's default)
        eng.close()
