"""The three device sorts at every size class and list overflow, with the inputs of tests/sort_classes_util.py
(tests/test_sort_classes_oracle.py pins what those inputs are): kp_anchor_bsort_kernel against the oracle's sorted anchors
and the library's radix sort, both of its LDS lists full at the default constants; kp_hit_sort_kernel against the oracle's
hit tables on both sides of every padded size and with runs of equal leading keys through both of its methods; the cull
order and the kept list of kp_reduce_kernel against the host statement of the reduction, up to the limit of 2048 kept hits
and one past it."""

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.pack import pack_sequences_flat
from kaptive_amd.serotyping.core import Serotyper
from tests import sort_classes_util as U
from tests.test_gpu_parity import _adversarial_hits, _results_equal, _rows_of, _same_records

pytestmark = pytest.mark.gpu


# ---- A. anchor bucket sort --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bucket_setup(oracle):
    codes, off = pack_sequences_flat(U.bucket_gene_sequences())
    odb = oracle.OracleDB(codes, off)
    asms = U.bucket_batch(U.edge_trims(odb))
    packed = [a.packed() for a in asms]
    once = {a.id: (odb.anchors(pa), odb.align(pa)) for a, pa in zip(asms, packed)}  # (the overflow assembly: once)
    return codes, off, asms, packed, [once[a.id] for a in asms]


def _check_sorted_anchors(batch, hits, offs, asms, want, what):
    for i, (asm, (anchors, want_hits)) in enumerate(zip(asms, want)):
        got = batch.anchors(i)
        assert np.array_equal(got, anchors), f"{what}, {asm.id} (entry {i}): {len(got)} anchors, the oracle has {len(anchors)}"
        assert (got[1:] > got[:-1]).all(), f"{what}, {asm.id} (entry {i}): not strictly increasing"
        _same_records(hits[offs[i] : offs[i + 1]], want_hits, f"{what}: hits of {asm.id} (entry {i})")


def test_bucket_sort_at_every_class_edge_and_with_both_lists_full(bucket_setup):
    """One batch: the assembly that fills both LDS lists of kp_anchor_bsort_kernel (more than BS_BIG_LIST buckets of
    25..512 keys of every network width, more than BS_HUGE_LIST above 512), an assembly without an anchor, an ordinary one,
    every size class on both sides of its edge on either strand, and the first assembly again.  Sorted anchors equal the
    oracle's and strictly increase, hits equal the oracle's; the two copies of the overflow assembly give the same bytes
    (blocks do not see each other), a second pass on the same context gives the same bytes, and so does the library's sort."""
    codes, off, asms, packed, want = bucket_setup
    c = _native.Context(0)
    c.load_genes(codes, off)
    first = c.batch(packed)
    hits, offs = first.align()
    _check_sorted_anchors(first, hits, offs, asms, want, "bucket sort")
    last = len(asms) - 1
    assert asms[0].id == asms[last].id and first.anchors(0).tobytes() == first.anchors(last).tobytes()
    assert hits[offs[0] : offs[1]].tobytes() == hits[offs[last] : offs[last + 1]].tobytes()
    assert len(first.anchors(1)) == 0 and offs[1] == offs[2]
    again = c.batch(packed)
    hits2, offs2 = again.align()
    assert np.array_equal(offs, offs2) and hits.tobytes() == hits2.tobytes()
    for i in range(len(asms)):
        assert first.anchors(i).tobytes() == again.anchors(i).tobytes(), f"second pass, entry {i}"
    c.set_option("library_sort", 1)
    lib = c.batch(packed)
    hits_lib, offs_lib = lib.align()
    _check_sorted_anchors(lib, hits_lib, offs_lib, asms, want, "library sort")
    assert np.array_equal(offs, offs_lib) and hits.tobytes() == hits_lib.tobytes()
    for b in (first, again, lib):
        b.close()
    c.close()


def test_buckets_that_span_two_values_above_and_below_their_values_class(oracle):
    """More than 16384 genes, so a bucket is a gene's two strands: one gene with some 300 anchors on either strand (each
    value below BS_STAGE, the bucket ranked by the block) and one with some 14 on either (each value a wave ranking's, the
    bucket a network's)."""
    db = U.span_db()
    codes, goff = pack_sequences_flat(db.genes)
    odb = oracle.OracleDB(codes, goff)
    asm, a, b = U.span_assembly(db)
    pa = asm.packed()
    want = odb.anchors(pa)
    c = _native.Context(0)
    c.load_genes(codes, goff)
    batch = c.batch([pa, pa])
    hits, off = batch.align()
    for i in range(2):
        got = batch.anchors(i)
        assert np.array_equal(got, want) and (got[1:] > got[:-1]).all(), f"entry {i}"
        _same_records(hits[off[i] : off[i + 1]], odb.align(pa), f"hits of entry {i}")
    assert {a, b} <= set(hits["gene"].tolist())
    c.set_option("library_sort", 1)
    lib = c.batch([pa, pa])
    hits_lib, off_lib = lib.align()
    assert np.array_equal(lib.anchors(0), want) and np.array_equal(off, off_lib) and hits.tobytes() == hits_lib.tobytes()
    for x in (batch, lib):
        x.close()
    c.close()


# ---- B. hit sort ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hit_db():
    return U.hit_db()


@pytest.fixture(scope="module")
def engine(hit_db):
    from kaptive_amd.engine import Engine

    eng = Engine(hit_db)
    typer = Serotyper(hit_db)
    typer._engine = eng
    yield eng, typer
    eng.close()


def test_hit_sort_on_both_sides_of_every_padded_size_and_with_ties(oracle, hit_db, engine):
    """A_n: exactly n raw hits (n = 1, 2, every power of two from 64 to SORT_LDS with its neighbours, 4300): the bitonic
    network at every padded size and the rank sort.  T_n: runs of 6 and 2 hits equal in gene, order score and contig, through
    the network's tie pass (64, 65, 4096) and the rank sort's (4097, 4304).  Order, duplicates and mapq equal the oracle's."""
    eng, _ = engine
    odb = oracle.OracleDB(*pack_sequences_flat(hit_db.genes))
    asms = [U.raw_hit_assembly(hit_db, n) for n in U.RAW_SIZES] + [U.tie_assembly(hit_db, n) for n in U.TIE_SIZES]
    packed = [a.packed() for a in asms]
    batch = eng.ctx.batch(packed)
    hits, off = batch.align()
    assert np.diff(off).tolist() == list(U.RAW_SIZES + U.TIE_SIZES)
    for i, (asm, pa) in enumerate(zip(asms, packed)):
        _same_records(hits[off[i] : off[i + 1]], odb.align(pa), f"hits of {asm.id}")
    batch.close()


# ---- C. reduction: cull order and kept hits ------------------------------------------------------------------------------------------
def test_cull_order_on_both_sides_of_every_padded_size():
    """Adversarial hit tables (equal scores, equal matches, mapq 0 / 1 / 255, heavy overlaps: few kept hits) of n hits for n
    around the cull round of 64, the padded sizes of the bitonic cull order and the switch to its rank sort at SORT_LDS, half
    of them with a gene's hits in any order, through kp_batch_set_hits in one batch: results equal the host reduction."""
    from kaptive_amd.engine import Engine
    from tests.golden_util import case_names, hits_to_alignments, load_case, load_db

    db = load_db("k")
    cases = [load_case(n) for n in case_names() if n.startswith("random_hits")]
    pool = [c[1] for c in cases if c[0] == "k"]
    assert pool
    rng = np.random.default_rng(20261017)
    genomes = [pool[i % len(pool)] for i in range(len(U.CULL_SIZES))]
    tables = [_adversarial_hits(rng, db, g, n, by_score=i % 2 == 0).astype(_native.HIT_DTYPE) for i, (g, n) in enumerate(zip(genomes, U.CULL_SIZES))]
    eng = Engine(db)
    typer = Serotyper(db)
    typer._engine = eng
    batch = eng.ctx.batch([g.packed() for g in genomes])
    batch.align_async()
    batch.wait()
    off = np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int64)
    batch.set_hits(np.concatenate(tables), off)
    res = eng.type_batch(typer, batch, [g.id for g in genomes], genomes, aligned=True).results()
    want = [typer.reduce(g, hits_to_alignments(db, g, t)) for g, t in zip(genomes, tables)]
    for g, t, r, w in zip(genomes, tables, res, want):
        _results_equal(r, w, f"table of {len(t)} hits on {g.id}")
    assert _rows_of(res) == _rows_of(want)
    n_kept = [len(np.asarray(next(iter(w.to_dict()["gene_hits"].values())))) for w in want]
    assert min(n_kept) >= 2, n_kept  # (the cull had something to keep and something to drop in every table)
    batch.close()
    eng.close()


def _typed(engine, genomes):
    eng, typer = engine
    batch = eng.ctx.batch([g.packed() for g in genomes])
    try:
        return eng.type_batch(typer, batch, [g.id for g in genomes], genomes).results()
    finally:
        batch.close()


def test_kept_hits_on_both_sides_of_the_lds_copy_and_up_to_the_limit(hit_db, engine):
    """A_n, where nothing overlaps and every hit is kept: n around the cull round (64, 65, 128, 129), around the largest kept
    list kp_reduce_kernel clusters in LDS (291, 292, 293), and 2047 and 2048, the last sizes the cull scratch holds (planted
    in gene order: the one-lane clustering meets its records nearly sorted).  Results and report rows equal the host
    reduction's."""
    _, typer = engine
    consts = U.kernel_constants()
    e, limit = U.kept_lds_edge(consts), consts["KEPT_LDS"]
    genomes = [U.raw_hit_assembly(hit_db, n) for n in (64, 65, 128, 129, e - 1, e, e + 1)]
    genomes += [U.raw_hit_assembly(hit_db, n, in_gene_order=True) for n in (limit - 1, limit)]
    got = _typed(engine, genomes)
    want = [typer.call_with_host_reduction(g) for g in genomes]
    for g, r, w in zip(genomes, got, want):
        _results_equal(r, w, g.id)
        n_kept = len(np.asarray(next(iter(w.to_dict()["gene_hits"].values()))))
        assert n_kept == int(g.id.split("_")[1]), (g.id, n_kept)
    assert _rows_of(got) == _rows_of(want)


def test_one_kept_hit_past_the_limit_is_refused_and_the_context_goes_on(hit_db, engine):
    _, typer = engine
    limit = U.kernel_constants()["KEPT_LDS"]
    over = U.raw_hit_assembly(hit_db, limit + 1, in_gene_order=True)
    with pytest.raises(_native.NativeError, match=f"more than {limit} non-overlapping hits in one assembly"):
        _typed(engine, [over])
    small = U.raw_hit_assembly(hit_db, 64)
    got = _typed(engine, [small])
    want = typer.call_with_host_reduction(small)
    _results_equal(got[0], want, small.id)
    assert _rows_of(got) == _rows_of([want])
