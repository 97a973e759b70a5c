"""What the inputs of tests/sort_classes_util.py are, by the CPU oracle alone: every size class of the anchor bucket sort on
both sides of its edge in either strand's buckets, more listed buckets than either LDS list of that kernel holds at the
default constants, buckets that span two values, exact raw-hit counts around every padded size of the hit sort, and runs of
equal leading keys on both sides of its rank sort.  Every edge is derived from the constants in csrc/kp_bsort.hip and
csrc/kp_reduce.hip: whoever changes one gets a failure here, not an edge that tests/test_gpu_sort_classes.py quietly no
longer meets."""

import re
from pathlib import Path

import numpy as np
import pytest

from kaptive_amd.pack import pack_sequences_flat
from tests import sort_classes_util as U

ROOT = Path(__file__).resolve().parent.parent
MIN_DP_SCORE = 80  # KP_MIN_DP_SCORE of include/kp_spec.h (asserted below): a band task below it is no raw hit


@pytest.fixture(scope="module")
def consts():
    return U.kernel_constants()


@pytest.fixture(scope="module")
def bucket_odb(oracle):
    seqs = U.bucket_gene_sequences()
    return oracle.OracleDB(*pack_sequences_flat(seqs)), 2 * len(seqs)


@pytest.fixture(scope="module")
def hit_setup(oracle):
    db = U.hit_db()
    return db, oracle.OracleDB(*pack_sequences_flat(db.genes))


def test_sizes_follow_the_constants_in_the_sources(consts):
    c = consts
    assert c == dict(BS_THREADS=512, BS_STAGE=512, BS_RANK_MAX=24, BS_TILE=1024, KP_BS_BIG_LIST=1024, KP_BS_HUGE_LIST=64,
                     KEPT_LDS=2048, SORT_LDS=4096), "a constant moved: rebuild the inputs of tests/sort_classes_util.py around it"  # fmt: skip
    assert U.EDGE_SIZES == U.bucket_edges(c)
    # hit sort: a network padded to a power of two of at least 64, up to SORT_LDS; one and two hits; past SORT_LDS a rank sort
    raw = {1, 2, *U.padding_edges(64, c["SORT_LDS"]), max(U.RAW_SIZES)}
    assert set(U.RAW_SIZES) == raw and c["SORT_LDS"] + 200 < max(raw) <= U.HIT_LOCI * U.HIT_GENES_PER_LOCUS
    assert set(U.TIE_SIZES) == {64, 65, c["SORT_LDS"], c["SORT_LDS"] + 1, max(U.TIE_SIZES)} and max(U.TIE_SIZES) > c["SORT_LDS"] + 200
    # cull order: the same switch and padding (every other padded size), 64 candidates a round
    cull = {v for p in (64, 128, 1024, 2048, 4096) for v in (p - 1, p, p + 1)} | {max(U.CULL_SIZES)}
    assert set(U.CULL_SIZES) == cull and max(cull) > c["SORT_LDS"] and c["KEPT_LDS"] in cull
    assert U.kept_lds_edge(c) == 292
    spec = (ROOT / "include" / "kp_spec.h").read_text()
    assert int(re.search(r"#define\s+KP_MIN_DP_SCORE\s+(\d+)", spec).group(1)) == MIN_DP_SCORE



# ---- A. anchor bucket sort --------------------------------------------------------------------------------------------------------
def test_every_edge_size_occurs_on_both_strands(bucket_odb):
    odb, n_values = bucket_odb
    fwd, rev = U.edge_assemblies(U.edge_trims(odb))
    for asm, strand in ((fwd, 0), (rev, 1)):
        s = U.bucket_sizes(odb.anchors(asm.packed()), n_values)
        own = s[strand : 2 * U.N_EDGE_GENES : 2]
        assert tuple(own) == U.EDGE_SIZES, f"{asm.id}: {own}"
        assert set(U.EDGE_SIZES) <= set(s.tolist())
        assert s.sum() - own.sum() < 10, f"{asm.id}: stray anchors {s.sum() - own.sum()}"


def test_overflow_assembly_fills_both_lists_at_the_default_constants(bucket_odb, consts):
    odb, n_values = bucket_odb
    asm = U.overflow_assembly()
    assert int(np.sum(asm.contigs.lengths)) < 620_000
    s = U.bucket_sizes(odb.anchors(asm.packed()), n_values)
    rank_max, stage = consts["BS_RANK_MAX"], consts["BS_STAGE"]
    n_big = int(((s > rank_max) & (s <= stage)).sum())
    n_huge = int((s > stage).sum())
    assert n_big >= 1100 and n_big >= consts["KP_BS_BIG_LIST"] + 76, n_big
    assert n_huge >= 72 and n_huge >= consts["KP_BS_HUGE_LIST"] + 8, n_huge
    assert int((s > 600).sum()) == 0, np.sort(s)[-5:]  # (the one-lane path this input once met: bm^2 compares per bucket)
    # every width of the bitonic network is plentiful: whichever buckets find the list full, each width sorts on both sides
    for lo, hi in ((64, 128), (128, 256), (256, stage)):
        assert int(((s > lo) & (s <= hi)).sum()) >= 40, (lo, hi)
    assert int(((s > rank_max) & (s <= 64)).sum()) >= 900
    # and in every 64-bucket piece a wave walks there is a bucket of the lists' sizes (the list fills from all waves)
    big = (s > rank_max).astype(int)
    pieces = np.add.reduceat(big, np.arange(0, len(big), 64))
    assert (pieces[1:-1] > 30).all(), pieces


def test_batch_shape_of_the_bucket_test(bucket_odb):
    odb, n_values = bucket_odb
    batch = U.bucket_batch(U.edge_trims(odb))
    assert [a.id for a in batch] == ["both_lists_full", "no_anchor", "ordinary", "edges_forward", "edges_reverse", "both_lists_full"]
    assert len(odb.anchors(batch[1].packed())) == 0  # the kernel's n == 0 return
    n = len(odb.anchors(batch[2].packed()))
    assert 300 < n < 3000, n


def test_buckets_that_span_two_values(oracle, consts):
    db = U.span_db()
    assert len(db.genes) > 16_384  # (32 768 counters: a bucket is a gene's two strands)
    odb = oracle.OracleDB(*pack_sequences_flat(db.genes))
    asm, a, b = U.span_assembly(db)
    s = U.bucket_sizes(odb.anchors(asm.packed()), 2 * len(db.genes))
    fa, ra, fb, rb = (int(x) for x in (s[2 * a], s[2 * a + 1], s[2 * b], s[2 * b + 1]))
    assert 250 <= fa <= consts["BS_STAGE"] and 250 <= ra <= consts["BS_STAGE"] and fa + ra > consts["BS_STAGE"], (fa, ra)
    assert 9 <= fb <= consts["BS_RANK_MAX"] and 9 <= rb <= consts["BS_RANK_MAX"] and fb + rb > consts["BS_RANK_MAX"], (fb, rb)


# ---- B. hit sort ------------------------------------------------------------------------------------------------------------------
def test_raw_hit_counts_are_exact(hit_setup):
    db, odb = hit_setup
    assert len(db.genes) >= 4300
    for n in U.RAW_SIZES:
        pa = U.raw_hit_assembly(db, n).packed()
        hits = odb.align(pa)
        assert len(odb.joins(pa)) == 0, n
        assert U.raw_hit_count(odb, pa, MIN_DP_SCORE) == n, n
        assert len(hits) == n and len(np.unique(hits["gene"])) == n and hits["score"].min() >= 3 * MIN_DP_SCORE, n
        assert (hits["strand"] == -1).sum() == n // 3, n  # every third copy is a reverse complement


def test_kept_edge_assemblies_hold_one_hit_per_gene_in_gene_order(hit_setup, consts):
    """The inputs of the kept-hit edges: nothing overlaps (distinct copies 60 and more bases apart), so kept = hits = n; the
    two largest are planted in the order of the database."""
    db, odb = hit_setup
    for n in (consts["KEPT_LDS"] - 1, consts["KEPT_LDS"]):
        asm = U.raw_hit_assembly(db, n, in_gene_order=True)
        hits = odb.align(asm.packed())
        assert len(hits) == n and len(np.unique(hits["gene"])) == n
        by_place = hits[np.lexsort((hits["t_start"], hits["contig"]))]
        assert (np.diff(by_place["gene"]) > 0).all()
        same = by_place["contig"][1:] == by_place["contig"][:-1]
        assert (by_place["t_start"][1:][same] - by_place["t_end"][:-1][same] >= 55).all()


def test_tie_assemblies_hold_runs_of_six_and_two(hit_setup):
    db, odb = hit_setup
    for n in U.TIE_SIZES:
        pa = U.tie_assembly(db, n).packed()
        hits = odb.align(pa)
        assert len(odb.joins(pa)) == 0 and U.raw_hit_count(odb, pa, MIN_DP_SCORE) == n and len(hits) == n, n
        runs = np.bincount(U.leading_runs(hits), minlength=7)
        want = np.zeros(7, int)
        want[[1, 2, 6]] = n % 8, n // 8, n // 8
        assert np.array_equal(runs, want), (n, runs)
