"""The compositions of tests/large_batch_util.py land where tests/test_gpu_large_batches.py needs them, from the oracle's
hit tables and the batches' word offsets alone (no words are concatenated, no GPU): totals on the intended side of 2^31,
2^32 and 2^33 bases, bases 2^31 and 2^32 strictly inside a hit of the K database (the second inside a joined one), every
source many times on either side of 2^32, and the fillers' hit counts.  This keeps the GPU comparisons from becoming
vacuous, and makes the compositions reviewable without a GPU."""

from collections import Counter

import numpy as np
import pytest

from tests import large_batch_util as L

# hits of the fillers on (K, O): the only entries of any batch that may be without hits.  Locus-free fillers hold no
# database sequence at all unless they carry the extra contig of two / three K genes, whose hits are those genes' and
# their relatives' in other loci; plain random contigs have none.
FILLER_HITS = {
    ("free", "kpsc", 41_000, 0): (0, 0),
    ("free", "kpsc", 41_001, 2): (139, 0),
    ("free", "kpsc", 41_002, 0): (0, 0),
    ("free", "kpsc", 41_003, 3): (153, 0),
}


@pytest.fixture(scope="module")
def case_a(oracle):
    return L.benchmark_shape_batch()


@pytest.fixture(scope="module")
def case_c(oracle):
    return L.inside_limit_batch()


def _counts_around(keys, its, boundary):
    e = L.entry_of(L.word_offsets(keys, its), boundary)
    return Counter(keys[:e]), Counter(keys[e + 1 :])  # (the entry that holds the boundary counts for neither side)


def test_benchmark_shape_totals_and_counts(case_a):
    keys, its, fillers = case_a
    assert len(keys) == 1026 and [k for k in keys if k[0] != "src"] == fillers
    assert L.total_bases(keys, its) > 1 << 32, "case a no longer passes 2^32 bases"
    assert L.total_bases(keys, its) < L.MAX_BASES
    below, above = _counts_around(keys, its, 1 << 32)
    for k in L.sources("kpsc"):
        assert below[k] >= 8 and above[k] >= 4, f"{k}: {below[k]} times below 2^32, {above[k]} above"
    n_hits = sum(len(h) for k in keys for h in its[k].hits)
    assert n_hits > 1000 * len(keys), f"{n_hits} hits in {len(keys)} entries"
    for f in fillers:  # plain random contigs, a multiple of 64 long: they move what follows them and nothing else
        assert f[0] == "rand" and f[2] % 64 == 0 and its[f].packed.padded_len == f[2]
        assert [len(h) for h in its[f].hits] == [0, 0], f"{f}: hits {[len(h) for h in its[f].hits]}"


@pytest.mark.parametrize("boundary, joined", [(1 << 31, False), (1 << 32, True)])
def test_boundary_lies_inside_a_hit(case_a, boundary, joined):
    keys, its, _ = case_a
    e, inside = L.hit_across(keys, its, boundary)
    assert keys[e][0] == "src" and len(inside), f"base {boundary} (entry {e}, {keys[e]}) lies in no hit of the K database"
    off = L.word_offsets(keys, its)
    assert 16 * off[e] < boundary < 16 * off[e + 1]
    sp = L.hit_spans(keys, its, off, e)[inside]
    assert (sp[:, 0] < boundary - 1).all() and (sp[:, 1] - 1 > boundary).all()
    if joined:
        assert its[keys[e]].joined[inside].any(), f"base {boundary}: none of the {len(inside)} hits across it is a joined one"
    # both sides of the boundary hold hits of that entry, which a position narrowed to 31 / 32 bits would tear apart
    all_sp = L.hit_spans(keys, its, off, e)
    assert (all_sp[:, 1] <= boundary).any() and (all_sp[:, 0] > boundary).any()


def test_joined_hits_are_where_the_sweep_plants_them(case_a):
    """Every source with mid-gene events (i % 4 == 3) has joined hits, so one of them can be put across a boundary."""
    _, its, _ = case_a
    for i, k in enumerate(L.sources("kpsc")):
        if i % 4 == 3:
            assert its[k].joined.any(), f"{k} has no joined hit"
        assert len(its[k].hits[0]) > 0 and len(its[k].hits[1]) > 0, f"{k}: no hits"


def test_many_contigs_totals_and_counts(oracle):
    keys, its = L.many_contigs_batch()
    assert len(keys) == 1100 and all(k[0] == "src" for k in keys)
    assert 1 << 32 < L.total_bases(keys, its) < L.MAX_BASES
    assert sum(len(its[k].packed.ctg_len) for k in keys) > 1_500_000
    below, above = _counts_around(keys, its, 1 << 32)
    for k in L.sources("ab_k"):
        assert below[k] >= 8 and above[k] >= 4, f"{k}: {below[k]} times below 2^32, {above[k]} above"
        assert len(its[k].hits[0]) > 0


def test_inside_limit_total_and_fillers(case_c):
    keys, its, last = case_c
    assert L.total_bases(keys, its) == (1 << 33) - 64
    assert keys[-1] == last and last[0] == "rand" and [len(h) for h in its[last].hits] == [0, 0]
    n_free = sum(k[0] == "free" for k in keys)
    assert n_free >= 1600 and all(k[0] == "free" for k in keys[:n_free]), "the locus-free fillers come first"
    real = keys[n_free:-1]
    assert len(real) == 48 and set(real) == set(L.sources("kpsc"))
    off = L.word_offsets(keys, its)
    assert 16 * off[n_free] > 7 << 30, "the real sources no longer sit at the highest positions"  # (2^33 - 2^30)
    assert 16 * off[-2] + 64 * 128 > (1 << 33) - 64, "the last contig is longer than 8192 bases"
    assert set(FILLER_HITS) == set(L.free_fillers())
    for k, want in FILLER_HITS.items():
        assert tuple(len(h) for h in its[k].hits) == want, f"{k}: hits {[len(h) for h in its[k].hits]}"
        assert Counter(keys)[k] >= 64
    # fillers with hits lie on either side of 2^32 as well
    below, above = _counts_around(keys, its, 1 << 32)
    for k, want in FILLER_HITS.items():
        assert below[k] >= 8 and above[k] >= 8, f"{k}: {below[k]} times below 2^32, {above[k]} above"
