"""The CPU oracle on both sides of every limit of the join path (kp-align v5, include/kp_spec.h), with the assemblies of
tests/join_limits_util.py: whether the gene is joined and in how many pieces, its hit spans and, for the chaining
kernel's instances, the exact anchor counts.  This keeps the constructions honest without a GPU, so that
tests/test_gpu_join_limits.py, which compares the device with the oracle on them, cannot become vacuous."""

import numpy as np
import pytest

from kaptive_amd.pack import pack_contigs, pack_sequences_flat
from tests import join_limits_util as J

# label -> (n_pieces of every join of the gene that reports a hit, sorted (contig, q_start, q_end) of the gene's hits)
EXPECT = {
    'KP_JOIN_BW: insertion (forward strand) = 499, inside the limit': ([2], [(0, 0, 4002)]),
    'KP_JOIN_BW: insertion (forward strand) = 500, inside the limit': ([2], [(0, 0, 4002)]),
    'KP_JOIN_BW: insertion (forward strand) = 501, outside the limit': ([], [(0, 0, 1200), (0, 1199, 4002)]),
    'KP_JOIN_BW: insertion (forward strand) = 502, next': ([], [(0, 0, 1200), (0, 1200, 4002)]),
    'KP_JOIN_BW: insertion (reverse strand) = 499, inside the limit': ([2], [(0, 0, 4002)]),
    'KP_JOIN_BW: insertion (reverse strand) = 500, inside the limit': ([2], [(0, 0, 4002)]),
    'KP_JOIN_BW: insertion (reverse strand) = 501, outside the limit': ([], [(0, 0, 1200), (0, 1200, 4002)]),
    'KP_JOIN_BW: insertion (reverse strand) = 502, next': ([], [(0, 0, 1202), (0, 1200, 4002)]),
    'KP_JOIN_BW: deletion (forward strand) = 499, inside the limit': ([2], [(0, 0, 4002)]),
    'KP_JOIN_BW: deletion (forward strand) = 500, inside the limit': ([2], [(0, 0, 4002)]),
    'KP_JOIN_BW: deletion (forward strand) = 501, outside the limit': ([], [(0, 0, 1200), (0, 1701, 4002)]),
    'KP_JOIN_BW: deletion (forward strand) = 502, next': ([], [(0, 0, 1200), (0, 1702, 4002)]),
    'KP_JOIN_BW: deletion (reverse strand) = 499, inside the limit': ([2], [(0, 0, 4002)]),
    'KP_JOIN_BW: deletion (reverse strand) = 500, inside the limit': ([2], [(0, 0, 4002)]),
    'KP_JOIN_BW: deletion (reverse strand) = 501, outside the limit': ([], [(0, 0, 1200), (0, 1701, 4002)]),
    'KP_JOIN_BW: deletion (reverse strand) = 502, next': ([], [(0, 0, 1200), (0, 1702, 4002)]),
    "KP_JOIN_BW: weak cluster's distance from both neighbours = 500, inside the limit": ([3], [(0, 0, 4002)]),
    "KP_JOIN_BW: weak cluster's distance from both neighbours = 501, outside the limit": ([], [(0, 0, 1500), (0, 1525, 4002)]),
    'KP_DIAG_GAP: insertion = 32, inside the limit': ([], [(0, 0, 4002)]),
    'KP_DIAG_GAP: insertion = 33, outside the limit': ([2], [(0, 0, 4002)]),
    'KP_DIAG_GAP: deletion = 32, inside the limit': ([], [(0, 0, 4002)]),
    'KP_DIAG_GAP: deletion = 33, outside the limit': ([2], [(0, 0, 4002)]),
    "KP_MAX_SPREAD: spread of one stretch's diagonals = 97, inside the limit": ([], [(0, 0, 4002)]),
    "KP_MAX_SPREAD: spread of one stretch's diagonals = 98, outside the limit": ([2], [(0, 0, 4002)]),
    'KP_JOIN_MAX_PIECES: pieces of a chain = 7, inside the limit': ([7], [(0, 0, 4002)]),
    'KP_JOIN_MAX_PIECES: pieces of a chain = 8, inside the limit': ([8], [(0, 0, 4002)]),
    'KP_JOIN_MAX_PIECES: pieces of a chain = 9, outside the limit': ([], [(0, 0, 4002), (0, 250, 2000)]),
    'KP_JOIN_MAX_PIECES: pieces of a chain (64-diagonal band) = 8, inside the limit': ([8], [(0, 0, 4002)]),
    'KP_JOIN_MAX_PIECES: pieces of a chain (64-diagonal band) = 9, outside the limit': ([], [(0, 0, 4002), (0, 250, 2000)]),
    'KP_JOIN_OPEN: further contigs = 3, inside the limit': ([2], [(0, 0, 800), (1, 800, 1100), (2, 1100, 1400), (3, 1400, 1700)]),
    'KP_JOIN_OPEN: further contigs = 4, outside the limit': ([], [(0, 0, 300), (0, 500, 800), (1, 800, 1100), (2, 1100, 1400), (3, 1400, 1700), (4, 1700, 2000)]),
    'KP_JOIN_OPEN: further contigs = 5, next': ([], [(0, 0, 300), (0, 500, 801), (1, 800, 1100), (2, 1100, 1400), (3, 1400, 1700), (4, 1700, 2000), (5, 2000, 2300)]),
    'KP_JOIN_OPEN: further contigs = 1, inside the limit': ([2], [(0, 0, 802), (1, 800, 1100)]),
    'KP_JOIN_GROUP_MAX: decoy clusters before the pair = 14, inside the limit': ([2], [(0, 0, 1205)]),
    'KP_JOIN_GROUP_MAX: decoy clusters before the pair = 15, outside the limit': ([], [(0, 0, 601), (0, 600, 1201)]),
    'KP_JOIN_GROUP_MAX: decoy clusters before the pair = 16, next': ([2], [(0, 0, 1200)]),
    'JA_SMALL: anchors of the group = 1024, inside the limit': ([2], [(0, 0, 5568)]),
    'JA_SMALL: anchors of the group = 1025, outside the limit': ([2], [(0, 0, 5571)]),
    'KP_JOIN_ANCHOR_MAX: anchors of the group = 4096, inside the limit': ([2], [(0, 0, 22009)]),
    'KP_JOIN_ANCHOR_MAX: anchors of the group = 4097, outside the limit': ([], [(0, 0, 2000), (0, 2000, 22014)]),
}


@pytest.fixture(scope="module")
def odb(oracle):
    return oracle.OracleDB(*pack_sequences_flat(J.database().genes))


@pytest.fixture(scope="module")
def sides():
    return J.join_limit_cases()


def test_every_side_is_expected(sides):
    assert [s.label for s in sides] == list(EXPECT), "a case was added, removed or renamed: update EXPECT"


@pytest.mark.parametrize("label", list(EXPECT))
def test_oracle_lands_on_the_intended_side(odb, sides, label):
    s = next(x for x in sides if x.label == label)
    pa = pack_contigs(s.asm.contigs)
    hits, joins = odb.align(pa), odb.joins(pa)
    hits, joins = hits[hits["gene"] == s.gene], joins[joins["gs"] // 2 == s.gene]
    joined = sorted(int(j["n_pieces"]) for j in joins if (j["piece"][:, 0] == 1).any())
    spans = sorted((int(h["contig"]), int(h["q_start"]), int(h["q_end"])) for h in hits)
    want_joined, want_spans = EXPECT[label]
    assert joined == want_joined, f"{label}: joins of {joined} pieces, expected {want_joined}"
    assert spans == want_spans, f"{label}: hits {spans}, expected {want_spans}"
    assert len(joins) == len(joined), f"{label}: a join whose path reports nothing"


def test_join_is_decided_by_the_limit(sides):
    """What EXPECT freezes follows the limits: inside KP_JOIN_BW, KP_JOIN_MAX_PIECES, KP_JOIN_OPEN, KP_JOIN_GROUP_MAX and
    KP_JOIN_ANCHOR_MAX the gene is one joined hit, just outside them it is two or more; KP_DIAG_GAP and KP_MAX_SPREAD work the
    other way round (inside: one cluster, no join); both instances of the chaining kernel join (JA_SMALL), and so does the
    pair behind 16 decoys, which fill a sequence of their own."""
    for s in sides:
        joined, spans = EXPECT[s.label]
        if s.limit == "JA_SMALL" or (s.limit == "KP_JOIN_GROUP_MAX" and s.side == "next"):
            want = True
        elif s.limit in ("KP_DIAG_GAP", "KP_MAX_SPREAD"):
            want = s.side != "inside"
        else:
            want = s.side == "inside"
        assert bool(joined) == want, f"{s.label}: joined {joined}"
        # contig 0 holds the limit's gene: one hit when joined or a single cluster, two or more when the join is lost
        single = want or s.limit in ("KP_DIAG_GAP", "KP_MAX_SPREAD")
        assert (sum(x[0] == 0 for x in spans) == 1) == single, f"{s.label}: hits {spans}"


def test_anchor_counts_of_the_chaining_instances(odb):
    """Case f holds exactly 1024, 1025, 4096 and 4097 anchors of F on its contig: a change in the generator or in the seeding
    shows up here, not as a quiet drift away from the instances' thresholds."""
    sides = J.anchor_counts()
    for s in sides:
        a = odb.anchors(pack_contigs(s.asm.contigs))
        n = int(((a >> np.uint64(46)) == np.uint64(2 * J.F)).sum())
        assert n == s.value, f"{s.label}: {n} anchors"
        assert len(a) == n, f"{s.label}: anchors of other genes ({len(a) - n})"
