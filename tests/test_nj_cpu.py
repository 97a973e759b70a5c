"""Neighbour joining without a GPU (include/kp_spec.h, NJ): kaptive_amd/csrc/kp_nj.h under g++ against the NumPy restatement of
tests/nj_util.py, byte for byte on the records; the section's known answers; the taxon rule at its edge; SUM64 against its
definition; a planted additive tree, whose splits and total length the rule must recover; and the formatter (kp_format_nj) with its
refusals.  tests/native_harness/nj_format_main.cpp repeats the formatter's part as a stand-alone program for the host sanitizers."""

from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from kaptive_amd import _native
from tests import distances_util as D
from tests import nj_util as NJ

ROOT = Path(__file__).resolve().parent.parent
FIVE = np.array([[0, 5, 9, 9, 8], [5, 0, 10, 10, 9], [9, 10, 0, 8, 7], [9, 10, 8, 0, 3], [8, 9, 7, 3, 0]], np.float64)
FIVE_NODES = np.array([(0, 1, -1, 0, 2, 3, 0), (5, 2, -1, 0, 3, 4, 0), (6, 4, 3, 0, 2, 1, 2)], NJ.NODE_DTYPE)


def _random_matrix(rng, n):
    """A symmetric matrix of p-distance-like ratios with many ties: few distinct numerators over few denominators."""
    num, den = rng.integers(0, 12, (n, n)), rng.integers(40, 44, (n, n))
    d = np.triu(num / den, 1)
    return d + d.T


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------------
def test_constants_match_the_headers():
    h = NJ.harness()
    assert h.kpy_nj_max_taxa() == NJ.MAX_TAXA == _native.NJ_MAX_TAXA == 16384
    assert h.kpy_nj_node_size() == NJ.NODE_DTYPE.itemsize == _native.NJ_NODE_DTYPE.itemsize == 40
    assert _native.NJ_NODE_DTYPE == NJ.NODE_DTYPE and _native.nj_header() == NJ.HEADER
    caps = (ROOT / "kaptive_amd" / "csrc" / "kp_caps.h").read_text()
    assert int(re.search(r"KP_NJ_MAX_TAXA\s*=\s*(\d+)", caps).group(1)) == NJ.MAX_TAXA
    spec = (ROOT / "include" / "kp_spec.h").read_text()
    assert "---- NJ (" in spec and "KP_NJ_MAX_TAXA = 16384" in spec


# ---- header against NumPy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 1, 2, 3, 4, 5, 6, 63, 64, 65, 129, 197))
def test_header_against_numpy(n):
    for seed in range(2):
        d = _random_matrix(np.random.default_rng([n, seed]), n)
        got, want = NJ.harness_nj(d), NJ.nj(d)
        assert len(got) == len(want) == (0 if n <= 1 else 1 if n == 2 else n - 2)
        if got.tobytes() != want.tobytes():
            i = next(i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes())
            raise AssertionError(f"n {n}, seed {seed}: record {i}: {got[i]} from the header, {want[i]} from NumPy")
        assert not got["pad"].any() and (got["c"][:-1] == -1).all() and not got["lc"][:-1].any()


def test_known_answers():
    for tree in (NJ.harness_nj(FIVE), NJ.nj(FIVE)):
        assert tree.tobytes() == FIVE_NODES.tobytes()
    # the second join: Q = -28 at the slots (0, 2) and (1, 3) -- after the first join the slots hold the nodes 5, 4, 2, 3
    d = FIVE.copy()
    u = 0.5 * ((d[0, 2:] + d[1, 2:]) - d[0, 1])
    four = np.zeros((4, 4))
    order = [None, 4, 2, 3]  # slot 1 took the last slot's node
    for s, node in enumerate(order[1:], 1):
        four[0, s] = four[s, 0] = u[node - 2]
        for s2, node2 in enumerate(order[1:], 1):
            four[s, s2] = d[node, node2]
    R = four.sum(axis=1)
    q = 2.0 * four - R[:, None] - R[None, :]
    assert q[0, 2] == q[1, 3] == -28.0 and min(q[a, b] for a in range(4) for b in range(a + 1, 4)) == -28.0
    zero = np.zeros((6, 6))
    want = np.array([(0, 1, -1, 0, 0, 0, 0), (6, 5, -1, 0, 0, 0, 0), (7, 4, -1, 0, 0, 0, 0), (8, 3, 2, 0, 0, 0, 0)], NJ.NODE_DTYPE)
    assert NJ.harness_nj(zero).tobytes() == NJ.nj(zero).tobytes() == want.tobytes()
    assert NJ.newick(list("abcde"), np.arange(5), FIVE_NODES) == b"(((a:2,b:3):3,c:4):2,e:1,d:2);"


# ---- the taxon rule at its edge ----------------------------------------------------------------------------------------------------------
def test_taxon_rule_at_its_edge():
    h = NJ.harness()
    W, mc = 64, 2
    assert h.kpy_nj_taxon(33, W, mc) == 1 and h.kpy_nj_taxon(32, W, mc) == 0
    assert h.kpy_nj_taxon(32, W, 0) == 0 and h.kpy_nj_taxon(33, W, 0) == 1 and h.kpy_nj_taxon(33, W, 1) == 1 and h.kpy_nj_taxon(33, W, 3) == 0  # m0 = max(min_compared, 1)
    codes = np.full((3, W), D.GAP, np.uint8)
    codes[0, :33], codes[1, 31:], codes[2, :32] = 0, 1, 0  # bases in columns 0..32, 31..63 and 0..31
    assert NJ.taxa_of(codes, mc).tolist() == [0, 1]
    assert D.counts(codes[0], codes[1]) == (2, 2, 62)  # the pigeonhole bound is met exactly: two compared columns
    blocks = D.pack(codes).reshape(3, -1)
    taxa, dist = NJ.harness_matrix(blocks, mc)
    assert taxa.tolist() == [0, 1] and dist.tolist() == [[0.0, 1.0], [1.0, 0.0]]
    assert dist.tobytes() == NJ.matrix_of(codes, taxa).tobytes()
    assert NJ.harness_nj(dist).tobytes() == NJ.nj(dist).tobytes() == np.array([(0, 1, -1, 0, 0.5, 0.5, 0)], NJ.NODE_DTYPE).tobytes()
    assert NJ.harness_matrix(blocks, 3)[0].tolist() == [] and NJ.taxa_of(codes, 3).tolist() == []


@pytest.mark.parametrize("R,nb,mc", ((40, 3, 1), (70, 9, 20), (20, 1, 0)))
def test_taxa_and_matrix_against_numpy(R, nb, mc):
    codes = D.population(np.random.default_rng([R, nb]), R, nb)
    taxa, dist = NJ.harness_matrix(D.pack(codes).reshape(R, -1), mc)
    want = NJ.taxa_of(codes, mc)
    assert 2 < len(want) < R and taxa.tobytes() == want.tobytes() and dist.tobytes() == NJ.matrix_of(codes, want).tobytes()
    if R >= 16:
        assert 2 not in taxa and 3 not in taxa  # the all-GAP and the all-N row
    assert NJ.harness_nj(dist).tobytes() == NJ.nj(dist).tobytes()


# ---- SUM64 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (0, 1, 2, 63, 64, 65, 66, 127, 128, 129, 130, 191, 192, 193))
def test_sum64_against_its_definition(m):
    v = 1.0 / (3.0 * np.arange(m) + 1.0) * np.random.default_rng(m).integers(1, 1000, m)
    s = [0.0] * 64
    for k in range(m):
        s[k % 64] = s[k % 64] + float(v[k])
    o = 32
    while o:
        for lane in range(o):
            s[lane] = s[lane] + s[lane + o]
        o //= 2
    assert NJ.harness_sum64(v) == float(NJ.sum64(v)) == s[0]


# ---- an additive tree ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (4, 5, 9, 40, 150))
def test_additive_tree_is_recovered(n):
    codes, planted, mutations, W = NJ.additive(np.random.default_rng(n), n)
    blocks = D.pack(codes).reshape(n, -1)
    taxa, dist = NJ.harness_matrix(blocks, 1)
    assert taxa.tolist() == list(range(n))
    nodes = NJ.harness_nj(dist)
    assert nodes.tobytes() == NJ.nj(NJ.matrix_of(codes, taxa)).tobytes()
    assert NJ.splits(n, nodes) == planted and len(planted) == n - 3
    assert abs(NJ.total_length(nodes) - mutations / W) <= 1e-12
    assert (np.concatenate([nodes["la"], nodes["lb"], nodes["lc"][-1:]]) > -1e-12).all()


# ---- the formatter -----------------------------------------------------------------------------------------------------------------------------
def _format(locus, names, taxa, nodes, rows=None):
    return _native.format_nj(locus, names, np.asarray(taxa, np.int32), np.asarray(nodes, NJ.NODE_DTYPE), rows)


def _rec(*r):
    return np.array([tuple(x[:3]) + (0,) + tuple(x[3:]) for x in r], NJ.NODE_DTYPE)


def test_formatter():
    names = list("abcde")
    assert _format("K1", names, range(5), FIVE_NODES) == b"K1\t5\t5\t(((a:2,b:3):3,c:4):2,e:1,d:2);\n" == NJ.line("K1", names, np.arange(5), FIVE_NODES)
    assert _format("", names, range(5), FIVE_NODES, rows=[4, 3, 2, 1, 0]) == b"\t5\t5\t(((e:2,d:3):3,c:4):2,a:1,b:2);\n"
    # quoting, %.9g, a negative length, three taxa among four rows
    odd, three = ["it's", "skipped", "two words", ""], _rec((0, 1, 2, 1.0 / 3.0, -0.125, 1e-12))
    assert _format("L", odd, [0, 2, 3], three) == b"L\t4\t3\t('it''s':0.333333333,'two words':-0.125,:1e-12);\n" == NJ.line("L", odd, [0, 2, 3], three)
    for v in (0.1 + 0.2, 123456789.123, 1e-5, 5e-324, 1.0, 0.0, -0.0, 2.5e-4 / 3):
        rec = _rec((0, 1, -1, v, v, 0.0))
        assert _format("L", ["x", "y"], [0, 1], rec) == f"L\t2\t2\t(x:{v:.9g},y:{v:.9g});\n".encode() == NJ.line("L", ["x", "y"], [0, 1], rec)  # two taxa
    assert _format("L", ["x", "y"], [1], np.zeros(0, NJ.NODE_DTYPE)) == b"" == _format("L", [], [], np.zeros(0, NJ.NODE_DTYPE))  # fewer than two taxa: no line
    # random trees: the writer against the restatement
    for n in (4, 7, 66):
        d = _random_matrix(np.random.default_rng(n), n)
        nodes, nm = NJ.nj(d), [f"asm {k}" if k % 3 == 0 else f"asm_{k}" for k in range(n + 2)]
        taxa = np.delete(np.arange(n + 2), [1, n])
        assert _format("KL2", nm, taxa, nodes) == NJ.line("KL2", nm, taxa, nodes)


def test_formatter_refusals():
    names, all5 = list("abcde"), list(range(5))
    k0, k1, k2 = ((0, 1, -1, 2, 3, 0), (5, 2, -1, 3, 4, 0), (6, 4, 3, 2, 1, 2))
    bad = [
        ([0, 1, 2, 3, 5], _rec(k0, k1, k2), None),  # a taxon outside the rows
        ([0, 1, 3, 2, 4], _rec(k0, k1, k2), None),  # taxa that do not ascend
        ([0, 1, 2, 3], _rec(k0, k1, k2), None),  # the records of another tree
        (all5, _rec(k0, k1), None),
        (all5, _rec((0, 7, -1, 0, 0, 0), k1, k2), None),  # a node id outside the range
        (all5, _rec((-1, 1, -1, 0, 0, 0), k1, k2), None),
        (all5, _rec((0, 5, -1, 0, 0, 0), k1, k2), None),  # a cycle: its own node
        (all5, _rec((0, 6, -1, 0, 0, 0), k1, k2), None),  # ... a later one
        (all5, _rec(k0, (5, 1, -1, 0, 0, 0), k2), None),  # a child used twice
        (all5, _rec(k0, (5, 5, -1, 0, 0, 0), k2), None),
        (all5, _rec((0, 1, 2, 0, 0, 0), k1, k2), None),  # a third child before the end
        (all5, _rec(k0, k1, (6, 4, -1, 0, 0, 0)), None),  # none at the end
        (all5, _rec(k0, k1, k2), [0, 1, 2, 3, 5]),  # a row outside the names
    ]
    for taxa, nodes, rows in bad:
        with pytest.raises(ValueError):
            _format("x", names, taxa, nodes, rows)
    with pytest.raises(ValueError):
        _format("x", ["x", "y"], [0, 1], _rec((0, 1, 0, 0, 0, 0)))
    lib = _native.lib()
    lib.kp_format_nj.restype = C.c_int64
    assert lib.kp_format_nj(b"x", 1, None, None, 0, None, None, 0, None, C.c_int64(0), None, C.c_int64(5)) == -1  # room without a buffer
    assert lib.kp_format_nj(None, 1, None, None, 0, None, None, 0, None, C.c_int64(0), None, C.c_int64(0)) == -1
