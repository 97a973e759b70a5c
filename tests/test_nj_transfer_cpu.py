"""Transfer bootstrap without a GPU (include/kp_spec.h, TRANSFER): kaptive_amd/csrc/kp_transfer.h under g++ against the set
restatement of tests/nj_transfer_util.py -- the distance of two splits from either side of either, the spec's known answer,
caterpillars against balanced trees, random record lists --; the label's thousandths at their edges; the formatter
(kp_format_nj_transfer) against the Python writer, sized and filled exactly, with its refusals; the binding; and the command line's
refusals."""

from __future__ import annotations

import ctypes as C
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from kaptive_amd import _native
from tests import nj_boot_util as B
from tests import nj_transfer_util as TR
from tests import nj_util as NJ

ROOT = Path(__file__).resolve().parent.parent


# ---- the spec and the binding ------------------------------------------------------------------------------------------------------------
def test_spec_and_binding():
    spec = (ROOT / "include" / "kp_spec.h").read_text()
    assert "---- TRANSFER (" in spec and spec.index("---- BOOTSTRAP (") < spec.index("---- TRANSFER (")
    boot = spec[spec.index("---- BOOTSTRAP (") : spec.index("---- TRANSFER (")]
    assert "transfer bootstrap" not in boot[boot.index("OUT OF SCOPE") :]
    caps = (ROOT / "kaptive_amd" / "csrc" / "kp_caps.h").read_text()
    assert re.search(r"static_assert\(KP_NJ_MAX_TAXA <= 65535", caps)
    lib = _native.lib()
    for name in ("kp_dist_nj_transfer", "kp_format_nj_transfer"):
        assert name in _native.EXPORTS and hasattr(lib, name), name
    assert hasattr(_native.Distances, "nj_transfer") and callable(_native.format_nj_transfer)


# ---- kp_transfer.h against sets -------------------------------------------------------------------------------------------------------------
def test_delta_from_both_sides_of_both_splits():
    h = TR.harness()
    for n in (4, 5, 9, 64, 200):
        rng = np.random.default_rng(n)
        everyone = frozenset(range(n))
        for _ in range(20):
            A = frozenset(rng.choice(n, int(rng.integers(1, n)), replace=False).tolist())
            S = frozenset(rng.choice(n, int(rng.integers(1, n)), replace=False).tolist())
            want = min(len(A ^ S), n - len(A ^ S))
            for a in (A, everyone - A):
                for s in (S, everyone - S):
                    assert h.kpy_transfer_delta(len(a), len(s), len(a & s), n) == want, (n, sorted(a), sorted(s))
            assert h.kpy_transfer_depth(len(A), n) == min(len(A), n - len(A)) == h.kpy_transfer_depth(n - len(A), n)
    assert h.kpy_transfer_delta(3, 3, 3, 8) == 0 and h.kpy_transfer_delta(3, 5, 0, 8) == 0  # the split itself, from either side


def test_the_known_answer_of_the_spec():
    ref, rep = TR.records(TR.KNOWN_REF), TR.records(TR.KNOWN_REP)
    assert [sorted(s) for s in B.record_splits(6, ref)[:3]] == [[2, 3, 4, 5], [3, 4, 5], [4, 5]] and TR.depths(6, ref) == [2, 3, 2, None]
    assert [sorted(s) for s in B.record_splits(6, rep)[:3]] == [[1, 2, 4, 5], [2, 4, 5], [4, 5]]
    assert TR.phi_of(6, ref, rep).tolist() == TR.KNOWN_PHI and TR.harness_phi(6, ref, rep).tolist() == TR.KNOWN_PHI[:3]
    support, transfer, phi = TR.sums_of(6, ref, [rep])
    assert support.tolist() == [0, 0, 1, -1] and transfer.tolist() == [1, 1, 0, -1] and B.support_of(6, ref, [rep]).tolist() == support.tolist()
    assert [TR.label(transfer[t], 1, d) for t, d in enumerate(TR.depths(6, ref)[:3])] == TR.KNOWN_LABELS
    h = TR.harness()
    assert [h.kpy_transfer_label(int(transfer[t]), 1, d) for t, d in enumerate((2, 3, 2))] == [0, 500, 1000]
    spec = (ROOT / "include" / "kp_spec.h").read_text()
    assert "(0, 3, -1), (6, 1, -1), (7, 2, -1), (8, 4, 5)" in spec and "0.000, 0.500, 1.000" in spec


@pytest.mark.parametrize("n", (8, 16))
def test_caterpillar_against_balanced(n):
    cat, bal = TR.caterpillar(n), TR.grown(n)
    assert TR.depths(n, cat)[:-1] == [min(k, n - k) for k in range(2, n - 1)] and max(TR.depths(n, cat)[:-1]) == n // 2
    for ref, rep in ((cat, bal), (bal, cat), (cat, cat), (bal, bal)):
        want = TR.phi_of(n, ref, rep)
        assert TR.harness_phi(n, ref, rep).tolist() == want[:-1].tolist() and want[-1] == -1
    assert TR.phi_of(n, cat, cat)[:-1].tolist() == [0] * (n - 3)
    mixed = TR.phi_of(n, cat, bal)[:-1]
    assert mixed.min() == 0 and mixed.max() >= 1  # the cherry (0, 1) is in both trees; the prefix {0, 1, 2} is in the caterpillar alone


@pytest.mark.parametrize("n", (4, 5, 6, 7, 34))
def test_random_record_lists(n):
    rng = np.random.default_rng([n, 11])
    seen = set()
    for _ in range(50):
        ref, rep = TR.grown(n, rng), TR.grown(n, rng)
        want = TR.phi_of(n, ref, rep)
        assert TR.harness_phi(n, ref, rep).tolist() == want[:-1].tolist()
        below = {k: 1 for k in range(n)}
        for t in range(n - 3):
            below[n + t] = below[int(ref[t]["a"])] + below[int(ref[t]["b"])]
        assert TR.harness_sizes(n, ref).tolist() == [below[n + t] for t in range(n - 3)]
        seen.update(want[:-1].tolist())
        assert (want[:-1] <= np.array(TR.depths(n, ref)[:-1]) - 1).all() and (want[:-1] >= 0).all()
        assert ((want[:-1] == 0) == (B.support_of(n, ref, [rep])[:-1] == 1)).all()  # the support relation
    if n == 34:
        assert max(seen) >= 5


def test_label_edges():
    h = TR.harness()
    cases = [(0, 1, 2), (1, 1, 2), (0, 7, 3), (14, 7, 3), (7, 7, 3), (6, 7, 3), (8, 7, 3)]  # D = 14: transfer 0, D, D / 2 and beside it
    cases += [(t, 5, 4) for t in range(16)]  # D = 15, odd: 2 * transfer = D - 1 and D + 1 among them
    cases += [(1, 1000, 2), (999, 1000, 2), (1, 3, 2), (2, 3, 2), (1, 6, 2), (5, 6, 2)]
    big = 10000 * 8191
    cases += [(0, 10000, 8192), (big, 10000, 8192), (big // 2, 10000, 8192), (big // 2 + 1, 10000, 8192), (big - 1, 10000, 8192), (1, 10000, 8192), (40955, 10000, 8192), (40956, 10000, 8192)]
    for transfer, replicates, depth in cases:
        D = replicates * (depth - 1)
        k = h.kpy_transfer_label(transfer, replicates, depth)
        want = ((1 - Fraction(transfer, D)) * 1000 + Fraction(1, 2)).__floor__()
        assert k == want and 0 <= k <= 1000, (transfer, replicates, depth, k)
        assert TR.label(transfer, replicates, depth) == f"{k // 1000}.{k % 1000:03d}".encode()
    assert 2 * 7 == 15 - 1 and 2 * 8 == 15 + 1 and h.kpy_transfer_label(7, 5, 4) == 533 and h.kpy_transfer_label(8, 5, 4) == 467
    assert h.kpy_transfer_label(big // 2, 10000, 8192) == 500 and 2000 * big + big < 2**63  # (and 2^39 in fact)


# ---- the formatter ---------------------------------------------------------------------------------------------------------------------------
def _format(locus, names, taxa, nodes, transfer, replicates, rows=None):
    return _native.format_nj_transfer(locus, names, np.asarray(taxa, np.int32), np.asarray(nodes, NJ.NODE_DTYPE), np.asarray(transfer, np.int64), replicates, rows)


def _rec(*r):
    return np.array([tuple(x[:3]) + (0,) + tuple(x[3:]) for x in r], NJ.NODE_DTYPE)


FIVE_NODES = _rec((0, 1, -1, 2, 3, 0), (5, 2, -1, 3, 4, 0), (6, 4, 3, 2, 1, 2))  # depths 2, 2


def test_formatter():
    names = list("abcde")
    assert _format("K1", names, range(5), FIVE_NODES, [13, 0, -1], 100) == b"K1\t5\t5\t100\t(((a:2,b:3)0.870:3,c:4)1.000:2,e:1,d:2);\n" == TR.line("K1", names, np.arange(5), FIVE_NODES, [13, 0, -1], 100)
    assert _format("", names, range(5), FIVE_NODES, [10000, 1, -1], 10000, rows=[4, 3, 2, 1, 0]) == b"\t5\t5\t10000\t(((e:2,d:3)0.000:3,c:4)1.000:2,a:1,b:2);\n"
    six = list("abcdef")
    assert _format("L", six, range(6), TR.records(TR.KNOWN_REF), [1, 1, 0, -1], 1) == b"L\t6\t6\t1\t((((a:0,b:0)0.000:0,c:0)0.500:0,d:0)1.000:0,e:0,f:0);\n"
    two = _rec((0, 1, -1, 0.5, 0.5, 0.0))
    assert _format("L", ["x", "y"], [0, 1], two, [-1], 7) == b"L\t2\t2\t7\t(x:0.5,y:0.5);\n" == TR.line("L", ["x", "y"], [0, 1], two, [-1], 7)
    odd, three = ["it's", "dropped", "two words", ""], _rec((0, 1, 2, 1 / 3, -0.125, 1e-12))
    assert _format("L", odd, [0, 2, 3], three, [-1], 1) == b"L\t4\t3\t1\t('it''s':0.333333333,'two words':-0.125,:1e-12);\n" == TR.line("L", odd, [0, 2, 3], three, [-1], 1)
    assert _format("L", ["x", "y"], [1], np.zeros(0, NJ.NODE_DTYPE), [], 5) == b"" == _format("L", [], [], np.zeros(0, NJ.NODE_DTYPE), [], 5)
    for n in (4, 5, 40):  # kp_format_nj_support's bytes but for the labels
        rng = np.random.default_rng(n)
        num, den = rng.integers(0, 12, (n, n)), rng.integers(40, 44, (n, n))
        dist = np.triu(num / den, 1)
        nodes, nm = NJ.nj(dist + dist.T), [f"asm {k}" if k % 3 == 0 else f"it's_{k}" if k % 3 == 1 else f"asm_{k}" for k in range(n + 2)]
        taxa, deep = np.delete(np.arange(n + 2), [1, n]), TR.depths(n, nodes)
        for N in (1, 16, 10000):
            sums = np.array([int(rng.integers(0, N * (d - 1) + 1)) for d in deep[:-1]] + [-1], np.int64)
            sums[0], sums[n - 4] = (0, N * (deep[n - 4] - 1)) if n > 4 else (N * (deep[0] - 1), N * (deep[0] - 1))
            got = _format("KL2", nm, taxa, nodes, sums, N)
            assert got == TR.line("KL2", nm, taxa, nodes, sums, N)
            counted = _native.format_nj_support("KL2", nm, taxa, nodes, np.array([0] * (n - 3) + [-1], np.int32), N)
            assert re.sub(rb"\)[01]\.\d{3}:", b")0:", got) == counted and len(re.findall(rb"\)[01]\.\d{3}:", got)) == n - 3
            assert b"." in got.split(b"\t", 4)[4]


def test_formatter_sized_then_filled_exactly():
    lib = _native.lib()
    lib.kp_format_nj_transfer.restype = C.c_int64
    names, taxa, sums = list("abcde"), np.arange(5, dtype=np.int32), np.array([13, 0, -1], np.int64)
    blob, off = _native._blob64(names)
    call = lambda nodes=B._p(FIVE_NODES), s=B._p(sums), out=None, cap=0, N=100: lib.kp_format_nj_transfer(  # noqa: E731
        b"x", 1, B._p(blob), B._p(off), 5, None, B._p(taxa), 5, nodes, C.c_int64(3), s, N, out, C.c_int64(cap))
    want = _format("x", names, taxa, FIVE_NODES, sums, 100)
    need = call()
    assert need == len(want)
    buf = np.full(need + 8, 0x3F, np.uint8)
    assert call(out=B._p(buf), cap=need) == need and buf[:need].tobytes() == want and (buf[need:] == 0x3F).all()
    short = np.full(need, 0x3F, np.uint8)
    assert call(out=B._p(short), cap=need - 1) == need and short[need - 1] == 0x3F  # one byte short: not written past
    assert call(s=None) == -1 and call(nodes=None) == -1 and call(cap=5) == -1  # null sums, null records, room without a buffer
    assert call(N=0) == -1 and call(N=10001) == -1


def test_formatter_refusals():
    names, all5 = list("abcde"), list(range(5))
    good = [3, 4, -1]  # depths 2, 2: at most `replicates` each
    bad = [
        (all5, FIVE_NODES, good, 0),  # replicates outside 1 .. 10 000
        (all5, FIVE_NODES, good, -1),
        (all5, FIVE_NODES, good, 10001),
        (all5, FIVE_NODES, [3, 5, -1], 4),  # more than replicates * (depth - 1)
        (all5, FIVE_NODES, [-1, 4, -1], 4),  # none at an inner edge
        (all5, FIVE_NODES, [3, -2, -1], 4),
        (all5, FIVE_NODES, [3, 4, 0], 4),  # one where there is no inner edge
        ([0, 1, 2, 3], FIVE_NODES, good, 4),  # kp_format_nj's refusals: the records of another tree
        ([0, 1, 3, 2, 4], FIVE_NODES, good, 4),
        (all5, _rec((0, 7, -1, 0, 0, 0), (5, 2, -1, 3, 4, 0), (6, 4, 3, 2, 1, 2)), good, 4),
        (all5, _rec((0, 1, -1, 0, 0, 0), (5, 5, -1, 3, 4, 0), (6, 4, 3, 2, 1, 2)), good, 4),  # a node that is a child twice
    ]
    for taxa, nodes, sums, N in bad:
        with pytest.raises(ValueError):
            _format("x", names, taxa, nodes, sums, N)
    assert _format("x", names, all5, FIVE_NODES, good, 4)
    with pytest.raises(ValueError):
        _format("x", names, all5, FIVE_NODES, good[:2], 4)  # a sum per record
    # the bound is the record's own: depth 3 of six taxa admits 2 a replicate, depth 2 only 1
    six, ref = list("abcdef"), TR.records(TR.KNOWN_REF)
    assert _format("x", six, range(6), ref, [3, 6, 3, -1], 3).count(b")0.000") == 3
    for sums in ([4, 6, 3, -1], [3, 7, 3, -1], [3, 6, 4, -1]):
        with pytest.raises(ValueError):
            _format("x", six, range(6), ref, sums, 3)


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
def test_command_line_flags(capsys):
    from kaptive_amd.cli import build_parser

    ap = build_parser()
    base = ["assembly", "db.npz", "a.fasta"]
    ns = ap.parse_args([*base, "--nj", "t.tsv", "--nj-bootstrap", "100"])
    assert ns.nj_bootstrap == 100 and not hasattr(ns, "nj_transfer")  # the bootstrap alone still parses, and says nothing of transfer
    ns = ap.parse_args([*base, "--nj", "t.tsv", "--nj-bootstrap", "100", "--nj-transfer"])
    assert ns.nj_transfer is True and ns.nj_bootstrap == 100
    assert ap.parse_args([*base, "--nj", "t.tsv", "--nj-transfer", "--nj-bootstrap", "7", "--nj-seed", "3"]).nj_seed == 3
    for bad, why in ((["--nj", "t.tsv", "--nj-transfer"], "--nj-transfer requires --nj-bootstrap N"), (["--nj-transfer"], "--nj-transfer requires --nj-bootstrap N"),
                     (["--nj-bootstrap", "5", "--nj-transfer"], "requires --nj FILE")):  # fmt: skip
        with pytest.raises(SystemExit):
            ap.parse_args([*base, *bad])
        assert why in capsys.readouterr().err, bad
