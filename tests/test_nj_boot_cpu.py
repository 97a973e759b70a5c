"""Bootstrap support without a GPU (include/kp_spec.h, BOOTSTRAP): kaptive_amd/csrc/kp_boot.h under g++ against the NumPy restatement
of tests/nj_boot_util.py -- the mixer, the draws and weights, the clamp, weighted counts, the keys of both sides of a split, the walk
over a record list against exact sets, the batch rule --; the formatter (kp_format_nj_support) against the Python writer, with its
refusals; and the command line's refusals."""

from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from kaptive_amd import _native
from tests import distances_util as D
from tests import nj_boot_util as B
from tests import nj_util as NJ

ROOT = Path(__file__).resolve().parent.parent
SEEDS = ((0, 0), (1, 0), (1, 1), (1, 9999), (2**64 - 1, 7), (0xDEADBEEF, 123))


def _random_matrix(rng, n):
    num, den = rng.integers(0, 12, (n, n)), rng.integers(40, 44, (n, n))
    d = np.triu(num / den, 1)
    return d + d.T


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------------
def test_constants_match_the_headers():
    out = np.zeros(4, np.int64)
    B.harness().kpy_boot_caps(B._p(out))
    assert out.tolist() == [B.MAX_REPLICATES, B.MATRIX_BYTES, B.MAX_BATCH, B.PLANES]
    assert (_native.BOOT_MAX_REPLICATES, _native.BOOT_MATRIX_BYTES, _native.BOOT_MAX_BATCH) == (B.MAX_REPLICATES, B.MATRIX_BYTES, B.MAX_BATCH)
    assert _native.nj_support_header() == B.HEADER and B.MATRIX_BYTES == NJ.MAX_TAXA**2 * 8
    caps = (ROOT / "kaptive_amd" / "csrc" / "kp_caps.h").read_text()
    assert int(re.search(r"KP_BOOT_MAX_REPLICATES\s*=\s*(\d+)", caps).group(1)) == B.MAX_REPLICATES
    spec = (ROOT / "include" / "kp_spec.h").read_text()
    assert "---- BOOTSTRAP (" in spec and "2^-64" in spec


# ---- kp_boot.h against NumPy ---------------------------------------------------------------------------------------------------------------
def test_mix():
    h = B.harness()
    xs = [0, 1, 2, 2**63, 2**64 - 1, 0x9E3779B97F4A7C15, *np.random.default_rng(1).integers(0, 2**63, 50).tolist()]
    want = B.mix(np.array(xs, np.uint64))
    assert [h.kpy_boot_mix(C.c_uint64(x)) for x in xs] == [int(v) for v in want]
    assert int(B.mix(np.array([0], np.uint64))[0]) == 0xE220A8397B1DCDAF  # SplitMix64's first output for the state 0


@pytest.mark.parametrize("W", (16, 64, 16 * 33))
def test_draws_and_weights(W):
    for seed, r in SEEDS:
        dr = B.draws(seed, r, W)
        assert B.harness_draws(seed, r, W).tolist() == dr.tolist() and dr.min() >= 0 and dr.max() < W
        w = B.weights(seed, r, W)
        assert B.harness_weights(seed, r, W).tobytes() == w.tobytes() and int(w.sum()) == W
    assert B.weights(1, 0, W).tobytes() != B.weights(1, 1, W).tobytes() != B.weights(2, 1, W).tobytes()


def test_the_clamp():
    count = [0, 1, 254, 255, 256, 1000, 2**32 - 1]
    assert B.harness_clamp(count).tolist() == B.clamp(count).tolist() == [0, 1, 254, 255, 255, 255, 255]


def test_weight_planes_of_a_word():
    h = B.harness()
    rng = np.random.default_rng(4)
    for W, hi in ((16, 256), (64, 4), (16 * 33, 9), (80, 1)):
        w = rng.integers(0, hi, W).astype(np.uint8)
        for word in range(-(-W // 64)):
            out = np.zeros(8, np.uint64)
            top = h.kpy_boot_word_planes(B._p(w), C.c_int64(W), C.c_int64(word), B._p(out))
            seg = np.concatenate([w[64 * word : 64 * word + 64], np.zeros(64, np.uint8)])[:64].astype(np.uint64)
            want = [int(sum(((int(v) >> k) & 1) << b for b, v in enumerate(seg))) for k in range(8)]
            assert [int(v) for v in out] == want and top == max([k + 1 for k in range(8) if want[k]], default=0)


@pytest.mark.parametrize("nb", (1, 4, 5, 33))
def test_weighted_counts(nb):
    rng = np.random.default_rng(nb)
    codes = D.population(rng, 24, nb)
    blocks = D.pack(codes).reshape(24, nb)
    for k, w in enumerate((B.weights(3, 0, 16 * nb), rng.integers(0, 256, 16 * nb).astype(np.uint8), np.zeros(16 * nb, np.uint8), np.ones(16 * nb, np.uint8))):
        for a, b in ((0, 1), (2, 5), (3, 4), (4, 10), (11, 12), (13, 20), (7, 7)):
            assert B.harness_counts(blocks[a], blocks[b], w) == B.weighted_counts(codes[a], codes[b], w), (k, a, b)
    comp, diff, _ = D.counts(codes[11], codes[12])
    assert B.weighted_counts(codes[11], codes[12], np.ones(16 * nb)) == (comp, diff)  # weight 1 everywhere: the unweighted counts


def test_keys_of_both_sides_of_a_split():
    h = B.harness()
    for n in (4, 5, 12, 200):
        rng = np.random.default_rng(n)
        total = int(h.kpy_boot_total(C.c_int32(n)))
        want_total = int(B.mix(np.arange(1, n + 1, dtype=np.uint64)).astype(object).sum()) & B.MASK
        assert total == want_total == B.harness_key(np.arange(n))
        for _ in range(5):
            side = np.sort(rng.choice(n, int(rng.integers(1, n)), replace=False))
            other = np.setdiff1d(np.arange(n), side)
            key = int(B.mix((side + 1).astype(np.uint64)).astype(object).sum()) & B.MASK
            assert B.harness_key(side) == key and B.harness_key(other) == (total - key) & B.MASK and len(other) == n - len(side)


@pytest.mark.parametrize("n", (4, 5, 6, 17, 66))
def test_the_walk_against_exact_sets(n):
    h = B.harness()
    total = int(h.kpy_boot_total(C.c_int32(n)))
    for seed in range(3):
        nodes = NJ.nj(_random_matrix(np.random.default_rng([n, seed]), n))
        got, want = B.harness_walk(n, nodes), B.record_splits(n, nodes)
        assert len(got) == n - 3 and want[n - 3 :] == [None]
        below = {k: frozenset([k]) for k in range(n)}
        for t in range(n - 3):
            below[n + t] = below[int(nodes[t]["a"])] | below[int(nodes[t]["b"])]
            s = sorted(want[t])
            assert 0 not in want[t] and int(got[t, 1]) == len(s) and int(got[t, 0]) == B.harness_key(s) and int(got[t, 2]) == (0 in below[n + t])
        assert len({(int(k), int(s)) for k, s, _ in got}) == n - 3  # the inner edges of a tree are different splits
    assert len(B.harness_walk(3, NJ.nj(_random_matrix(np.random.default_rng(0), 3)))) == 0 and total == B.harness_key(range(n))


def test_the_batch_rule():
    h = B.harness()
    for n, reps, most, want in ((4, 100, 0, 100), (4, 10000, 0, 10000), (16384, 100, 0, 1), (16383, 100, 0, 1), (11585, 100, 0, 2), (11586, 100, 0, 1), (1024, 10000, 0, 256),
                                (1024, 100, 7, 7), (1024, 100, 1, 1), (1024, 3, 7, 3), (2, 10000, 0, 10000), (0, 5, 0, 5), (1024, 10000, 1000, 256)):  # fmt: skip
        assert h.kpy_boot_batch(n, reps, most) == want == max(1, min(reps, B.MAX_BATCH, most or reps, (B.MATRIX_BYTES // (n * n * 8)) if n else reps)), (n, reps, most)


# ---- the formatter ---------------------------------------------------------------------------------------------------------------------------
def _format(locus, names, taxa, nodes, support, replicates, rows=None):
    return _native.format_nj_support(locus, names, np.asarray(taxa, np.int32), np.asarray(nodes, NJ.NODE_DTYPE), np.asarray(support, np.int32), replicates, rows)


def _rec(*r):
    return np.array([tuple(x[:3]) + (0,) + tuple(x[3:]) for x in r], NJ.NODE_DTYPE)


FIVE_NODES = _rec((0, 1, -1, 2, 3, 0), (5, 2, -1, 3, 4, 0), (6, 4, 3, 2, 1, 2))


def test_formatter():
    names = list("abcde")
    assert _format("K1", names, range(5), FIVE_NODES, [87, 0, -1], 100) == b"K1\t5\t5\t100\t(((a:2,b:3)87:3,c:4)0:2,e:1,d:2);\n" == B.line("K1", names, np.arange(5), FIVE_NODES, [87, 0, -1], 100)
    assert _format("", names, range(5), FIVE_NODES, [10000, 1, -1], 10000, rows=[4, 3, 2, 1, 0]) == b"\t5\t5\t10000\t(((e:2,d:3)10000:3,c:4)1:2,a:1,b:2);\n"
    # two and three taxa: no label; fewer: no line
    two = _rec((0, 1, -1, 0.5, 0.5, 0.0))
    assert _format("L", ["x", "y"], [0, 1], two, [-1], 7) == b"L\t2\t2\t7\t(x:0.5,y:0.5);\n" == B.line("L", ["x", "y"], [0, 1], two, [-1], 7)
    odd, three = ["it's", "dropped", "two words", ""], _rec((0, 1, 2, 1 / 3, -0.125, 1e-12))
    assert _format("L", odd, [0, 2, 3], three, [-1], 1) == b"L\t4\t3\t1\t('it''s':0.333333333,'two words':-0.125,:1e-12);\n" == B.line("L", odd, [0, 2, 3], three, [-1], 1)
    assert _format("L", ["x", "y"], [1], np.zeros(0, NJ.NODE_DTYPE), [], 5) == b"" == _format("L", [], [], np.zeros(0, NJ.NODE_DTYPE), [], 5)
    # random trees of 4, 5 and 40 taxa, names that need quoting, support 0 and support N: the writer against the restatement, and
    # kp_format_nj's bytes but for the labels and the column
    for n in (4, 5, 40):
        rng = np.random.default_rng(n)
        nodes, nm = NJ.nj(_random_matrix(rng, n)), [f"asm {k}" if k % 3 == 0 else f"it's_{k}" if k % 3 == 1 else f"asm_{k}" for k in range(n + 2)]
        taxa = np.delete(np.arange(n + 2), [1, n])
        for N in (1, 16, 10000):
            support = np.concatenate([rng.integers(0, N + 1, n - 3), [-1]]).astype(np.int32)
            support[0], support[n - 4] = (0, N) if n > 4 else (N, N)
            got = _format("KL2", nm, taxa, nodes, support, N)
            assert got == B.line("KL2", nm, taxa, nodes, support, N)
            plain = _native.format_nj("KL2", nm, taxa, nodes)
            head, text = got.split(b"\t", 4)[:4], got.split(b"\t", 4)[4]
            assert head == plain.split(b"\t")[:3] + [str(N).encode()] and re.sub(rb"\)\d+", b")", text) == plain.split(b"\t")[3]
            assert len(re.findall(rb"\)\d+:", text)) == n - 3 and text.endswith(b");\n")  # every inner edge labelled, the outermost node not


def test_formatter_refusals():
    names, all5 = list("abcde"), list(range(5))
    good = [3, 4, -1]
    bad = [
        (all5, FIVE_NODES, good, 0),  # replicates outside 1 .. 10 000
        (all5, FIVE_NODES, good, -1),
        (all5, FIVE_NODES, good, 10001),
        (all5, FIVE_NODES, [3, 5, -1], 4),  # more support than replicates
        (all5, FIVE_NODES, [3, -1, -1], 4),  # none at an inner edge
        (all5, FIVE_NODES, [3, 4, 0], 4),  # one where there is no inner edge
        ([0, 1, 2, 3], FIVE_NODES, good, 4),  # kp_format_nj's refusals: the records of another tree
        ([0, 1, 3, 2, 4], FIVE_NODES, good, 4),
        (all5, _rec((0, 7, -1, 0, 0, 0), (5, 2, -1, 3, 4, 0), (6, 4, 3, 2, 1, 2)), good, 4),
    ]
    for taxa, nodes, support, N in bad:
        with pytest.raises(ValueError):
            _format("x", names, taxa, nodes, support, N)
    assert _format("x", names, all5, FIVE_NODES, good, 4)
    with pytest.raises(ValueError):
        _format("x", names, all5, FIVE_NODES, good[:2], 4)  # a support value per record
    lib = _native.lib()
    lib.kp_format_nj_support.restype = C.c_int64
    taxa, sup = np.arange(5, dtype=np.int32), np.array(good, np.int32)
    blob, off = _native._blob64(names)
    call = lambda nodes=B._p(FIVE_NODES), s=B._p(sup), out=None, cap=0: lib.kp_format_nj_support(  # noqa: E731
        b"x", 1, B._p(blob), B._p(off), 5, None, B._p(taxa), 5, nodes, C.c_int64(3), s, 4, out, C.c_int64(cap))
    assert call() == len(_format("x", names, all5, FIVE_NODES, good, 4))  # the sizing form
    assert call(s=None) == -1 and call(nodes=None) == -1 and call(cap=5) == -1  # null support, null records, room without a buffer


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
def test_command_line_flags(capsys):
    from kaptive_amd.cli import build_parser

    ap = build_parser()
    base = ["assembly", "db.npz", "a.fasta"]
    ns = ap.parse_args([*base, "--nj", "t.tsv"])
    assert ns.nj == "t.tsv" and not hasattr(ns, "nj_bootstrap") and not hasattr(ns, "nj_seed")
    ns = ap.parse_args([*base, "--nj", "t.tsv", "--nj-bootstrap", "100"])
    assert ns.nj_bootstrap == 100 and not hasattr(ns, "nj_seed")
    ns = ap.parse_args([*base, "--nj", "t.tsv", "--nj-bootstrap", "10000", "--nj-seed", "0"])
    assert (ns.nj_bootstrap, ns.nj_seed) == (10000, 0)
    assert ap.parse_args([*base, "--nj", "t.tsv", "--nj-bootstrap", "1", "--nj-seed", str(2**64 - 1)]).nj_seed == 2**64 - 1
    for bad, why in ((["--nj-bootstrap", "5"], "requires --nj"), (["--newick", "n.tsv", "--nj-bootstrap", "5"], "requires --nj"),
                     (["--nj", "t.tsv", "--nj-seed", "3"], "requires --nj-bootstrap"), (["--nj", "t.tsv", "--nj-bootstrap", "0"], "out of range"),
                     (["--nj", "t.tsv", "--nj-bootstrap", "10001"], "out of range"), (["--nj", "t.tsv", "--nj-bootstrap", "-3"], "out of range"),
                     (["--nj", "t.tsv", "--nj-bootstrap", "5", "--nj-seed", "-1"], "out of range"), (["--nj", "t.tsv", "--nj-bootstrap", "x"], "invalid")):  # fmt: skip
        with pytest.raises(SystemExit):
            ap.parse_args([*base, *bad])
        assert why in capsys.readouterr().err, bad
