"""Pairwise locus distances, the parts that need no GPU (include/kp_spec.h, DISTANCES): the specification's known answers through the
restatement of tests/distances_util.py and through kp_dist.h built with g++ (tests/native_harness/dist_harness.cpp) -- planes of a
block, counts of a plane word, the padding mask, the listing predicate at its edges, the tile a workgroup owns --; ``LocusRows`` on
hand-made kept and row tables against the gene-by-gene restatement; ``state()`` / ``merge()``; kp_format_distances byte for byte; the
mirrors of the header's constants; the command line's flags."""

from __future__ import annotations

import ctypes as C
import pickle
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.distances import DIST_RECORD_DTYPE, LocusRows, pad_masks
from kaptive_amd.serotyping.batch import KEPT_DTYPE, SUMMARY_DTYPE
from tests import distances_util as D

ROOT = Path(__file__).resolve().parent.parent
ROW_A, ROW_B = "--acgt--nacg--------", "--cgtn--acgt--------"  # the known-answer rows of ALIGNED ROWS, a gene of 20 bases
BLOCKS_A, BLOCKS_B = (0xF0C3010000900E40, 0x000F000000000000), (0xF0C3002000E40390, 0x000F000000000000)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the specification's known answers ---------------------------------------------------------------------------------------------------
def test_known_answers_through_the_restatement_and_the_header():
    a, b, gap = D.codes_of(ROW_A), D.codes_of(ROW_B), np.full(20, D.GAP, np.uint8)
    assert D.counts(a, b) == (6, 6, 0) and D.counts(a, gap) == (0, 0, 8) and D.counts(b, gap) == (0, 0, 8) and D.counts(gap, gap) == (0, 0, 0)
    ba, bb, bg = D.gene_blocks(a), D.gene_blocks(b), D.gene_blocks(gap)
    # the locus row is the ALIGNED ROWS row with the padding flagged: ffff, not 000f, in the second block's gap mask
    assert [int(x) for x in ba] == [BLOCKS_A[0], BLOCKS_A[1] | (0xFFF0 << 48)] and int(ba[1]) >> 48 == 0xFFFF
    assert [int(x) for x in bb] == [BLOCKS_B[0], BLOCKS_B[1] | (0xFFF0 << 48)]
    assert D.harness_counts(ba, bb) == (6, 6, 0) and D.harness_counts(ba, bg) == (0, 0, 8) and D.harness_counts(bg, bb) == (0, 0, 8)
    assert D.harness_counts(bg, bg) == (0, 0, 0)  # GAP against GAP, padding against padding included
    # left unflagged, the twelve padding columns would read as base a on both sides
    assert D.harness_counts(np.array(BLOCKS_A, np.uint64), np.array(BLOCKS_B, np.uint64)) == (18, 6, 0)
    assert D.all_pairs(np.stack([D.unpack(ba), D.unpack(bb), D.unpack(bg)])).tolist() == [(0, 1, 6, 6, 0, 0), (0, 2, 0, 0, 8, 0), (1, 2, 0, 0, 8, 0)]


def test_planes_of_a_block_and_of_a_short_last_word():
    h = D.harness()
    out = np.zeros(4, np.uint32)
    h.kpy_dist_block_planes(C.c_uint64(BLOCKS_A[0]), _p(out))
    codes = D.codes_of(ROW_A[:16])
    want = [sum(((int(c) >> bit) & 1) << j for j, c in enumerate(codes) if c < 4) for bit in (0, 1)]
    assert out.tolist() == [*want, sum(1 << j for j, c in enumerate(codes) if c < 4), sum(1 << j for j, c in enumerate(codes) if c != D.GAP)]
    rng = np.random.default_rng(3)
    for nb in (1, 3, 4, 5, 9):
        codes = rng.integers(0, 6, 16 * nb).astype(np.uint8)
        blocks = D.pack(codes)
        # a block whose N or GAP columns carry stray code bits gives the same planes: the bits are dropped
        dirty = blocks | np.uint64(0xFFFFFFFF) if nb == 3 else blocks
        nw = (nb + 3) // 4
        got = np.zeros(4 * nw, np.uint64)
        h.kpy_dist_word_planes(_p(np.ascontiguousarray(dirty)), C.c_int64(nb), _p(got))
        padded = np.concatenate([codes, np.full(64 * nw - len(codes), D.GAP, np.uint8)]).reshape(nw, 64)  # missing columns: invalid, not present
        if nb == 3:
            padded = np.where(padded < 4, 3, padded)  # (the stray bits make every valid column a t)
        for w in range(nw):
            c = padded[w]
            bits = lambda mask: sum(1 << int(j) for j in np.flatnonzero(mask))  # noqa: E731
            assert [int(x) for x in got[4 * w : 4 * w + 4]] == [bits((c < 4) & (c & 1 == 1)), bits((c < 4) & (c & 2 == 2)), bits(c < 4), bits(c != D.GAP)], (nb, w)


def test_counts_of_random_rows_word_by_word():
    rng = np.random.default_rng(4)
    for nb in (1, 2, 4, 5, 31, 32, 33):
        for _ in range(6):
            a, b = (rng.choice(6, 16 * nb, p=[0.22, 0.22, 0.22, 0.22, 0.04, 0.08]).astype(np.uint8) for _ in range(2))
            assert D.harness_counts(D.pack(a), D.pack(b)) == D.counts(a, b), nb


def test_padding_mask():
    h = D.harness()
    for L in (16, 32, 1, 17, 15, 31, 20, 65535):
        want = sum(1 << (48 + c) for c in range(L % 16, 16)) if L % 16 else 0
        assert int(h.kpy_dist_pad_mask(L)) == want == int(pad_masks([L])[0]), L
        codes = np.arange(L, dtype=np.uint8) % 4
        assert (D.unpack(D.gene_blocks(codes))[L:] == D.GAP).all() and int(D.gene_blocks(codes)[-1]) >> 48 == want >> 48


def test_listing_predicate_at_its_edges():
    h = D.harness()
    top = 2**31 - 1
    for comp, diff, md, mc, want in ((5, 3, 3, 5, 1), (5, 4, 3, 5, 0), (4, 3, 3, 5, 0), (5, 2, 3, 5, 1), (6, 3, 3, 5, 1), (0, 0, 0, 0, 1), (0, 0, 0, 1, 0),
                                     (0, 1, 0, 0, 0), (top, top, top, 0, 1), (0, 0, top, 0, 1), (10, 10, 10, 1, 1), (10, 11, 10, 1, 0)):  # fmt: skip
        assert h.kpy_dist_listed(comp, diff, md, mc) == want, (comp, diff, md, mc)
    codes = np.stack([D.codes_of("acgtacgtacgtacgt"), D.codes_of("acgtacgtacgtaaaa"), D.codes_of("acgtacgtacgt----")])  # 0-1: 16 / 3; 0-2: 12 / 0; 1-2: 12 / 0
    assert [tuple(p)[:4] for p in D.all_pairs(codes, 3, 12)] == [(0, 1, 16, 3), (0, 2, 12, 0), (1, 2, 12, 0)]
    assert [tuple(p)[:2] for p in D.all_pairs(codes, 2, 12)] == [(0, 2), (1, 2)] and [tuple(p)[:2] for p in D.all_pairs(codes, 3, 13)] == [(0, 1)]


def test_tiles_on_or_above_the_diagonal():
    h = D.harness()
    out = np.zeros(2, np.int32)
    for nt in (1, 2, 3, 7, 157, 1000):
        want = [(i, j) for i in range(nt) for j in range(i, nt)]
        assert h.kpy_dist_tiles(nt) == len(want)
        for t in (range(len(want)) if nt <= 157 else (0, 1, nt - 1, nt, len(want) // 2, len(want) - 2, len(want) - 1)):
            h.kpy_dist_tile_of(C.c_int64(t), C.c_int64(nt), _p(out))
            assert tuple(out) == want[t], (nt, t)
    nt = D.MAX_ROWS // D.TILE  # the largest grid: its last tiles, where the square root is least exact
    total = h.kpy_dist_tiles(nt)
    assert total == nt * (nt + 1) // 2 and total * 256 < 2**32  # a grid dimension holds fewer than 2^32 work items: 256 lanes a tile
    for t, want in ((total - 1, (nt - 1, nt - 1)), (total - 2, (nt - 2, nt - 1)), (total - 3, (nt - 2, nt - 2)), (nt - 1, (0, nt - 1)), (nt, (1, 1))):
        h.kpy_dist_tile_of(C.c_int64(t), C.c_int64(nt), _p(out))
        assert tuple(out) == want, t


# ---- the mirrors ---------------------------------------------------------------------------------------------------------------------------
def test_header_constants_and_their_mirrors():
    out = np.zeros(8, np.int32)
    D.harness().kpy_dist_layout(_p(out))
    assert out.tolist() == [24, D.TILE, D.CHUNK, D.WORD_BLOCKS, D.MAX_DIFF, D.MIN_COMPARED, D.MAX_ROWS, 4]
    assert (_native.DIST_TILE, _native.DIST_CHUNK, _native.DIST_MAX_DIFF, _native.DIST_MIN_COMPARED, _native.DIST_MAX_ROWS) == (D.TILE, D.CHUNK, D.MAX_DIFF, D.MIN_COMPARED, D.MAX_ROWS)
    text = (ROOT / "kaptive_amd" / "csrc" / "kp_dist.h").read_text()
    defs = {m[1]: int(m[2]) for m in re.finditer(r"#define (KP_DIST_\w+) (\d+)", text)}
    assert defs["KP_DIST_TILE"] == _native.DIST_TILE and defs["KP_DIST_CHUNK"] == _native.DIST_CHUNK
    spec = (ROOT / "include" / "kp_spec.h").read_text()
    assert re.search(r"#define KP_DIST_MAX_DIFF 10\b", spec) and re.search(r"#define KP_DIST_MIN_COMPARED 1\b", spec)
    body = re.search(r"typedef struct kp_dist_pair \{(.*?)\} kp_dist_pair;", spec, re.S)[1]
    fields = [f.strip() for decl in re.findall(r"int32_t ([^;]+);", body) for f in decl.split(",")]
    assert fields == ["a", "b", "compared", "differences", "unshared", "pad_"]
    assert [n.rstrip("_") for n in fields] == list(_native.DIST_PAIR_DTYPE.names) and _native.DIST_PAIR_DTYPE == D.PAIR_DTYPE and _native.DIST_PAIR_DTYPE.itemsize == 24
    assert _native.DISTANCES_HEADER == D.HEADER
    assert len(_native.REPORTS) == 5 and "distances" not in [r.name for r in _native.REPORTS]  # a layer beside the per-batch reports
    assert "kp_dist.hip" in __import__("kaptive_amd.build", fromlist=["SOURCES"]).SOURCES


# ---- LocusRows on hand-made tables --------------------------------------------------------------------------------------------------------
def _hand_db():
    """Two loci: L0 with genes of 16, 17 and 31 bases, L1 with one gene of 20."""
    return SimpleNamespace(genes=SimpleNamespace(lengths=np.array([16, 17, 31, 20], np.int32)), locus_gene_offsets=np.array([0, 3], np.int32),
                           locus_gene_lengths=np.array([3, 1], np.int32), loci=SimpleNamespace(ids=["L0", "L1"]))  # fmt: skip


def _hand_batch(db, seed, ids, plan, best):
    """A BatchTyping stand-in.  ``plan[a]``: (gene, flags) of every kept record of assembly a; every record gets a random row."""
    rng = np.random.default_rng(seed)
    stride = max([len(p) for p in plan] + [1]) + 1  # (one slot beyond the fullest list: it must be ignored)
    kept, rows, blocks = np.zeros((len(plan), stride), KEPT_DTYPE), np.zeros((len(plan), stride), _native.ALIGNED_ROW_DTYPE), [np.zeros(3, np.uint64)]
    off = 3
    sums = np.zeros(len(plan), SUMMARY_DTYPE)
    for a, recs in enumerate(plan):
        sums["n_kept"][a] = len(recs)
        for i, (gene, flags) in enumerate(recs):
            L = int(db.genes.lengths[gene])
            codes = rng.choice(6, L, p=[0.2, 0.2, 0.2, 0.2, 0.1, 0.1]).astype(np.uint8)
            b = D.pack(np.concatenate([codes, np.zeros(-L % 16, np.uint8)]))  # ALIGNED ROWS: the padding columns carry no bit
            kept[a, i]["gene"], kept[a, i]["flags"] = gene, flags
            rows[a, i] = (off, L, int((codes != D.GAP).sum()), 0, 0)
            blocks.append(b)
            off += len(b)
        kept[a, len(recs)]["gene"], kept[a, len(recs)]["flags"] = 0, D.F_PRIMARY  # beyond n_kept: not a record
        rows[a, len(recs)] = (0, 16, 0, 0, 0)
    blocks = np.concatenate(blocks)
    return SimpleNamespace(ids=list(ids), sums=sums, kept=kept, best_locus=np.array(best, np.int32), aligned=lambda: (rows, blocks), rows=rows, blocks=blocks)


P, S, E = D.F_PRIMARY | 1, D.F_SPURIOUS, 1
PLAN_1 = [[(0, P), (1, E), (2, E), (2, P), (3, P)],  # gene 1 has a fragment but no primary record; gene 2 a fragment before its primary one; gene 3's primary lies outside L0
          [(0, P), (1, P), (2, P), (3, S)],           # a spurious record
          [],                                         # an assembly without a hit, typed L1
          [(3, P), (0, P)]]                           # L1; gene 0's record belongs to another locus
PLAN_2 = [[(2, P)], [(3, E), (3, P)], [(0, P), (1, P), (2, P)]]


def _want_matrix(db, bt, locus):
    members = [a for a in range(len(bt.ids)) if int(bt.best_locus[a]) == locus]
    return members, np.stack([D.locus_row(db, locus, bt.sums["n_kept"][a], bt.kept[a], bt.rows[a], bt.blocks) for a in members])


def test_locus_rows_from_hand_made_tables():
    db = _hand_db()
    b1 = _hand_batch(db, 1, ["a0", "a1", "a2", "a3"], PLAN_1, [0, 0, 1, 1])
    b2 = _hand_batch(db, 2, ["b0", "b1", "b2"], PLAN_2, [0, 1, 0])
    lr = LocusRows(db)
    lr.add(b1)
    assert (lr.n_blocks(0), lr.n_blocks(1), lr.columns(0), lr.columns(1)) == (1 + 2 + 2, 2, 64, 20) and lr.loci() == [0, 1]
    for locus in (0, 1):
        members, want = _want_matrix(db, b1, locus)
        idx, mat = lr.locus_matrix(locus)
        assert idx.tolist() == members and mat.dtype == np.uint64 and D.unpack(mat).tolist() == want.tolist()
    idx, mat = lr.locus_matrix(0)
    codes = D.unpack(mat)
    assert (codes[0, 16:48] == D.GAP).all()  # gene 1 of a0: a fragment, no primary record -> all GAP
    assert (codes[:, 33:48] == D.GAP).all() and (codes[:, 79:80] == D.GAP).all()  # padding of the 17- and the 31-base gene
    assert (codes[1, 16:33] != D.GAP).any()
    assert (D.unpack(lr.locus_matrix(1)[1])[0] == D.GAP).all()  # the assembly without a hit
    lr.add(b2)
    assert lr.ids == ["a0", "a1", "a2", "a3", "b0", "b1", "b2"] and lr.best.tolist() == [0, 0, 1, 1, 0, 1, 0]
    idx, mat = lr.locus_matrix(0)
    m2, w2 = _want_matrix(db, b2, 0)
    assert idx.tolist() == [0, 1, 4, 6] and D.unpack(mat[2:]).tolist() == w2.tolist() and m2 == [0, 2]
    with pytest.raises(ValueError):
        bad = _hand_batch(db, 1, ["x"], [[(0, P)]], [0])
        bad.rows["gene_len"][0, 0] = 17
        LocusRows(db).add(bad)


def test_state_and_merge_round_trip():
    db = _hand_db()
    b1 = _hand_batch(db, 1, ["a0", "a1", "a2", "a3"], PLAN_1, [0, 0, 1, 1])
    b2 = _hand_batch(db, 2, ["b0", "b1", "b2"], PLAN_2, [0, 1, 0])
    whole = LocusRows(db)
    whole.add(b1)
    whole.add(b2)
    parts = []
    for b in (b1, b2):
        lr = LocusRows(db)
        lr.add(b)
        parts.append(pickle.loads(pickle.dumps(lr.state())))  # as it travels between processes
    merged = LocusRows(db)
    for s in parts:
        merged.merge(s)
    assert merged.ids == whole.ids and merged.best.tolist() == whole.best.tolist() and merged.loci() == whole.loci()
    for locus in whole.loci():
        (i1, m1), (i2, m2) = whole.locus_matrix(locus), merged.locus_matrix(locus)
        assert i1.tolist() == i2.tolist() and m1.tobytes() == m2.tobytes()
    again = LocusRows(db)
    again.merge(whole.state())
    assert again.state()["ids"] == whole.ids and all(again.locus_matrix(L)[1].tobytes() == whole.locus_matrix(L)[1].tobytes() for L in whole.loci())
    with pytest.raises(ValueError):
        bad = whole.state()
        bad["loci"][0] = (bad["loci"][0][0], bad["loci"][0][1][:, :-1])
        LocusRows(db).merge(bad)
    assert DIST_RECORD_DTYPE.names == ("locus", "a", "b", "compared", "differences", "unshared")


# ---- the formatter ---------------------------------------------------------------------------------------------------------------------------
def test_format_distances_byte_for_byte():
    names = ["iso_1", "", "a name with spaces", "é"]
    pairs = np.array([(0, 1, 25000, 0, 0, 0), (0, 3, 2**31 - 1, 2**31 - 1, 2**31 - 1, 0), (2, 3, 0, 0, 17, 0)], D.PAIR_DTYPE)
    assert _native.format_distances("KL107", 25123, names, pairs) == D.format_lines("KL107", 25123, names, pairs)
    assert _native.format_distances("KL107", 25123, names, pairs[:0]) == b"" == _native.format_distances("", 0, [], pairs[:0])
    many = np.zeros(5000, D.PAIR_DTYPE)  # more than the first buffer holds: the size-then-fill convention
    many["b"], many["compared"] = 2, np.arange(5000)
    assert _native.format_distances("L" * 300, 7, names, many) == D.format_lines("L" * 300, 7, names, many)
    for bad in ((0, 4, 1, 1, 1, 0), (-1, 2, 1, 1, 1, 0)):
        with pytest.raises(ValueError):
            _native.format_distances("x", 1, names, np.array([bad], D.PAIR_DTYPE))
    lib = _native.lib()
    lib.kp_format_distances.restype = C.c_int64
    off = np.array([0, 1, 2], np.int64)
    one = np.array([(0, 1, 1, 1, 1, 0)], D.PAIR_DTYPE)
    need = lib.kp_format_distances(b"x", C.c_int32(1), C.c_int64(3), b"ab", _p(off), C.c_int32(2), _p(one), C.c_int64(1), None, C.c_int64(0))
    assert need == len(b"x\ta\tb\t3\t1\t1\t1\n")  # the sizing call
    assert lib.kp_format_distances(b"x", C.c_int32(1), C.c_int64(3), b"ab", _p(off), C.c_int32(2), _p(one), C.c_int64(1), None, C.c_int64(8)) == -1
    assert lib.kp_format_distances(b"x", C.c_int32(1), C.c_int64(-3), b"ab", _p(off), C.c_int32(2), _p(one), C.c_int64(1), None, C.c_int64(0)) == -1
    assert lib.kp_format_distances(b"x", C.c_int32(1), C.c_int64(3), b"ab", None, C.c_int32(2), _p(one), C.c_int64(1), None, C.c_int64(0)) == -1


# ---- the command line's flags and the keyword ----------------------------------------------------------------------------------------------
def test_command_line_flags_and_keyword():
    from kaptive_amd.cli import build_parser
    from kaptive_amd.serotyping.core import MultiSerotyper, Serotyper
    from kaptive_amd.synth import make_db

    ap = build_parser()
    ns = ap.parse_args(["assembly", "db.npz", "a.fasta", "--distances", "d.tsv"])
    assert ns.distances == "d.tsv" and not hasattr(ns, "max_distance") and not hasattr(ns, "aligned")
    ns = ap.parse_args(["assembly", "db.npz", "a.fasta", "--distances", "d.tsv", "--max-distance", "0", "--min-compared", "100"])
    assert (ns.max_distance, ns.min_compared) == (0, 100)
    for bad in (["--max-distance", "3"], ["--min-compared", "3"], ["--distances", "d.tsv", "--max-distance", "-1"], ["--distances", "d.tsv", "--min-compared", str(2**31)]):
        with pytest.raises(SystemExit):
            ap.parse_args(["assembly", "db.npz", "a.fasta", *bad])
    db = make_db("kpsc_k", seed=7, n_loci=9)
    plain, typer = Serotyper(db), Serotyper(db, distances=True)
    assert plain.locus_rows is None and not plain._aligned and typer._aligned and isinstance(typer.locus_rows, LocusRows) and len(typer.locus_rows) == 0
    ms = MultiSerotyper([db, make_db("kpsc_o", seed=8)], distances=True)
    assert ms._aligned and all(isinstance(s.locus_rows, LocusRows) and s.locus_rows.db is s._db for s in ms.serotypers)
