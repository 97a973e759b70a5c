"""Aligned rows, the parts that need no GPU (include/kp_spec.h, ALIGNED ROWS): the known answers of the specification from the Python
restatement of tests/aligned_util.py and from kp_aligned.h built with g++ (tests/native_harness/aligned_harness.cpp); the header
against the restatement over random canonical op lists of 1 to 2000 ops on both strands, every residue modulo 16 of q_start, of the
contig position and of the gene length, N runs on both edges of a segment, I and D ops that start and end on block boundaries,
partial hits and each kind of invalid walk; kp_format_aligned against a Python formatter; the command line's flag."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.serotyping import batch as B
from kaptive_amd.serotyping.batch import KEPT_DTYPE
from tests import aligned_util as A

M, I, D = A.M, A.I, A.D
KNOWN_CONTIG = "ttacgtnacgga"
KNOWN_OPS = [A.op(M, 4), A.op(I, 2), A.op(M, 3), A.op(D, 1), A.op(M, 1)]
KNOWN = {1: ("--acgt--nacg--------", (0xF0C3010000900E40, 0x000F000000000000)), -1: ("--cgtn--acgt--------", (0xF0C3002000E40390, 0x000F000000000000))}


def codes_of(text: str) -> np.ndarray:
    return np.array([b"acgtn".index(c) for c in text.encode()], np.uint8)


def both(ops, pa, contig, Lq, strand, q_start, q_end, t_start, found=True, label=""):
    """The restatement and the header on one record: the packed rows and the counts must agree.  Returns (codes, counts, valid)."""
    c0 = int(pa.ctg_start[contig])
    row, covered, inserted, n_ins = A.row_from_ops(ops, pa.codes, Lq, strand, q_start, q_end, t_start, c0, c0 + int(pa.ctg_len[contig]), found)
    ok, blocks, counts = A.harness_row(ops, pa, contig, Lq, strand, q_start, q_end, t_start, found)
    want = A.pack_blocks(row)
    assert blocks.tolist() == want.tolist(), f"{label}: blocks differ, first at {np.flatnonzero(blocks != want)[:1]}"
    assert counts == (covered, inserted, n_ins), label
    assert A.unpack_blocks(blocks, Lq).tolist() == row.tolist()
    return row, counts, ok


def canonical_ops(rng, n_ops: int, max_len: int = 24):
    """A canonical op list of exactly n_ops ops (not 2): M first and last, no two neighbours of one kind, no length 0.  m M ops
    with a gap of one op (I or D) or of two (I D or D I) between neighbours."""
    assert n_ops >= 1 and n_ops != 2
    m = int(rng.integers((n_ops + 4) // 3, (n_ops + 1) // 2 + 1))  # 2 m - 1 <= n_ops <= 3 m - 2
    double = np.zeros(m - 1, bool)
    double[rng.permutation(m - 1)[: n_ops - (2 * m - 1)]] = True
    kinds = [M]
    for two in double:
        first = int(rng.choice((I, D)))
        kinds += [first, I + D - first, M] if two else [first, M]
    assert len(kinds) == n_ops and kinds[-1] == M and all(a != b for a, b in zip(kinds, kinds[1:]))
    lens = rng.integers(1, max_len + 1, size=n_ops)
    lens[rng.random(n_ops) < 0.05] = 16 * rng.integers(1, 4)  # whole blocks now and then
    return [A.op(k, int(n)) for k, n in zip(kinds, lens)]


def spans(ops):
    rows = sum(o >> 4 for o in ops if o & 15 != D)
    cols = sum(o >> 4 for o in ops if o & 15 != I)
    return rows, cols


def contig_for(rng, n: int, n_runs: int = 3):
    c = rng.integers(0, 4, size=n).astype(np.uint8)
    for _ in range(n_runs):
        s = int(rng.integers(0, max(n - 1, 1)))
        c[s : s + int(rng.integers(1, 40))] = 4
    return c


# ---- known answers ---------------------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_specification():
    pa = A.pack([codes_of("gattaca"), codes_of(KNOWN_CONTIG)])
    for strand, (want_text, want_blocks) in KNOWN.items():
        row, counts, ok = both(KNOWN_OPS, pa, 1, 20, strand, 2, 12, 2, label=f"strand {strand}")
        assert ok and A.text(row) == want_text.encode() and counts == (8, 1, 1)
        assert tuple(int(v) for v in A.pack_blocks(row)) == want_blocks
        assert tuple(int(v) for v in A.harness_row(KNOWN_OPS, pa, 1, 20, strand, 2, 12, 2)[1]) == want_blocks
    out = (C.c_int32 * 3)()
    A.harness().kpy_aln_layout(out)
    assert list(out) == [24, 16, 48] and _native.ALIGNED_ROW_DTYPE == A.ALIGNED_ROW_DTYPE and _native.ALIGNED_ROW_DTYPE.itemsize == 24
    assert _native.ALIGNED_GAP == A.GAP


def test_the_reverse_strand_is_the_forward_row_of_the_reverse_complemented_contig():
    rng = np.random.default_rng(3)
    ops = canonical_ops(rng, 41)
    rows, cols = spans(ops)
    contig = contig_for(rng, cols + 9)
    rc = np.where(contig[::-1] <= 3, 3 - contig[::-1], 4).astype(np.uint8)
    Lq = rows + 11
    fwd, cf, _ = both(ops, A.pack([contig]), 0, Lq, 1, 4, 4 + rows, 5)
    # the same path seen from the other strand: the ops back to front, the contig reverse-complemented
    rev, cr, _ = both(ops[::-1], A.pack([rc]), 0, Lq, -1, 4, 4 + rows, len(contig) - 5 - cols)
    assert fwd.tolist() == rev.tolist() and cf == cr


# ---- the header against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strand", (1, -1))
def test_random_canonical_op_lists(strand):
    rng = np.random.default_rng(100 + strand)
    sizes = [1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 511, 513, 1999, 2000] + [int(x) for x in rng.integers(4, 1500, size=10)]
    seen_gap_inside = seen_inserted = False
    for n_ops in sizes:
        if n_ops == 2:  # (M first and last, no equal neighbours: no canonical list has two ops)
            continue
        ops = canonical_ops(rng, n_ops)
        assert len(ops) == n_ops
        rows, cols = spans(ops)
        q_start, t_start = int(rng.integers(0, 50)), int(rng.integers(0, 50))
        Lq = q_start + rows + int(rng.integers(0, 50))
        pa = A.pack([contig_for(rng, 30), contig_for(rng, t_start + cols + int(rng.integers(0, 20)))], junk_rng=rng)
        row, counts, ok = both(ops, pa, 1, Lq, strand, q_start, q_start + rows, t_start, label=f"{n_ops} ops")
        assert ok and counts[0] == sum(o >> 4 for o in ops if o & 15 == M)
        assert (row[:q_start] == A.GAP).all() and (row[q_start + rows :] == A.GAP).all()
        seen_gap_inside |= bool((row[q_start : q_start + rows] == A.GAP).any())
        seen_inserted |= counts[1] > 0
    assert seen_gap_inside and seen_inserted


@pytest.mark.parametrize("strand", (1, -1))
def test_every_residue_of_q_start_contig_position_and_gene_length(strand):
    rng = np.random.default_rng(16 + strand)
    ops = [A.op(M, 37), A.op(I, 5), A.op(M, 16), A.op(D, 7), A.op(M, 1), A.op(I, 16), A.op(D, 2), A.op(M, 40)]
    rows, cols = spans(ops)
    contig = contig_for(rng, cols + 40)
    pa = A.pack([contig_for(rng, 5), contig], junk_rng=rng)
    n = 0
    for q_res in range(16):
        for t_res in range(16):
            for L_res in ((q_res + t_res) % 16, (q_res * 5 + 3) % 16):
                q_start = 16 + q_res
                Lq = q_start + rows + 16
                Lq += (L_res - Lq) % 16
                _, _, ok = both(ops, pa, 1, Lq, strand, q_start, q_start + rows, 16 + t_res, label=f"{q_res} {t_res} {L_res}")
                assert ok
                n += 1
    for L_res in range(16):  # every gene-length residue with the hit running to the gene's last base
        Lq = 16 * 9 + L_res
        if Lq >= rows:
            _, _, ok = both(ops, pa, 1, Lq, strand, Lq - rows, Lq, 3, label=f"ends on the last base, Lq {Lq}")
            assert ok
            n += 1
    assert n >= 16 * 16 * 2 + 8


@pytest.mark.parametrize("strand", (1, -1))
def test_n_runs_on_both_edges_of_a_segment(strand):
    rng = np.random.default_rng(77)
    ops = [A.op(M, 20), A.op(I, 3), A.op(M, 33), A.op(D, 4), A.op(M, 20)]
    rows, cols = spans(ops)
    t_start = 7
    seg2 = t_start + 20  # the second segment's first contig base; it ends before seg2 + 33, the D bases follow
    cases = {"first base of a segment": [(seg2, seg2 + 1)], "last base of a segment": [(seg2 + 32, seg2 + 33)], "across a segment's start": [(seg2 - 2, seg2 + 2)],
             "across a segment's end into the dropped bases": [(seg2 + 30, seg2 + 35)], "only the dropped bases": [(seg2 + 33, seg2 + 37)],
             "a whole segment": [(seg2, seg2 + 33)], "the hit's first and last base": [(t_start, t_start + 1), (t_start + cols - 1, t_start + cols)],
             "before and behind only": [(t_start - 3, t_start), (t_start + cols, t_start + cols + 3)], "all of it": [(0, t_start + cols + 5)]}  # fmt: skip
    base = rng.integers(0, 4, size=t_start + cols + 9).astype(np.uint8)
    plain, _, _ = both(ops, A.pack([base]), 0, rows + 5, strand, 2, 2 + rows, t_start)
    for q_off in (0, 9):
        for name, runs in cases.items():
            codes = base.copy()
            for a, z in runs:
                codes[a:z] = 4
            row, counts, ok = both(ops, A.pack([codes], junk_rng=rng), 0, rows + 5 + q_off, strand, 2 + q_off, 2 + q_off + rows, t_start, label=name)
            assert ok and counts == (rows - 3, 4, 1), "an N column is covered"
            n4 = int((row == 4).sum())
            if name in ("before and behind only", "only the dropped bases"):
                assert n4 == 0 and (q_off or row.tolist() == plain.tolist()), name
            else:
                assert n4 > 0, name
            if name == "all of it":
                assert n4 == rows - 3


@pytest.mark.parametrize("strand", (1, -1))
def test_gaps_that_start_and_end_on_block_boundaries(strand):
    rng = np.random.default_rng(5)
    ops = [A.op(M, 16), A.op(I, 16), A.op(M, 32), A.op(D, 16), A.op(M, 16), A.op(I, 48), A.op(M, 16)]
    rows, cols = spans(ops)
    pa = A.pack([contig_for(rng, cols + 32, n_runs=0)])
    for q_start, Lq in ((0, rows), (16, rows + 32), (0, rows + 1), (32, rows + 32)):
        row, counts, ok = both(ops, pa, 0, Lq, strand, q_start, q_start + rows, 16, label=f"{q_start} {Lq}")
        assert ok and counts == (80, 16, 1)
        blocks = A.pack_blocks(row)
        whole_gap = [int(v) == 0xFFFF << 48 for v in blocks]
        if not (strand < 0 and Lq % 16):  # (for strand -1 the walk starts at Lq - q_end: on a block boundary when Lq is)
            assert sum(whole_gap) >= 4, "the I ops are whole blocks of GAP"


def test_partial_hits_and_a_hit_of_one_base():
    rng = np.random.default_rng(8)
    pa = A.pack([contig_for(rng, 300)])
    for strand in (1, -1):
        for q_start, q_end, Lq in ((0, 100, 1000), (900, 1000, 1000), (450, 550, 1000), (7, 8, 9), (0, 1, 1), (15, 16, 16), (16, 17, 17)):
            n = q_end - q_start
            row, counts, ok = both([A.op(M, n)], pa, 0, Lq, strand, q_start, q_end, 300 - n, label=f"{q_start}-{q_end} of {Lq}")
            assert ok and counts == (n, 0, 0) and int((row != A.GAP).sum()) == n


def test_every_kind_of_invalid_walk_gives_the_all_gap_row():
    rng = np.random.default_rng(9)
    pa = A.pack([contig_for(rng, 40), contig_for(rng, 200)])
    ops = [A.op(M, 50), A.op(D, 3), A.op(M, 47)]  # 97 rows, 100 columns
    good = dict(Lq=120, strand=1, q_start=10, q_end=107, t_start=100)
    _, counts, ok = both(ops, pa, 1, **good)
    assert ok and counts == (97, 3, 1)  # (it ends on the contig's last base)
    bad = {"the hit is not found": dict(found=False), "the contig ends before the ops do": dict(t_start=101), "a negative contig position": dict(t_start=-1),
           "the gene ends before the ops do": dict(Lq=106), "a negative row": dict(q_start=-1), "strand -1: the walk's first row is negative": dict(strand=-1, q_end=121),
           "strand -1: the gene ends before the ops do": dict(strand=-1, q_end=96), "a gene without a base": dict(Lq=0)}  # fmt: skip
    for name, change in bad.items():
        args = {**good, **change}
        found = args.pop("found", True)
        row, counts, ok = both(ops, pa, 1, found=found, label=name, **args)
        assert not ok and counts == (0, 0, 0) and (row == A.GAP).all(), name
    # an op of an unknown kind moves nothing, but the check counts its length on both sides, as the variant walk's does
    _, counts, ok = both([A.op(M, 5), A.op(4, 100), A.op(M, 5)], pa, 1, 300, 1, 0, 110, 91)
    assert not ok and counts == (0, 0, 0)
    _, counts, ok = both([A.op(M, 5), A.op(4, 100), A.op(M, 5)], pa, 1, 300, 1, 0, 110, 90)
    assert ok and counts == (10, 0, 0)
    # lengths whose sum passes 32 bits are an invalid walk, not a crash
    _, counts, ok = both([A.op(M, (1 << 28) - 1)] * 40, pa, 1, 120, 1, 0, 100, 0)
    assert not ok and counts == (0, 0, 0)


# ---- kp_format_aligned -----------------------------------------------------------------------------------------------------------------
def _table():
    """Three assemblies: none, five records (one spurious, both strands, an all-GAP row, a gene of 16 and one of 33 bases), two."""
    rng = np.random.default_rng(12)
    stride = 6
    kept, rows = np.zeros((3, stride), KEPT_DTYPE), np.zeros((3, stride), A.ALIGNED_ROW_DTYPE)
    lens = [16, 33, 1, 250, 40]
    blocks, off = [], 0
    spec = [(0, 0, 1, 0), (1, 1, -1, 0), (2, 0, 1, A.F_SPURIOUS), (3, 1, -1, 0), (4, 0, 1, 0)]
    for i, ((g, c, st, fl), L) in enumerate(zip(spec, lens)):
        codes = rng.integers(0, 6, size=L).astype(np.uint8) if i != 3 else np.full(L, A.GAP, np.uint8)
        k = kept[1, i]
        k["gene"], k["contig"], k["strand"], k["flags"], k["t_start"], k["t_end"], k["q_start"], k["q_end"] = g, c, st, fl, 100 * i, 100 * i + L, i, L
        rows[1, i] = (off, L, int((codes != A.GAP).sum()), i, i // 2)
        b = A.pack_blocks(codes)
        blocks.append(b)
        off += len(b)
    kept[2, :2], rows[2, :2] = kept[1, :2], rows[1, :2]
    return kept, rows, np.concatenate(blocks), np.array([0, 5, 2], np.int32)


def test_formatter_against_the_python_formatter():
    kept, rows, blocks, n_kept = _table()
    genes, asm_names, contigs = [f"gene{i}" for i in range(5)], ["empty", "asm two", "three"], [["x"], ["c1", "contig two"], ["a", "b"]]
    flat, first = [c for cs in contigs for c in cs], [0, 1, 3, 5]
    want = A.format_tsv(asm_names, contigs, genes, n_kept, kept, rows, blocks)
    args = (genes, asm_names, flat, first, n_kept, kept, rows, blocks)
    got = _native.format_aligned(*args)
    assert got == want and got.count(b"\n") == 4 + 2
    lines = [ln.split(b"\t") for ln in got.splitlines()]
    assert all(len(ln) == 13 for ln in lines) and _native.ALIGNED_HEADER == A.HEADER and A.HEADER.count(b"\t") == 12
    for ln in lines:
        assert len(ln[12]) == int(ln[6]) and int(ln[9]) == len(ln[12].replace(b"-", b"")) and set(ln[12]) <= set(b"acgtn-")
    assert lines[0][:9] == [b"asm two", b"gene0", b"c1", b"1", b"16", b"+", b"16", b"1", b"16"]
    assert lines[1][:9] == [b"asm two", b"gene1", b"contig two", b"101", b"133", b"-", b"33", b"2", b"33"] and lines[1][10:12] == [b"1", b"0"]
    assert lines[2][1] == b"gene3" and lines[2][12] == b"-" * 250 and b"gene2" not in {ln[1] for ln in lines}, "a spurious record leaves the table"
    # the size-only call, an exact buffer and one that is a byte short
    h = _native.lib()
    h.kp_format_aligned.restype = C.c_int64
    gn_b, gn_o = _native._blob(genes)
    an_b, an_o = _native._blob64(asm_names)
    cn_b, cn_o = _native._blob64(flat)
    f64 = np.array(first, np.int64)
    p = _native._p
    t = _native.VariantTables(gene_names=p(gn_b).value, gene_name_off=p(gn_o).value, n_genes=5, asm_names=p(an_b).value, asm_name_off=p(an_o).value,
                              ctg_names=p(cn_b).value, ctg_name_off=p(cn_o).value, asm_first_ctg=p(f64).value)  # fmt: skip

    def call(out, cap, rows_=rows, n_blocks=len(blocks)):
        return h.kp_format_aligned(C.byref(t), C.c_int32(3), p(n_kept), p(kept), C.c_int32(6), p(rows_), p(blocks), C.c_int64(n_blocks),
                                   p(out) if out is not None else None, C.c_int64(cap))  # fmt: skip

    assert call(None, 0) == len(want)
    exact = np.zeros(len(want) + 8, np.uint8)
    exact[:] = 0x23
    assert call(exact, len(want)) == len(want) and exact[: len(want)].tobytes() == want and (exact[len(want) :] == 0x23).all()
    short = np.full(len(want) + 8, 0x23, np.uint8)
    assert call(short, len(want) - 1) == len(want) and (short[len(want) - 1 :] == 0x23).all()
    # refusals: a row whose off or gene_len runs outside the blocks, counts beyond the stride, unknown genes and contigs
    for field, value in (("off", len(blocks)), ("off", -1), ("off", len(blocks) - 1), ("gene_len", -1), ("gene_len", 16 * len(blocks) + 1)):
        r2 = rows.copy()
        r2[1, 1][field] = value
        assert call(None, 0, rows_=r2) == -1, (field, value)
    assert call(None, 0, n_blocks=len(blocks) - 1) == -1 and call(None, 0, n_blocks=-1) == -1

    def bad(i, change):
        a = [np.array(x).copy() if isinstance(x, np.ndarray) else x for x in args]
        change(a[i])
        with pytest.raises(ValueError):
            _native.format_aligned(*a)

    bad(4, lambda n: n.__setitem__(1, 7))
    bad(4, lambda n: n.__setitem__(1, -1))
    bad(5, lambda k: k["gene"].__setitem__((1, 3), 5))
    bad(5, lambda k: k["gene"].__setitem__((1, 3), -1))
    bad(5, lambda k: k["contig"].__setitem__((1, 3), 2))
    r2 = rows.copy()
    r2[1, 2]["off"] = 1 << 40  # (a spurious record's row is not read)
    assert _native.format_aligned(*args[:6], r2, blocks) == want
    with pytest.raises(ValueError):
        _native.format_aligned(*args[:6], rows[:, :-1], blocks)
    assert _native.format_aligned(genes, [], [], [0], [], kept[:0], rows[:0], blocks[:0]) == b""


def test_codes_of_a_row():
    kept, rows, blocks, _ = _table()
    for i in range(5):
        L = int(rows[1, i]["gene_len"])
        got = _native.aligned_codes(rows[1, i], blocks)
        assert got.dtype == np.uint8 and got.tolist() == A.unpack_blocks(blocks[int(rows[1, i]["off"]) :], L).tolist()
    r = rows[1, 4].copy()
    r["off"] = len(blocks)
    with pytest.raises(ValueError):
        _native.aligned_codes(r, blocks)


# ---- the command line and the library's refusal ----------------------------------------------------------------------------------------------
def test_flag_is_absent_from_the_namespace_unless_given():
    from kaptive_amd.cli import build_parser

    plain = build_parser().parse_args(["assembly", "db.npz", "a.fasta"])
    assert not hasattr(plain, "aligned")
    given = build_parser().parse_args(["assembly", "db.npz", "a.fasta", "--aligned", "rows.tsv"])
    assert given.aligned == "rows.tsv"
    assert not any(hasattr(given, f) for f in ("variants", "breakpoints", "alleles", "paf"))
    with pytest.raises(SystemExit):
        build_parser().parse_args(["assembly", "db.npz", "a.fasta", "--aligned"])


def test_with_several_databases_the_table_needs_a_file_name(tmp_path):
    from kaptive_amd.cli import build_parser, run_type

    fasta = tmp_path / "a.fasta"
    fasta.write_bytes(b">c\nACGT\n")
    args = build_parser().parse_args(["assembly", str(tmp_path / "db.npz"), str(fasta), "--db", str(tmp_path / "o.npz"), "--aligned", "-"])
    with pytest.raises(ValueError, match="--aligned with --db"):
        run_type(args)


def test_a_batch_typed_without_the_option_names_it():
    bt = B.BatchTyping.__new__(B.BatchTyping)
    bt._aligned = None
    for call in (bt.aligned, bt.aligned_tsv, lambda: bt.aligned_codes(0, 0)):
        with pytest.raises(ValueError, match="aligned=True"):
            call()
