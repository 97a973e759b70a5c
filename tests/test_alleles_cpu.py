"""Allele digests, the parts that need no GPU (include/kp_spec.h, ALLELES): the known answers of the specification from the numpy
restatement of tests/alleles_util.py and from kp_alleles.h -- the functions the device kernel gives a lane per block -- built with g++
(tests/native_harness/alleles_harness.cpp); the header against the restatement over every start offset inside a packed word, both
strands, lengths around one block, two blocks and one sweep of a wave, and N runs on every edge; kp_format_alleles against a Python
formatter; the command line's flag."""

from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.serotyping import batch as B
from kaptive_amd.serotyping.batch import KEPT_DTYPE, PIECE_DTYPE
from tests import alleles_util as A

NT_KNOWN = (("", 0x332E6D2B1A14193E), ("a", 0xC8754B03323395A8), ("aa", 0x0AFCEF52C019382F), ("acgt", 0x5EECCFC7D63EED1E),
            ("acgt" * 4, 0x06B0D6973A4C5FD8), ("acgt" * 4 + "a", 0x57CB97575F7AD496), ("acgtnacgt", 0x90DD01A6934EA7E4),
            ("n" * 17, 0xF06F6C1F40429398))  # fmt: skip
AA_KNOWN = ((b"", 0xB5A8304702ECFCEF), (b"M", 0x137859F1719B82AD), (b"MKLV*", 0x7103B19B365B9924), (b"MKLVAAAA", 0x329E08CCFFB44565),
            (b"MKLVAAAAW", 0x973B1FF3DAD4BCAC))  # fmt: skip
LOCUS_KNOWN = (("acgt", "tgca"), 0xEEF6D079D9303A4A)
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025)


def pack(contigs, junk_rng=None):
    """One assembly from code arrays (0..3, 4 = N): contigs start on word edges, the words end with the last contig's last word, N
    runs are listed in the padded space.  ``junk_rng``: the two bits under an N are random (a digest must not read them)."""
    starts, at = [], 0
    for c in contigs:
        starts.append(at)
        at += (len(c) + 15) // 16 * 16
    codes = np.zeros(at, np.uint8)
    for s, c in zip(starts, contigs):
        codes[s : s + len(c)] = c
    is_n = np.concatenate([[0], (codes == 4).astype(np.int8), [0]])
    edges = np.flatnonzero(np.diff(is_n))
    bits = np.where(codes == 4, junk_rng.integers(0, 4, size=at) if junk_rng is not None else 0, codes).astype(np.uint32)
    words = (bits.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint32)
    return SimpleNamespace(words=words, n_runs=edges.astype(np.int32).reshape(-1, 2), ctg_start=np.array(starts, np.int32),
                           ctg_len=np.array([len(c) for c in contigs], np.int32), codes=codes)  # fmt: skip


def revcomp(codes):
    c = np.asarray(codes, np.uint8)[::-1]
    return np.where(c <= 3, 3 - c, 4).astype(np.uint8)


def want_nt(pa, contig, start, end, strand) -> int:
    c0 = int(pa.ctg_start[contig])
    return A.nt_digest(A.interval_codes(pa.codes, c0 + start, c0 + end, strand))


# ---- known answers ---------------------------------------------------------------------------------------------------------------------
def test_known_answers_from_the_restatement():
    for text, want in NT_KNOWN:
        assert A.nt_digest(A.text_codes(text)) == want, text
    for prot, want in AA_KNOWN:
        assert A.aa_digest(prot) == want, prot
    pieces = [A.nt_digest(A.text_codes(t)) for t in LOCUS_KNOWN[0]]
    assert A.locus_digest(pieces, [0, 1]) == LOCUS_KNOWN[1] and A.locus_digest(pieces, []) == 0
    assert A.locus_digest(pieces, [1, 0]) != LOCUS_KNOWN[1], "the order of the pieces counts"


def test_known_answers_from_the_header():
    for text, want in NT_KNOWN:
        pa = pack([A.text_codes("gattaca"), A.text_codes(text)])
        for lanes in (0, 1, 64):
            assert A.harness_nt(pa, 1, 0, len(text), 1, lanes) == want, (text, lanes)
    for prot, want in AA_KNOWN:
        assert A.harness_aa(prot) == want, prot
    pieces = [A.nt_digest(A.text_codes(t)) for t in LOCUS_KNOWN[0]]
    assert A.harness_locus(pieces, [0, 1]) == LOCUS_KNOWN[1] and A.harness_locus(pieces, []) == 0
    assert A.harness_locus(pieces[::-1], [1, 0]) == LOCUS_KNOWN[1]
    for z in (0, 1, 0xDEADBEEF, A.M64):
        assert int(A.harness().kpy_al_mix(C.c_uint64(z))) == A.mix1(z) == int(A.mix(np.array([z], np.uint64))[0])
    out = (C.c_int32 * 2)()
    A.harness().kpy_al_layout(out)
    assert list(out) == [16, 16] and _native.ALLELE_DTYPE == A.ALLELE_DTYPE and _native.ALLELE_DTYPE.itemsize == 16


def test_every_single_base_substitution_has_a_digest_of_its_own():
    rng = np.random.default_rng(1200)
    gene = rng.integers(0, 4, size=1200).astype(np.uint8)
    seen = {A.nt_digest(gene)}
    for at in range(1200):
        for d in (1, 2, 3):
            alt = gene.copy()
            alt[at] = (alt[at] + d) & 3
            seen.add(A.nt_digest(alt))
    assert len(seen) == 3601


# ---- the header against the restatement: interval shapes -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain():
    rng = np.random.default_rng(4242)
    return pack([rng.integers(0, 4, size=37).astype(np.uint8), rng.integers(0, 4, size=2400).astype(np.uint8)])


@pytest.mark.parametrize("strand", (1, -1))
def test_every_start_offset_and_length(plain, strand):
    rng = np.random.default_rng(7 + strand)
    lengths = LENGTHS + tuple(int(x) for x in rng.integers(34, 2300, size=4))
    n = 0
    for off in range(16):
        for L in lengths:
            start = off + 16 * int(rng.integers(0, 3))
            want = want_nt(plain, 1, start, start + L, strand)
            assert A.harness_nt(plain, 1, start, start + L, strand) == want, (off, L)
            if L in (1, 17, 1025) or L > 1025:
                for lanes in (64, 7):  # the blocks dealt out as the kernel deals them
                    assert A.harness_nt(plain, 1, start, start + L, strand, lanes) == want, (off, L, lanes)
            n += 1
    assert n == 16 * 15
    # ... and an interval outside the contig has no digest
    assert A.harness_nt(plain, 1, -1, 5, strand) == 0 and A.harness_nt(plain, 1, 5, 2401, strand) == 0 and A.harness_nt(plain, 1, 9, 8, strand) == 0


def test_strand_minus_is_the_reverse_complement(plain):
    fwd = plain.codes[int(plain.ctg_start[1]) :][:2400]
    rc = pack([np.zeros(5, np.uint8), revcomp(fwd)])
    for start, end in ((0, 2400), (3, 20), (17, 1041), (1000, 1001), (1375, 2400)):
        d = A.harness_nt(plain, 1, start, end, -1)
        assert d == A.harness_nt(rc, 1, 2400 - end, 2400 - start, 1) == A.nt_digest(revcomp(fwd[start:end]))
        assert d != A.harness_nt(plain, 1, start, end, 1)


def _n_cases(s, e):
    """N runs (contig coordinates) against the interval [s, e): on its first and last base, on a block edge, one base long, a whole
    block, across both ends."""
    return {"starts on the first base": [(s, s + 3)], "ends on the first base": [(s - 3, s + 1)], "starts on the last base": [(e - 1, e + 2)],
            "ends on the last base": [(e - 4, e)], "across a block edge": [(s + 15, s + 17)], "ends on a block edge": [(s + 9, s + 16)],
            "starts on a block edge": [(s + 16, s + 19)], "one base": [(s + 5, s + 6)], "a whole block": [(s + 16, s + 32)],
            "twenty across an edge": [(s + 28, s + 48)], "all of it": [(s - 2, e + 2)], "before and behind only": [(s - 4, s), (e, e + 4)],
            "several": [(s + 1, s + 2), (s + 30, s + 34), (e - 2, e - 1)]}  # fmt: skip


@pytest.mark.parametrize("strand", (1, -1))
def test_n_runs_on_every_edge(strand):
    rng = np.random.default_rng(99)
    base = rng.integers(0, 4, size=1400).astype(np.uint8)
    n = 0
    for off in (0, 1, 7, 15):
        for L in (33, 64, 1025):
            s, e = 16 + off, 16 + off + L
            for name, runs in _n_cases(s, e).items():
                codes = base.copy()
                for a, z in runs:
                    codes[a:z] = 4
                pa = pack([A.text_codes("acgtn"), codes], junk_rng=rng)
                want = want_nt(pa, 1, s, e, strand)
                for lanes in (0, 64):
                    assert A.harness_nt(pa, 1, s, e, strand, lanes) == want, (name, off, L, lanes)
                if name == "before and behind only":
                    assert want == A.nt_digest(A.interval_codes(base, s, e, strand)), "runs that only touch the interval change nothing"
                else:
                    assert want != A.nt_digest(A.interval_codes(base, s, e, strand)), name
                n += 1
    assert n == 4 * 3 * 13


def test_an_interval_ending_on_the_last_base_of_the_last_word():
    rng = np.random.default_rng(5)
    for clen in (16, 32, 1024 + 16):
        pa = pack([rng.integers(0, 4, size=20).astype(np.uint8), rng.integers(0, 4, size=clen).astype(np.uint8)])
        assert len(pa.words) * 16 == int(pa.ctg_start[1]) + clen, "the contig ends with the assembly's last word"
        for strand in (1, -1):
            for start in (0, 1, clen - 16, clen - 15, clen - 1):
                assert A.harness_nt(pa, 1, start, clen, strand) == want_nt(pa, 1, start, clen, strand)
                assert A.harness_nt(pa, 1, start, clen, strand, 64) == want_nt(pa, 1, start, clen, strand)


def test_the_real_packer_agrees():
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from tests import cigar_util as U

    rng = np.random.default_rng(31)
    seqs = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].copy() for n in (50, 1301)]
    seqs[1][100:120] = ord("N")
    seqs[1][700] = ord("N")
    pa = GenomeAssembly("g", Sequences.from_records([SeqRecord(f"c{i}", s.tobytes()) for i, s in enumerate(seqs)])).packed()
    codes = U.assembly_codes(pa)
    for strand in (1, -1):
        for start, end in ((0, 1301), (95, 125), (101, 119), (699, 701), (3, 1028)):
            c0 = int(pa.ctg_start[1])
            want = A.nt_digest(A.interval_codes(codes, c0 + start, c0 + end, strand))
            text = seqs[1][start:end].tobytes()
            assert want == A.nt_digest(A.text_codes(text) if strand > 0 else revcomp(A.text_codes(text)))
            assert A.harness_nt(pa, 1, start, end, strand) == want


def test_protein_lengths():
    rng = np.random.default_rng(8)
    for n in (0, 1, 7, 8, 9, 4097):
        prot = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY*X", np.uint8)[rng.integers(0, 22, size=n)].tobytes()
        assert A.harness_aa(prot) == A.aa_digest(prot), n
        if n:
            assert A.aa_digest(prot) != A.aa_digest(prot[:-1]) and A.aa_digest(prot) != A.aa_digest(prot + b"\0"), "the length counts"


# ---- kp_format_alleles -----------------------------------------------------------------------------------------------------------------
def _formatter_table():
    """Three assemblies: one without a kept record, one with every Set value, a spurious record, a record without a protein and two
    pieces whose order differs from their index order, one without a piece."""
    rows = [(0, 0, 1, 0, 300), (1, 0, -1, 400, 1000), (2, 1, 1, 5, 905), (3, 1, -1, 1000, 1100), (4, 0, 1, 2000, 2600), (5, 1, 1, 3000, 3001),
            (6, 0, -1, 4000, 4100), (7, 1, 1, 0, 16)]  # fmt: skip
    flags = [A.F_EXPECTED | A.F_INSIDE | 32, A.F_EXPECTED, A.F_INSIDE, 0, A.F_EXTRA | A.F_INSIDE, A.F_EXTRA, A.F_INSIDE | A.F_SPURIOUS, A.F_EXPECTED | A.F_INSIDE | 8]
    states = [0, 1, 2, 3, 0, 0, 3, 1]
    prot = [(0, 100), (100, 200), (300, 0), (300, 33), (333, 200), (533, 1), (534, 30), (564, 5)]
    stride = len(rows) + 2
    kept = np.zeros((3, stride), KEPT_DTYPE)
    kept[1, : len(rows)] = A.kept_rows(rows, flags, states, prot)
    kept[2, :2] = A.kept_rows(rows[:2], flags[:2], states[:2], prot[:2])
    rng = np.random.default_rng(11)
    alleles = np.zeros((3, stride), A.ALLELE_DTYPE)
    alleles["nt"] = rng.integers(0, 1 << 63, size=(3, stride), dtype=np.uint64) * 2 + 1
    alleles["aa"] = rng.integers(0, 1 << 63, size=(3, stride), dtype=np.uint64)
    alleles["aa"][1, 2] = 0
    alleles["nt"][1, 0] = 0x00000000000000AB  # leading zeros are printed
    pieces = np.zeros((3, 3), PIECE_DTYPE)
    pieces["mean_pos"][1, :2] = (7.5, 2.25)
    piece_digests = rng.integers(0, 1 << 63, size=(3, 3), dtype=np.uint64)
    return kept, alleles, pieces, piece_digests, np.array([0, len(rows), 2], np.int32), np.array([0, 2, 0], np.int32), np.array([3, 1, 0], np.int32)


def test_formatter_against_the_python_formatter():
    kept, alleles, pieces, piece_digests, n_kept, n_pieces, best = _formatter_table()
    genes, loci = [f"gene{i}" for i in range(8)], ["KL1", "KL 2", "KL3", "KL4"]
    asm_names, contigs = ["empty", "asm two", "three"], [["x"], ["c1", "contig two"], ["a", "b"]]
    flat, first = [c for cs in contigs for c in cs], [0, 1, 3, 5]
    order = _native.piece_order(pieces, n_pieces)
    assert order[1].tolist() == [1, 0, 2] and order[0].tolist() == [0, 1, 2]
    want = A.format_tsv(asm_names, contigs, genes, loci, best, n_kept, kept, alleles, n_pieces, pieces, piece_digests)
    args = (genes, loci, asm_names, flat, first, n_kept, n_pieces, best, kept, alleles, piece_digests, order)
    got = _native.format_alleles(*args)
    assert got == want and got.count(b"\n") == 7 + 2
    lines = [ln.split(b"\t") for ln in got.splitlines()]
    assert all(len(ln) == 14 for ln in lines) and _native.ALLELES_HEADER == A.HEADER and A.HEADER.count(b"\t") == 13
    assert [ln[4] for ln in lines[:7]] == [b"expected_in", b"expected_out", b"other_in", b"other_out", b"extra_in", b"extra_out", b"expected_in"]
    assert [ln[9] for ln in lines[:7]] == [b"normal", b"partial", b"truncated", b"below_id_threshold", b"normal", b"normal", b"partial"]
    assert b"gene6" not in {ln[3] for ln in lines}, "a spurious record leaves the table"
    locus = A.locus_digest(piece_digests[1], [1, 0])
    assert lines[0] == [b"asm two", b"KL 2", b"%016x" % locus, b"gene0", b"expected_in", b"c1", b"1", b"300", b"+", b"normal", b"300",
                        b"00000000000000ab", b"100", b"%016x" % int(alleles["aa"][1, 0])]  # fmt: skip
    assert lines[1][5:9] == [b"c1", b"401", b"1000", b"-"] and lines[2][12:] == [b"0", b"."] and lines[2][5] == b"contig two"
    assert lines[7][:3] == [b"three", b"KL1", b"."], "an assembly without a piece has no locus allele"
    assert int(_native.locus_alleles(piece_digests, order, n_pieces)[1]) == locus == A.harness_locus(piece_digests[1], order[1, :2])
    assert _native.locus_alleles(piece_digests, order, n_pieces).tolist() == [0, locus, 0]
    # counts beyond the strides, and records that name a locus, gene, contig, piece or state the tables do not have, are refused
    def bad(i, value, field=None):
        a = [np.array(x).copy() if isinstance(x, np.ndarray) else x for x in args]
        if field is None:
            a[i][1] = value
        else:
            a[i][field][1, 3] = value
        with pytest.raises(ValueError):
            _native.format_alleles(*a)

    bad(5, kept.shape[1] + 1)  # n_kept
    bad(5, -1)
    bad(6, 4)  # n_pieces
    bad(7, 4)  # best locus
    bad(7, -1)
    bad(8, 8, "gene")
    bad(8, -1, "gene")
    bad(8, 2, "contig")
    bad(8, 4, "state")
    a = list(args)
    a[11] = order.copy()
    a[11][1, 0] = 2  # an order entry beyond the assembly's two pieces
    with pytest.raises(ValueError):
        _native.format_alleles(*a)
    with pytest.raises(ValueError):
        _native.format_alleles(*args[:9], alleles[:, :-1], *args[10:])
    assert _native.format_alleles(genes, loci, [], [], [0], [], [], [], kept[:0], alleles[:0], piece_digests[:0], order[:0]) == b""


# ---- the command line and the library's refusal ----------------------------------------------------------------------------------------------
def test_flag_is_absent_from_the_namespace_unless_given():
    from kaptive_amd.cli import build_parser

    plain = build_parser().parse_args(["assembly", "db.npz", "a.fasta"])
    assert not hasattr(plain, "alleles")
    given = build_parser().parse_args(["assembly", "db.npz", "a.fasta", "--alleles", "al.tsv"])
    assert given.alleles == "al.tsv" and not hasattr(given, "variants") and not hasattr(given, "breakpoints") and not hasattr(given, "paf")


def test_a_batch_typed_without_the_option_names_it():
    bt = B.BatchTyping.__new__(B.BatchTyping)
    bt._alleles = None
    for call in (bt.alleles, bt.locus_alleles, bt.alleles_tsv):
        with pytest.raises(ValueError, match="alleles=True"):
            call()
