"""Rescue records of the missing genes, the parts that need no GPU (include/kp_spec.h, RESCUE): kp_rescue.h -- the geometry and the
residue reader the device kernels call, built with g++ (tests/native_harness/rescue_harness.cpp) -- against the yardstick of
tests/rescue_util.py (``oracle.extract`` + ``oracle.translate``) over every offset inside a packed word, both strands, three frames,
window lengths of every residue class modulo 3, windows clipped at either contig end, one ending on the assembly's last base and N
runs across codon and word edges; kp_format_rescue against the Python formatter for every call and every edge value; the
preconditions of the GPU cases from the oracle's own pipeline; the command line's flags."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.serotyping import batch as B
from tests import rescue_util as R


def _genome(name, contigs):
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences

    return GenomeAssembly(name, Sequences.from_records([SeqRecord(f"{name}_{i}", np.ascontiguousarray(c).tobytes()) for i, c in enumerate(contigs)]))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the header against the yardstick --------------------------------------------------------------------------------------------------
def test_layout_and_constants():
    out = np.zeros(8, np.int32)
    R.harness().kpy_rs_layout(_p(out))
    assert out.tolist() == [56, 6, *R.STRIP_LIMITS, R.FLANK, R.MIN_SCORE, R.FLANK_MAX]
    assert _native.RESCUE_DTYPE == R.RESCUE_DTYPE and _native.RESCUE_DTYPE.itemsize == 56 and _native.RESCUE_HEADER == R.HEADER
    assert (_native.RESCUE_FLANK, _native.RESCUE_MIN_SCORE) == (R.FLANK, R.MIN_SCORE)
    for piece in (0, 1, 7):
        for strand in (1, -1):
            for f in range(3):
                assert R.harness().kpy_rs_task(piece, strand, f) == (piece * 2 + (strand < 0)) * 3 + f


def test_windows_and_frame_lengths():
    out = np.zeros(5, np.int32)
    for start, end, clen, flank in ((100, 200, 1000, 50), (10, 20, 1000, 50), (900, 990, 1000, 50), (0, 1000, 1000, 4096), (5, 5, 9, 0), (5, 6, 9, 0),
                                    (5, 7, 9, 0), (5, 8, 9, 0), (5, 9, 9, 0), (0, 5, 5, 0), (3, 3, 1000, 65535)):  # fmt: skip
        assert R.harness().kpy_rs_window(start, end, clen, flank, _p(out)) == 1
        ws, we = R.window(start, end, clen, flank)
        assert out.tolist() == [ws, we, *(max(0, (we - ws - f) // 3) for f in range(3))], (start, end, clen, flank)
    for bad in ((-1, 5, 10, 0), (6, 5, 10, 0), (0, 11, 10, 0)):  # a piece outside its contig: no window
        assert R.harness().kpy_rs_window(*bad, _p(out)) == 0 and out.tolist() == [0] * 5


def test_frame_texts_at_every_word_offset_strand_and_frame():
    from kaptive_amd.synth import random_dna

    rng = np.random.default_rng(5)
    first = random_dna(rng, 523, 0.5)
    first[40:43] = ord("N")     # inside one codon of some frame, across two in the others
    first[94:98] = ord("N")     # across the edge of a packed word (96)
    first[200] = ord("N")
    last = random_dna(rng, 16 * 9, 0.5)  # ends on a word edge: its last word is the assembly's last
    last[-1] = ord("G")
    odd = random_dna(rng, 77, 0.5)       # ... and one that ends inside a word, as the assembly's last contig
    for contigs in ([first, last], [last, first, odd]):
        g = _genome("t", contigs)
        pa, texts = g.packed(), None
        texts = R.contig_texts(pa)
        assert [bytes(t) for t in texts] == [bytes(c) for c in contigs]
        n_checked = 0
        for c, text in enumerate(texts):
            n = len(text)
            spans = [(ws, ws + ln) for ws in range(16) for ln in (0, 1, 2, 3, 4, 5, 60, 61, 62) if ws + ln <= n]
            spans += [(0, n), (n - 61, n), (n - 16, n), (n - 3, n), (max(0, n - 200), n), (30, 110), (190, 212)]  # clipped at either end; the last base
            for ws, we in spans:
                if not (0 <= ws <= we <= n):
                    continue
                for strand in (1, -1):
                    for f in range(3):
                        want = R.frame_text(text, ws, we, strand, f)
                        got = R.harness_text(pa, c, ws, we, strand, f)
                        assert got.tobytes() == want.tobytes(), (c, ws, we, strand, f)
                        n_checked += 1
        assert n_checked > 1500
        assert {(int(pa.ctg_start[c]) + ws) % 16 for c in range(len(texts)) for ws in range(16)} == set(range(16))
    # the window that ends on the assembly's last base reads the last word and nothing behind it
    from types import SimpleNamespace

    full = _genome("t", [first, last]).packed()
    end = int(full.ctg_start[-1]) + int(full.ctg_len[-1])
    assert end % 16 == 0
    pa = SimpleNamespace(words=np.ascontiguousarray(full.words[: end // 16]).copy(), n_runs=full.n_runs, ctg_start=full.ctg_start, ctg_len=full.ctg_len)
    assert int(pa.ctg_start[-1]) + int(pa.ctg_len[-1]) == 16 * len(pa.words)
    for ws in (0, 100, 141):
        for strand in (1, -1):
            for f in range(3):
                assert R.harness_text(pa, 1, ws, 144, strand, f).tobytes() == R.frame_text(last, ws, 144, strand, f).tobytes()
    assert b"X" in R.harness_text(_genome("t", [first]).packed(), 0, 30, 110, 1, 0).tobytes()


def test_coordinates_and_edges():
    out = np.zeros(3, np.int32)
    for ws, we in ((0, 300), (7, 298), (11, 12)):
        for sf in range(6):
            strand, f = (-1 if sf >= 3 else 1), sf % 3
            A = max(0, (we - ws - f) // 3)
            for a0, a1 in ((0, A), (0, 0), (A // 2, A), (1, max(1, A - 1))):
                if a1 > A or a0 > a1:
                    continue
                for clen, tol in ((300, 5), (305, 0), (1000, 5)):
                    R.harness().kpy_rs_coords(ws, we, sf, a0, a1, clen, tol, _p(out))
                    t0, t1 = (ws + f + 3 * a0, ws + f + 3 * a1) if strand > 0 else (we - f - 3 * a1, we - f - 3 * a0)
                    assert out.tolist() == [t0, t1, (1 if t0 <= tol else 0) | (2 if t1 >= clen - tol else 0)]


# ---- the formatter ------------------------------------------------------------------------------------------------------------------------
def _record(**kw):
    r = np.zeros(1, R.RESCUE_DTYPE)
    for k, v in kw.items():
        r[k] = v
    return r


def test_format_rescue_against_the_python_formatter():
    genes, loci, prot_len = ["gA", "gB", "gC"], ["L1", "L2"], np.array([100, 250, 1], np.int32)
    full = dict(piece=0, contig=1, t_start=30, t_end=330, matches=70, mismatches=28, gaps=2, p_start=0, p_end=100, a_len=400, strand=1, frame=2)
    rows = [
        _record(gene=0, score=R.MIN_SCORE, **full),                              # exactly at the threshold: diverged
        _record(gene=0, score=R.MIN_SCORE - 1, **full),                          # one below: absent
        _record(gene=0, score=300, stops=2, **full),                             # interrupted
        _record(gene=0, score=300, edge=1, **{**full, "p_start": 20}),           # partial, start
        _record(gene=0, score=300, edge=2, **{**full, "p_end": 89, "strand": -1}),  # partial, end, reverse strand
        _record(gene=0, score=300, edge=3, **{**full, "p_end": 50}),             # partial, both
        _record(gene=0, score=300, edge=3, **full),                              # edges but the whole protein: diverged
        _record(gene=0, score=300, **{**full, "p_start": 11}),                   # 89 % covered: fragment
        _record(gene=0, score=300, **{**full, "p_start": 10}),                   # 90 %: diverged
        _record(gene=1, piece=-1),                                               # nothing found
        _record(gene=2, score=1, piece=0, contig=0, t_start=0, t_end=3, matches=1, p_end=1, a_len=5, strand=-1, frame=0, stops=1, edge=1),
        _record(gene=1, score=200, **{**full, "matches": 1, "mismatches": 2, "gaps": 0, "p_end": 83}),  # 33.33 / 33.20
    ]
    recs = np.concatenate(rows)
    off = np.array([0, 9, 9, len(recs)], np.int64)
    asm, contigs, best = ["a0", "empty", "a2"], [["c0", "c1"], ["x"], ["y0", "y1"]], np.array([0, 1, 1], np.int32)
    first = np.array([0, 2, 3, 5], np.int64)
    for min_score in (R.MIN_SCORE, 0, 250):
        got = _native.format_rescue(genes, loci, asm, [n for c in contigs for n in c], first, prot_len, best, recs, off, min_score)
        assert got == R.tsv(recs, off, asm, contigs, genes, loci, best, prot_len, min_score), min_score
    got = _native.format_rescue(genes, loci, asm, [n for c in contigs for n in c], first, prot_len, best, recs, off)
    calls = [ln.split(b"\t")[4] for ln in got.splitlines()]
    assert calls == [b"diverged", b"absent", b"interrupted", b"partial", b"partial", b"partial", b"diverged", b"fragment", b"diverged", b"absent",
                     b"absent", b"fragment"]  # fmt: skip
    assert [ln.split(b"\t")[-1] for ln in got.splitlines()] == [b".", b".", b".", b"start", b"end", b"both", b"both", b".", b".", b".", b"start", b"."]
    zero = got.splitlines()[9].split(b"\t")
    assert zero[5] == b"0" and zero[6:13] == [b"."] * 7 and zero[16:18] == [b"0.00", b"0.00"]
    assert got.splitlines()[11].split(b"\t")[16:18] == [b"33.33", b"33.20"] and all(len(ln.split(b"\t")) == 20 for ln in got.splitlines())
    assert len(R.HEADER.rstrip(b"\n").split(b"\t")) == 20
    bad = recs.copy()
    bad["gene"][0] = 3
    with pytest.raises(ValueError):
        _native.format_rescue(genes, loci, asm, [n for c in contigs for n in c], first, prot_len, best, bad, off)
    bad = recs.copy()
    bad["contig"][0] = 2
    with pytest.raises(ValueError):
        _native.format_rescue(genes, loci, asm, [n for c in contigs for n in c], first, prot_len, best, bad, off)
    assert _native.format_rescue(genes, loci, [], [], [0], prot_len, [], recs[:0], [0]) == b""


# ---- the preconditions of the GPU cases, from the oracle's own pipeline ------------------------------------------------------------------
def test_planted_genes_are_missing_and_the_yardstick_finds_them(oracle):
    from kaptive_amd.pack import pack_sequences_flat
    from kaptive_amd.serotyping.core import Serotyper
    from tests import harness_util as H

    db = R.plant_db()
    typer = Serotyper(db, aligner=lambda g: None)
    hdb, prm = H.HarnessDb(db), H.params(db, typer)
    odb = oracle.OracleDB(*pack_sequences_flat(db.genes))
    cases = R.plants(db)
    assert len(cases) == 27
    prot_len = np.asarray(db.translations.lengths)
    assert int(prot_len[cases["diverged"][1]]) <= R.STRIP_LIMITS[1] < R.STRIP_LIMITS[2] < int(prot_len[cases["long"][1]])
    for name, (genome, gene, expect) in cases.items():
        if name.startswith("shift") and name not in ("shift0", "shift7"):
            continue  # (the same gene behind k more bases: the GPU test compares every one of them)
        pa = genome.packed()
        hits = np.array(odb.align(pa))
        if name == "no_hit":
            assert len(hits) == 0
            continue
        scores, counts = H.locus_scores(hits, hdb, typer.min_gene_coverage)
        best, _, _ = B.choose_best_loci(scores[None, :], counts[None, :], typer._expected_genes_per_locus)
        assert int(best[0]) == R.PLANT_LOCUS, name
        kept, pieces, summary, _ = H.reduce(hits, hdb, prm, best[0], pa)
        g0 = int(db.locus_gene_offsets[R.PLANT_LOCUS])
        assert [g0 + j for j in R.subjects(summary)] == [gene], f"{name}: the edited gene, and no other, is missing"
        recs = R.restate(summary, pieces, pa, db, R.FLANK, typer.partial_edge_tolerance)
        assert len(recs) == 1 and int(recs["gene"][0]) == gene
        r = recs[0]
        assert (int(r["score"]) >= R.MIN_SCORE) == expect["found"], (name, r)
        if "call" in expect:
            assert R.call(r, int(prot_len[gene]), R.MIN_SCORE) == expect["call"], (name, r)
        if "piece_contig" in expect:
            assert int(r["contig"]) == expect["piece_contig"] and len({int(p["contig"]) for p in pieces}) >= 3, name
        if expect.get("unclipped"):
            pc = pieces[int(r["piece"])]
            ws, we = R.window(int(pc["start"]), int(pc["end"]), int(pa.ctg_len[int(pc["contig"])]), R.FLANK)
            assert ws == int(pc["start"]) - R.FLANK and we == int(pc["end"]) + R.FLANK, "the default flank fits the contig on both sides"
        if name == "reversed":
            assert int(r["strand"]) == -1
        if name == "n_run":
            assert int(r["mismatches"]) >= 7  # (the codons under the N run read X)


# ---- the surface that needs no device ---------------------------------------------------------------------------------------------------
def test_flags_are_absent_unless_given_and_need_the_report(capsys):
    from kaptive_amd.cli import build_parser

    plain = build_parser().parse_args(["assembly", "db.npz", "a.fasta"])
    assert not hasattr(plain, "rescue") and not hasattr(plain, "rescue_flank") and not hasattr(plain, "rescue_min_score")
    ns = build_parser().parse_args(["assembly", "db.npz", "a.fasta", "--rescue", "r.tsv", "--rescue-flank", "0", "--rescue-min-score", "120"])
    assert (ns.rescue, ns.rescue_flank, ns.rescue_min_score) == ("r.tsv", 0, 120)
    for extra in (["--rescue-flank", "100"], ["--rescue-min-score", "50"], ["--rescue", "r.tsv", "--rescue-flank", "65536"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["assembly", "db.npz", "a.fasta", *extra])
        assert "--rescue" in capsys.readouterr().err
    assert _native.REPORTS[-1] == _native.Report("rescue", _native.RESCUE_HEADER, "rescue", "rescue_tsv", "rescue records") and len(_native.REPORTS) == 5


def test_typers_refuse_rescue_options_without_the_report():
    from kaptive_amd.serotyping.core import Serotyper

    db = R.plant_db()
    for kw in (dict(rescue_flank=10), dict(rescue_min_score=10)):
        with pytest.raises(ValueError, match="rescue=True"):
            Serotyper(db, **kw)
    assert Serotyper(db, rescue=True, rescue_min_score=33).rescue_min_score == 33 and Serotyper(db).rescue_min_score == R.MIN_SCORE
