"""Breakpoint records, the parts that need no GPU (include/kp_spec.h, BREAKPOINTS): kp_breakpoints.h's functions -- the ones the
device kernel gives a lane per b -- built with g++ (tests/native_harness/breakpoints_harness.cpp) and compared, record for record,
with the Python restatement of tests/breakpoints_util.py on seeded random kept lists and on hand-made ones that sit on every
limit; kp_format_breakpoints against a Python formatter; and, end to end, the eight planted events of the miniature database from
the oracle's hits through the harness reduction to their records."""

from __future__ import annotations

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.serotyping import batch as B
from kaptive_amd.serotyping.batch import KEPT_DTYPE
from tests import breakpoints_util as P
from tests import cigar_util as U
from tests import cs_util as S

SIZES = (0, 1, 2, 63, 64, 65, 300, 2048)


def _table(n):
    rng = np.random.default_rng(515100 + n)
    lay = P.Layout(rng, rng.integers(600, 1801, size=40), frag=300 if n <= 300 else 40, duplicates=True).fill(n)
    pa = lay.genome(f"fuzz{n}").packed()
    return lay, pa, lay.kept()


@pytest.fixture(scope="module")
def tables():
    return {n: _table(n) for n in SIZES}


def _same(got, want, label):
    assert got.dtype == want.dtype and len(got) == len(want), f"{label}: {len(got)} records, the restatement has {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.tobytes() == w.tobytes(), f"{label}: record {i} {g} vs the restatement's {w}"


@pytest.mark.parametrize("n", SIZES)
def test_header_equals_the_restatement_on_random_kept_lists(tables, n):
    lay, pa, kept = tables[n]
    assert len(kept) == n
    want = P.restate(kept, pa.ctg_start, pa.ctg_len, U.assembly_codes(pa))
    for tile in (1 << 20, 64, 7):  # the candidates in one piece, in the kernel's smallest tile, in tiles that cut genes apart
        got, guard = P.harness_records(kept, pa, tile)
        assert guard, "a record stored beyond one per kept record"
        _same(got, want, f"{n} records, tile {tile}")
    assert (np.diff(want["kept_b"]) > 0).all() and not want["pad"].any()
    assert n <= 2 or len(want) > 0


def test_what_the_random_lists_cover(tables):
    classes: dict = {}
    kinds, per_gene, index_decides, spurious_candidate, ir = set(), set(), 0, 0, 0
    for n, (lay, pa, kept) in tables.items():
        for k, v in lay.classes.items():
            classes[k] = classes.get(k, 0) + v
        rec = P.restate(kept, pa.ctg_start, pa.ctg_len, U.assembly_codes(pa))
        kinds |= {int(k) for k in rec["kind"]}
        ir += int((rec["ir_cols"] > 0).sum())
        per_gene |= {int(c) for c in np.unique(kept["gene"], return_counts=True)[1]} if n else set()
        for r in rec:
            b = kept[int(r["kept_b"])]
            keys, dead = [], 0
            for ia in np.flatnonzero(kept["gene"] == b["gene"]):
                p = P._pair(kept[ia], b, int(pa.ctg_len[kept[ia]["contig"]]), int(pa.ctg_len[b["contig"]])) if ia != r["kept_b"] else None
                if p is not None and kept["flags"][ia] & P.F_SPURIOUS:
                    dead += 1
                elif p is not None:
                    keys.append(p[0])
            index_decides += keys.count(min(keys)) > 1
            spurious_candidate += dead > 0
    for name in ("t_gap -64", "t_gap -65", "q overlap 64", "q overlap 65", "equal keys", "full copies", "three ranks", "rank 1 wins",
                 "rank 2 wins", "duplicate", "scattered"):  # fmt: skip
        assert classes.get(name, 0) > 0, f"no table holds the class {name!r}: {classes}"
    assert kinds == {P.COLLINEAR, P.INVERTED, P.DISORDERED, P.CONTIGS}
    assert {1, 2, 3, 4, 5, 6} <= per_gene, per_gene
    assert index_decides >= 3 and spurious_candidate >= 3 and ir >= 10


def _hand(rows, flags=None):
    """A kept list from (gene, contig, strand, q_start, q_end, t_start, t_end) rows."""
    k = np.zeros(len(rows), KEPT_DTYPE)
    for i, r in enumerate(rows):
        k[i]["gene"], k[i]["contig"], k[i]["strand"], k[i]["q_start"], k[i]["q_end"], k[i]["t_start"], k[i]["t_end"] = r
    if flags is not None:
        k["flags"] = flags
    return k


class _TwoContigs:  # what a packed assembly of two contigs of 6000 random bases holds
    def __init__(self):
        self.codes = np.random.default_rng(8).integers(0, 4, size=2 * 6016).astype(np.uint8)
        self.ctg_start, self.ctg_len = np.array([0, 6016], np.int32), np.array([6000, 6000], np.int32)
        self.words, self.n_runs = S.pack_target(self.codes)[0], np.zeros((0, 2), np.int32)


def _both(kept):
    """The records of a hand-made list by the restatement, after the header has given the same."""
    pa = _TwoContigs()
    want = P.restate(kept, pa.ctg_start, pa.ctg_len, pa.codes)
    got, guard = P.harness_records(kept, pa)
    assert guard
    _same(got, want, "hand-made list")
    return want


def test_limits_of_the_pair_rule_and_of_the_kinds():
    # gene overlap of exactly 64 is a pair, 65 is none
    r = _both(_hand([(0, 0, 1, 0, 400, 100, 500), (0, 0, 1, 336, 900, 500, 1064), (1, 0, 1, 0, 400, 2000, 2400), (1, 0, 1, 335, 900, 2400, 2965)]))
    assert [(int(x["kept_a"]), int(x["kept_b"]), int(x["q_gap"])) for x in r] == [(0, 1, -64)]
    # target overlap of exactly 64 is collinear, 65 disordered (and then ranked by the distance of the junction bases)
    r = _both(_hand([(0, 0, 1, 0, 400, 100, 900), (0, 0, 1, 400, 900, 836, 1600), (1, 0, -1, 0, 400, 3000, 3800), (1, 0, -1, 400, 900, 2265, 3065)]))
    assert [(int(x["kind"]), int(x["t_gap"]), int(x["t_lo"])) for x in r] == [(P.COLLINEAR, -64, 0), (P.DISORDERED, 0, 0)]
    # two full copies: no pair; a full copy next to two fragments: only the fragments pair (the copy ends where b ends, it starts where a starts)
    assert len(_both(_hand([(0, 0, 1, 0, 900, 100, 1000), (0, 1, 1, 0, 900, 100, 1000)]))) == 0
    r = _both(_hand([(0, 1, 1, 0, 900, 100, 1000), (0, 0, 1, 0, 400, 100, 500), (0, 0, 1, 400, 900, 1700, 2200)]))
    assert [(int(x["kept_a"]), int(x["kept_b"]), int(x["t_gap"]), int(x["t_lo"]), int(x["ir_cols"])) for x in r] == [(1, 2, 1200, 500, 32)]
    # equal keys: the kept index decides, whatever the list order
    rows = [(0, 1, -1, 0, 400, 7, 407), (0, 0, 1, 400, 900, 50, 550), (0, 1, -1, 0, 400, 7, 407)]
    assert [(int(x["kept_a"]), int(x["kept_b"])) for x in _both(_hand(rows))] == [(0, 1)]
    assert [(int(x["kept_a"]), int(x["kept_b"])) for x in _both(_hand(rows[::-1] + rows[:1]))] == [(0, 1)]
    # a spurious record is neither an a nor a b
    rows = [(0, 0, 1, 0, 400, 100, 500), (0, 0, 1, 400, 900, 503, 1003), (0, 1, 1, 0, 390, 100, 490)]
    assert [(int(x["kept_a"]), int(x["kind"])) for x in _both(_hand(rows))] == [(0, P.COLLINEAR)]
    assert [(int(x["kept_a"]), int(x["kind"])) for x in _both(_hand(rows, [16, 0, 0]))] == [(2, P.CONTIGS)]
    assert len(_both(_hand(rows, [0, 16, 0]))) == 0
    # all three ranks for one b: collinear beats inverted beats another contig, however near the others are
    rows = [(0, 1, 1, 0, 400, 5600, 6000), (0, 0, -1, 0, 400, 1001, 1401), (0, 0, 1, 0, 400, 100, 500), (0, 0, 1, 400, 900, 1000, 1500)]
    for dead, want in (([0, 0, 0, 0], (2, P.COLLINEAR)), ([0, 0, 16, 0], (1, P.INVERTED)), ([0, 16, 16, 0], (0, P.CONTIGS))):
        r = _both(_hand(rows, dead))
        assert [(int(x["kept_a"]), int(x["kind"])) for x in r] == [want]
    assert (r[0]["edge_a"], r[0]["edge_b"]) == (0, 1000)
    # the inverted repeat: t_gap 1 has no column, 2 and 3 have one, 65 has 32
    for gap, cols in ((1, 0), (2, 1), (3, 1), (63, 31), (64, 32), (65, 32)):
        r = _both(_hand([(0, 0, -1, 0, 400, 1500 + gap, 2000), (0, 0, -1, 400, 900, 1000, 1500)]))
        assert (int(r[0]["t_gap"]), int(r[0]["t_lo"]), int(r[0]["ir_cols"])) == (gap, 1500, cols) and r[0]["ir_matches"] <= cols


def test_layout_constants():
    import ctypes as C

    out = (C.c_int32 * 4)()
    P.harness().kpy_bp_layout(out)
    assert list(out) == [32, P.MAX_OVERLAP, P.IR_COLS, 8] and _native.BREAKPOINT_DTYPE.itemsize == 32


# ---- kp_format_breakpoints -------------------------------------------------------------------------------------------------------------
def _formatter_table():
    """Two assemblies (the first without a record): a kept list whose records name every event, on both sides of the edge tolerance."""
    rows = [(2, 0, 1, 0, 409, 1000, 1409), (2, 0, 1, 400, 1398, 2609, 3607),  # insertion with a duplication of 9
            (0, 1, -1, 0, 300, 2000, 2300), (0, 1, -1, 900, 1398, 1502, 2000),  # deletion, strand -1
            (1, 0, 1, 0, 300, 4000, 4300), (1, 0, 1, 350, 900, 4340, 4890),  # replacement
            (3, 1, 1, 0, 300, 100, 400), (3, 1, 1, 290, 700, 390, 800),  # overlap
            (4, 0, 1, 0, 700, 5000, 5700), (4, 0, -1, 700, 1398, 5700, 5990),  # inversion
            (5, 1, 1, 0, 300, 3000, 3300), (5, 1, 1, 300, 700, 2500, 2900),  # rearrangement
            (6, 0, 1, 0, 500, 5495, 5995), (6, 1, 1, 500, 900, 5, 405),  # contig break: both edges 5
            (7, 0, 1, 0, 500, 5494, 5994), (7, 1, 1, 500, 900, 5, 405)]  # translocation: an edge of 6
    kept = np.zeros((2, len(rows) + 1), KEPT_DTYPE)
    kept[1, : len(rows)] = _hand(rows)
    records = _both(kept[1, : len(rows)])
    return kept, records, np.array([0, 0, len(records)], np.int64)


def test_formatter_against_the_python_formatter():
    kept, records, bp_off = _formatter_table()
    genes = [f"gene{i}" for i in range(8)]
    asm_names, contigs = ["empty", "asm two"], [["x"], ["c1", "contig two"]]
    flat, first = [c for cs in contigs for c in cs], [0, 1, 3]
    for tol in (5, 4, 6):
        want = P.format_tsv(asm_names, contigs, genes, kept, records, bp_off, tol)
        got = _native.format_breakpoints(genes, asm_names, flat, first, kept, records, bp_off, tol)
        assert got == want and got.count(b"\n") == len(records) == 8
    lines = [ln.split(b"\t") for ln in _native.format_breakpoints(genes, asm_names, flat, first, kept, records, bp_off, 5).splitlines()]
    assert all(len(ln) == 16 for ln in lines) and _native.BREAKPOINTS_HEADER == P.HEADER and P.HEADER.count(b"\t") == 15
    assert {ln[2] for ln in lines} == set(P.EVENTS)
    by_event = {ln[2]: ln for ln in lines}
    assert by_event[b"insertion"] == [b"asm two", b"gene2", b"insertion", b"409", b"-9", b"c1", b"1409", b"+", b"c1", b"2610", b"+", b"1200", b"9", b"4591",
                                      b"2609", by_event[b"insertion"][15]]  # fmt: skip
    assert by_event[b"deletion"][3:13] == [b"300", b"600", b"contig two", b"2001", b"-", b"contig two", b"2000", b"-", b"0", b"0"]
    assert by_event[b"inversion"][11] == b"." and by_event[b"overlap"][15] == b"." and b"/" in by_event[b"insertion"][15]
    # the edge tolerance decides between a contig break and a translocation
    at4 = {ln.split(b"\t")[1]: ln.split(b"\t")[2] for ln in _native.format_breakpoints(genes, asm_names, flat, first, kept, records, bp_off, 4).splitlines()}
    at6 = {ln.split(b"\t")[1]: ln.split(b"\t")[2] for ln in _native.format_breakpoints(genes, asm_names, flat, first, kept, records, bp_off, 6).splitlines()}
    assert (at4[b"gene6"], at4[b"gene7"], at6[b"gene6"], at6[b"gene7"]) == (b"translocation", b"translocation", b"contig_break", b"contig_break")
    # a record that names a kept record, a gene or a contig the tables do not have is refused
    for field, value in (("kept_b", kept.shape[1]), ("kept_a", -1), ("kind", 4)):
        bad = records.copy()
        bad[field][0] = value
        with pytest.raises(ValueError):
            _native.format_breakpoints(genes, asm_names, flat, first, kept, bad, bp_off, 5)
    with pytest.raises(ValueError):
        _native.format_breakpoints(genes[:2], asm_names, flat, first, kept, records, bp_off, 5)
    with pytest.raises(ValueError):
        _native.format_breakpoints(genes, asm_names, ["x", "only one"], [0, 1, 2], kept, records, bp_off, 5)
    assert _native.format_breakpoints(genes, [], [], [0], kept[:0], records[:0], [0], 5) == b""


# ---- end to end on the CPU: oracle hits -> harness reduction -> records --------------------------------------------------------------------
def test_planted_events_from_the_oracles_hits(oracle):
    from kaptive_amd.pack import pack_sequences_flat
    from kaptive_amd.serotyping.core import Serotyper
    from tests import harness_util as H

    db = P.plant_db()
    typer = Serotyper(db, aligner=lambda g: None)
    hdb, prm = H.HarnessDb(db), H.params(db, typer)
    odb = oracle.OracleDB(*pack_sequences_flat(db.genes))
    cases = P.plants(db)
    assert len(cases) == 8
    for name, genome, gene_index, expect in cases:
        pa = genome.packed()
        hits = np.array(odb.align(pa))
        scores, counts = H.locus_scores(hits, hdb, typer.min_gene_coverage)
        best, _, _ = B.choose_best_loci(scores[None, :], counts[None, :], typer._expected_genes_per_locus)
        assert int(best[0]) == P.PLANT_LOCUS
        kept, pieces, summary, prot = H.reduce(hits, hdb, prm, best[0], pa)
        dp = oracle.protein_align(prot, kept["prot_off"], kept["prot_len"], db.translations.seqs, db.translations.offsets[kept["gene"]],
                                  db.translations.lengths[kept["gene"]])  # fmt: skip
        kept = H.states(kept, hdb, prm, genome.contigs.lengths, dp, summary)
        want = P.restate(kept, pa.ctg_start, pa.ctg_len, U.assembly_codes(pa))
        got, guard = P.harness_records(kept, pa)
        assert guard
        _same(got, want, name)
        P.check_plant(name, gene_index, expect, kept, got, typer.partial_edge_tolerance)  # ... and the unedited genes give no record


# ---- the surface that needs no device ---------------------------------------------------------------------------------------------------------
def test_flag_is_absent_from_the_namespace_unless_given():
    from kaptive_amd.cli import build_parser

    plain = build_parser().parse_args(["assembly", "db.npz", "a.fasta"])
    assert not hasattr(plain, "breakpoints")
    given = build_parser().parse_args(["assembly", "db.npz", "a.fasta", "--breakpoints", "bp.tsv"])
    assert given.breakpoints == "bp.tsv" and not hasattr(given, "variants") and not hasattr(given, "paf")


def test_a_batch_typed_without_the_option_names_it():
    bt = B.BatchTyping.__new__(B.BatchTyping)
    bt._breakpoints = None
    with pytest.raises(ValueError, match="breakpoints=True"):
        bt.breakpoints()
    with pytest.raises(ValueError, match="breakpoints=True"):
        bt.breakpoints_tsv()
