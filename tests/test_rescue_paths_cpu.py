"""The preconditions of tests/test_gpu_rescue_paths.py, without a device: every case of tests/rescue_paths_util.py through the g++ build
of the typing reduction (tests/harness_util.py: the summaries and pieces its hand-made hit tables give) and the yardstick of
tests/rescue_util.py.  Proved here, with the yardstick alone: each intended tie is a tie -- the two cells, each aligned without the
other, score the same, and the whole alignment reports the (row, column)-first --; each intended best cell lies on the intended side
of its limit (strip, columns per lane, row chunk); the winning frame texts have k - 1, k and k + 1 residues for k = 64, 128, 192; the
many-subjects batch has more subjects and several times more tasks than the fill launch has blocks; kp_rescue.h reads every window
with an N run at or across its edge as the yardstick does, with and without the shortcut for windows clear of runs."""

from __future__ import annotations

import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from kaptive_amd.serotyping import batch as B
from tests import rescue_paths_util as P
from tests import rescue_util as R


_TYPING: dict = {}


def _typing(db):
    from kaptive_amd.serotyping.core import Serotyper
    from tests import harness_util as H

    if db.metadata.name not in _TYPING:
        typer = Serotyper(db, aligner=lambda g: None)
        _TYPING[db.metadata.name] = (db, typer, H.HarnessDb(db), H.params(db, typer))
    return _TYPING[db.metadata.name]


@lru_cache(maxsize=None)
def _state(make, *args):
    """(case, packed, summaries, pieces per assembly, the yardstick's records, offsets) of a case, the reduction done by the harness."""
    from tests import harness_util as H

    case = make(*args)
    db, typer, hdb, prm = _typing(case.db)
    packed, sums, pieces = [g.packed() for g in case.genomes], [], []
    for pa, hits in zip(packed, case.tables):
        scores, counts = H.locus_scores(hits, hdb, typer.min_gene_coverage)
        best, _, _ = B.choose_best_loci(scores[None, :], counts[None, :], typer._expected_genes_per_locus)
        kept, pcs, summary, _ = H.reduce(hits, hdb, prm, best[0], pa)
        assert len(kept) == len(hits), "every hand-made hit is kept"
        sums.append(summary)
        pieces.append(pcs)
    sums = np.array(sums)
    recs = [R.restate(s, p, pa, db, case.flank, typer.partial_edge_tolerance) for s, p, pa in zip(sums, pieces, packed)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    return case, packed, sums, pieces, np.concatenate(recs), off


def _expect(make, *args):
    case, packed, sums, pieces, records, off = _state(make, *args)
    P.check_expect(case, packed, sums, pieces, records, off)
    return case, packed, sums, pieces, records, off


def test_row_chunk_and_ring_are_the_kernels():
    lanes = int(R.harness().kpy_rs_lanes())  # KP_RS_LANES
    assert (P.ROW_CHUNK, P.RING) == (lanes, 2 * lanes) and R.STRIP_LIMITS == tuple(P.ROW_CHUNK * nc for nc in (2, 4, 6)) and P.STRIP == 6 * lanes
    assert R.MAX_LOCUS_GENES == P.MANY_GENES == 4 * 64
    # The block counts of the fill launch are literals of ensure_rescue (kp_typing.hip), in no header the harness could compile: they are
    # read out of the source, whatever its spacing.  A change of how that function names them has to be followed here.
    src = (Path(__file__).resolve().parent.parent / "kaptive_amd" / "csrc" / "kp_typing.hip").read_text()
    body = src[src.index("static int ensure_rescue(") :]
    counts = tuple(int(x) for x in re.findall(r"\bn_blocks\s*=\s*(\d+)\s*;", body[: body.index("kp_launch_rescue_fill(")]))
    assert counts == P.FILL_BLOCKS


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------
def test_planted_tails_end_on_the_last_row_of_windows_around_every_chunk():
    case, packed, sums, pieces, records, off = _expect(P.rows_case)
    assert len(case.genomes) == len(P.ROW_KS) * len(P.ROW_DELTAS)
    G, lens = P.ROWS_GENE, {}
    for e in case.expect:
        r = P.record_of(case, sums, records, off, e["asm"], e["gene"])
        k = int(case.ids[e["asm"]][1:].split("d")[0])
        lens.setdefault((k, e["gene"]), set()).add(int(r["a_len"]))
    for k in P.ROW_KS:
        for name in ("S", "M", "W", "D"):
            assert lens[(k, G[name])] == {k - 1, k, k + 1}, (k, name)
    assert lens[(P.ROW_KS[0], G["T"])] == {63, 64, 65}
    # the window lengths are what the reduction's pieces give (every strip protein's stretch crosses a strip boundary: check_expect)
    for a, name in enumerate(case.ids):
        k, d = (int(x) for x in name[1:].split("d"))
        for pc in pieces[a]:
            ws, we = R.window(int(pc["start"]), int(pc["end"]), int(packed[a].ctg_len[int(pc["contig"])]), case.flank)
            assert we - ws == 3 * k + d and ws > 0 and we < int(packed[a].ctg_len[int(pc["contig"])])
    limits = R.STRIP_LIMITS
    lp = P.ROWS_PROTEINS
    assert sum("crosses" in e for e in case.expect) == len(case.genomes) + len(P.ROW_DELTAS) and {e["crosses"] for e in case.expect if "crosses" in e} == {P.STRIP, 2 * P.STRIP}
    assert lp["S"] <= limits[0] < lp["M"] <= limits[1] < lp["W"] <= limits[2] < lp["D"] <= 2 * limits[2] < lp["T"] <= 3 * limits[2]


def test_one_to_three_rows_against_a_strip_protein():
    case, packed, sums, pieces, records, off = _expect(P.few_rows_case)
    assert sorted({e["a_len"] for e in case.expect}) == [1, 2, 3] and P.ROWS_PROTEINS["E"] > P.STRIP
    prot = R.protein(case.db, P.ROWS_GENE["E"])
    assert bytes(prot[P.STRIP - 1 : P.STRIP + 2]) == b"WCW" and bytes(prot).count(b"W") == 2 and bytes(prot).count(b"C") == 1


# ---- ties inside a task -------------------------------------------------------------------------------------------------------------------
def test_tying_cells_tie_and_the_first_in_row_major_order_is_reported():
    case, packed, sums, pieces, records, off = _expect(P.ties_case)
    assert len(case.expect) == len(P.TIE_CELLS)
    for (tname, pname), cells in P.TIE_CELLS.items():
        text = np.frombuffer(P.TIE_TEXTS[tname].encode(), np.uint8)
        prot = R.protein(case.db, P.TIE_GENE[pname])
        a = case.ids.index(tname)
        assert R.harness_text(packed[a], 0, 51, 51 + 3 * len(text), 1, 0).tobytes() == text.tobytes(), "frame text 0 is the designed one"
        for row, col in cells:  # each cell without the other: the rectangle that ends on it, less the rows and columns the other needs
            other = cells[1] if (row, col) == cells[0] else cells[0]
            r0 = other[0] if other[0] < row else 0
            c0 = other[1] if other[1] < col else 0
            alone = R.align(text[r0:row], prot[c0:col])
            assert int(alone[0]) == P.TIE_SCORE and (r0 + int(alone[5]), c0 + int(alone[7])) == (row, col), (tname, pname, row, col, alone)
        whole = R.align(text, prot)
        assert int(whole[0]) == P.TIE_SCORE and (int(whole[5]), int(whole[7])) == cells[0] and cells[0] < cells[1], (tname, pname, whole)
        # no other frame of the window comes near: the tie is inside one task
        r = P.record_of(case, sums, records, off, a, P.TIE_GENE[pname])
        ws, we = P.window_of(case, packed, pieces, a, r)
        others = [int(R.align(R.frame_text(R.contig_texts(packed[a])[0], ws, we, s, f), prot)[0]) for s in (1, -1) for f in range(3)][1:]
        assert max(others) < P.TIE_SCORE // 2
    lane = lambda col, nc: ((col - 1) % P.STRIP) // nc  # noqa: E731
    assert lane(10, 2) != lane(40, 2) and lane(10, 4) != lane(170, 4) and lane(10, 6) != lane(320, 6)
    assert lane(10, 6) != lane(410, 6) and lane(10, 6) == lane(394, 6) and 394 > P.STRIP < 410


# ---- the second pass's rectangle --------------------------------------------------------------------------------------------------------------
def test_best_cells_on_both_sides_of_every_column_class_and_of_a_row_chunk():
    case, packed, sums, pieces, records, off = _expect(P.rect_case)
    got = {(int(r["p_end"]), P.end_rows(r, *P.window_of(case, packed, pieces, e["asm"], r))[1])
           for e in case.expect for r in [P.record_of(case, sums, records, off, e["asm"], e["gene"])]}  # fmt: skip
    assert got == {(c, a) for c in P.RECT_COLUMNS for a in P.RECT_ROWS}
    for lim in (*R.STRIP_LIMITS, 2 * P.STRIP):
        assert {lim - 1, lim + 1} <= set(P.RECT_COLUMNS)
    assert P.RECT_ROWS == (P.ROW_CHUNK - 1, P.ROW_CHUNK + 1) and P.ROWS_PROTEINS["T"] >= 800


# ---- ties between the tasks of one window -------------------------------------------------------------------------------------------------------
def test_two_tasks_of_one_window_tie_and_the_lower_index_is_reported():
    case, packed, sums, pieces, records, off = _expect(P.task_ties_case)
    g = P.ROWS_GENE["S"]
    prot = R.protein(case.db, g)
    for a, (first, second) in case.notes.items():
        r = P.record_of(case, sums, records, off, a, g)
        ws, we = P.window_of(case, packed, pieces, a, r)
        text = R.contig_texts(packed[a])[0]
        scores = [int(R.align(R.frame_text(text, ws, we, s, f), prot)[0]) for s in (1, -1) for f in range(3)]
        assert scores[first] == scores[second] == max(scores) == int(r["score"]), (case.ids[a], scores)
        assert sorted(scores)[-3] < scores[first] and first < second
        assert (0 if int(r["strand"]) > 0 else 3) + int(r["frame"]) == first
    assert {case.ids[a]: t for a, t in case.notes.items()} == dict(plus_minus=(0, 4), second_copy=(0, 2), first_copy=(0, 1))


# ---- many subjects -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_second", [P.MANY_SECOND, P.MANY_WIDE])
def test_many_subjects_fill_every_mask_word_and_queue_in_both_passes(n_second):
    case, packed, sums, pieces, records, off = _expect(P.many_case, n_second)
    assert case.db.metadata.name == ("wide" if n_second > P.MANY_GENES else "many") and P.MANY_WIDE == 257
    P.check_many(case, sums, records, off)
    a = case.ids.index("all1")
    mask = sums["missing_mask"][a]
    for bit in P.MANY_BITS:
        assert (int(mask[bit >> 6]) >> (bit & 63)) & 1
    assert int(case.db.translations.lengths[P.MANY_STRIP_GENE]) > P.STRIP
    lens = [int(x) for x in case.db.translations.lengths[2 : P.MANY_GENES] if int(x) != P.MANY_STRIP_LEN]
    assert 20 <= min(lens) and max(lens) <= 60


def test_a_longer_boundary_column_than_the_many_subjects_batch_has():
    case, packed, sums, pieces, records, off = _expect(P.long_scratch_case)
    _, mp, _, mpieces, _, _ = _state(P.many_case, P.MANY_SECOND)
    longest = max(int(pc["end"]) - int(pc["start"]) for pcs in mpieces for pc in pcs)
    assert 3 * 667 > longest + 600, "stale rows far beyond any frame text of the batch that follows"


# ---- N runs --------------------------------------------------------------------------------------------------------------------------------------
def test_windows_with_n_runs_at_and_across_their_edges():
    case, packed, sums, pieces, records, off = _expect(P.n_runs_case)
    assert len(case.genomes) == 2 * (len(P.N_PLACEMENTS) - 1) + 1
    for a, (place, at) in case.notes.items():
        pa = packed[a]
        (pc,) = pieces[a]
        ws, we = R.window(int(pc["start"]), int(pc["end"]), int(pa.ctg_len[0]), case.flank)
        assert (ws, we) == (P.N_LEFT, P.N_LEFT + 300)
        runs = np.asarray(pa.n_runs).reshape(-1, 2) - int(pa.ctg_start[0])
        assert [tuple(int(x) for x in r) for r in runs] == at
        touches = any(s < we and e > ws for s, e in at)
        assert touches == (place not in P.N_CLEAR)
        if place == "ends_at_ws":
            assert at[0][1] == ws
        if place == "starts_at_we":
            assert at[0][0] == we
        if place == "first_base":
            assert at[0][0] < ws and at[0][1] == ws + 1
        if place == "last_base":
            assert at[0][0] == we - 1 and at[0][1] > we
        text = R.contig_texts(pa)[0]
        for strand in (1, -1):
            for f in range(3):
                want = R.frame_text(text, ws, we, strand, f)
                assert R.harness_text(pa, 0, ws, we, strand, f).tobytes() == want.tobytes(), (place, strand, f)
                if place == "all_n":
                    assert len(want) > 0 and (want == ord("X")).all()
                if place in ("first_base", "last_base") and f == 0:
                    assert (want == ord("X")).sum() == 1 and ord("X") in (want[0], want[-1])
        if place == "in_codon":
            assert all((R.frame_text(text, ws, we, -1, f) == ord("X")).any() for f in range(3))
