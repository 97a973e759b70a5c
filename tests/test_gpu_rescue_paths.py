"""Every row, strip, tie and queue path of the rescue fill on the device (kaptive_amd/csrc/kp_rescue.hip, kp_rescue.h, kp_prot_cell.h)
against the yardstick of tests/rescue_util.py, byte for byte, on the cases of tests/rescue_paths_util.py: frame texts of k - 1, k and
k + 1 residues for k = 64, 128, 192 (the refill of the LDS ring, the publication of the previous strip's last column, lane 63's
flush) with the best cell on the last row, for every columns-per-lane class and for proteins of two and three strips, and of one to
three residues against a strip protein; two cells of one matrix with the maximal score -- in one lane, in two lanes (rs_reduce), in
two strips (the !ROW_MAJOR branch of prot_cell_lean) --; second-pass rectangles that end on both sides of every column class and of
a row chunk; two tasks of one window with the same score; 254 subjects an assembly in every word of the missing mask, a locus
beyond KP_MAX_LOCUS_GENES, several tasks and subjects per wave with strip and small tasks mixed, twice, and on a work slot whose boundary
scratch a longer strip task has filled; N runs at and across the window's edges on both strands.  The only other assertions are the scenario checks of
rescue_paths_util on the yardstick's records.  (Their preconditions are proved without a device in tests/test_rescue_paths_cpu.py.)"""

from __future__ import annotations

import numpy as np
import pytest

from kaptive_amd import _native
from tests import rescue_paths_util as P
from tests import rescue_util as R

pytestmark = pytest.mark.gpu


def _same(got, want, label, ids):
    (g, g_off), (w, w_off) = got, want
    assert g.dtype == _native.RESCUE_DTYPE == R.RESCUE_DTYPE, label
    assert g_off.tolist() == w_off.tolist(), f"{label}: offsets {g_off.tolist()} vs {w_off.tolist()}"
    if g.tobytes() != w.tobytes():
        i = next(i for i in range(len(g)) if g[i] != w[i])
        a = int(np.searchsorted(w_off, i, side="right")) - 1
        raise AssertionError(f"{label}: assembly {a} ({ids[a]}) record {i}: device {g[i]} vs the yardstick's {w[i]}")


class Run:
    """One context for one database; `batch(case)` makes the case's batch resident, replaces its hit table with the hand-made one and
    reduces it."""

    def __init__(self, db):
        from kaptive_amd.engine import Engine
        from kaptive_amd.serotyping.core import Serotyper

        self.db = db
        self.eng = Engine(db, rescue=True, rescue_flank=0)
        self.typer = Serotyper(db)
        self.typer._engine = self.eng

    def batch(self, case):
        from kaptive_amd.serotyping import batch as B

        packed = [g.packed() for g in case.genomes]
        b = self.eng.ctx.batch(packed)
        b.align_async()
        b.wait()
        off = np.concatenate([[0], np.cumsum([len(t) for t in case.tables])]).astype(np.int64)
        b.set_hits(np.concatenate(case.tables), off)
        scores, counts = b.score(self.typer.min_gene_coverage)
        best, _, _ = B.choose_best_loci(scores, counts, self.typer._expected_genes_per_locus)
        b.reduce_async(best, self.eng.typing_params(self.typer))
        return b, packed

    def check(self, case, b, packed):
        """The device's records against the yardstick's on the device's own summaries and pieces, then the case's scenario checks on
        the yardstick's records.  Returns (summaries, the device's records and offsets, the yardstick's)."""
        self.eng.ctx.set_option("rescue_flank", case.flank)
        sums, kept, pieces = b.typing(0)
        got = b.rescue(0)
        want = R.restate_batch(sums, pieces, packed, self.db, case.flank, self.typer.partial_edge_tolerance)
        _same(got, want, case.name, case.ids)
        P.check_expect(case, packed, sums, pieces, *want)
        return sums, got, want

    def whole(self, case):
        b, packed = self.batch(case)
        try:
            return self.check(case, b, packed)
        finally:
            b.close()

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def rows():
    run = Run(P.rows_db())
    yield run
    run.close()


def test_frame_texts_around_every_row_chunk_with_the_best_cell_on_the_last_row(rows):
    case = P.rows_case()
    sums, got, (records, off) = rows.whole(case)
    G = P.ROWS_GENE
    for k in P.ROW_KS:
        for name in ("S", "M", "W", "D", *(["T"] if k == P.ROW_KS[0] else [])):
            lens = {int(P.record_of(case, sums, records, off, e["asm"], e["gene"])["a_len"])
                    for e in case.expect if e["gene"] == G[name] and case.ids[e["asm"]].startswith(f"k{k}d")}  # fmt: skip
            assert lens == {k - 1, k, k + 1}, (k, name, lens)


def test_one_to_three_rows_against_a_strip_protein(rows):
    rows.whole(P.few_rows_case())


def test_second_pass_rectangles_on_both_sides_of_every_column_class(rows):
    case = P.rect_case()
    sums, got, (records, off) = rows.whole(case)
    assert {int(P.record_of(case, sums, records, off, e["asm"], e["gene"])["p_end"]) for e in case.expect} == set(P.RECT_COLUMNS)


def test_two_tasks_of_one_window_with_the_same_score(rows):
    rows.whole(P.task_ties_case())


def test_n_runs_at_and_across_the_windows_edges(rows):
    rows.whole(P.n_runs_case())


def test_two_cells_of_one_matrix_with_the_maximal_score():
    run = Run(P.ties_db())
    try:
        run.whole(P.ties_case())
    finally:
        run.close()


def test_many_subjects_and_waves_through_mixed_tasks():
    case, long_case = P.many_case(P.MANY_SECOND), P.long_scratch_case()
    run = Run(case.db)
    try:
        b, packed = run.batch(case)
        sums, first, (records, off) = run.check(case, b, packed)
        P.check_many(case, sums, records, off)
        # the same batch again: the records are kept per flank, so another flank and the first one again make them twice more
        run.eng.ctx.set_option("rescue_flank", 1)
        b.rescue(0)
        run.eng.ctx.set_option("rescue_flank", case.flank)
        second = b.rescue(0)
        assert second[0].tobytes() == first[0].tobytes() and second[1].tobytes() == first[1].tobytes()
        b.close()
    finally:
        run.close()
    # A second context, where the batch finds a boundary scratch that a strip task of 667 rows wrote.  The scratch belongs to a work
    # slot's typing run (KpRescueState in KpTypingRun), and a context hands its WORK_SLOTS slots to newly aligned batches in turn
    # (kp_batch_align: work[next_slot++ % KP_WORK_SLOTS]; closing a batch does not turn the counter back).  So the long case goes
    # through WORK_SLOTS batches -- slots 0, 1, 2: every slot's scratch now holds its rows --, and the batch that follows takes slot
    # WORK_SLOTS % WORK_SLOTS = 0 again: a scratch sized and filled for 667 rows, stale beyond every A of this batch.
    run = Run(case.db)
    try:
        _, long_first, _ = run.whole(long_case)
        for _ in range(1, _native.WORK_SLOTS):
            lb, _ = run.batch(long_case)
            again = lb.rescue(0)
            lb.close()
            assert again[0].tobytes() == long_first[0].tobytes() and again[1].tobytes() == long_first[1].tobytes()
        b, packed = run.batch(case)
        _, third, _ = run.check(case, b, packed)
        assert third[0].tobytes() == first[0].tobytes() and third[1].tobytes() == first[1].tobytes()
        b.close()
    finally:
        run.close()


def test_a_locus_beyond_the_missing_mask_never_reaches_the_rescue():
    """The yardstick's rule for such a locus -- no record, the offset does not advance (test_rescue_paths_cpu.py, on the harness's
    summaries) -- has no device counterpart: the database is refused when it is loaded."""
    with pytest.raises(ValueError, match="KP_MAX_LOCUS_GENES"):
        Run(P.many_db(P.MANY_WIDE)).close()
