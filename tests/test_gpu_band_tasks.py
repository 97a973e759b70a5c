"""The stretch between the sorted anchor list and the filled bands -- kp_chain_kernel's clusters, kp_chain_score_kernel,
kp_task_hist_kernel / kp_task_scatter_kernel and kp_sw_kernel -- on every case of tests/band_tasks_util.py
(tests/test_band_tasks_oracle.py pins, with the oracle alone, that each case is what its label says).  For every assembly of
every batch: the anchors, the band tasks (sorted on all eight fields), every task's raw fill result, the join records and
the hits equal the oracle's (a fill result's score is the reported one: the best cell plus the two-piece credit of gaps
longer than 20 columns, as tests/test_gpu_trace_summary.py compares it).  Every batch runs a second time on the same context and a third time with its assemblies in
reverse order: the rows are the same wherever an assembly stands and whichever task shares a register pair with another.
Integers throughout: no tolerance, no case left out of a comparison.

The fill results are compared in the order of the SORTED task list: once the device's sorted tasks equal the oracle's, the
oracle's fill of its own sorted list is odb.sw(pa, Batch.tasks(i)) up to that permutation, and it is computed once for the
three runs.  Not repeated here: N runs under the fill (test_gpu_parity.py::test_n_runs_under_every_fill_and_walk_match_oracle),
genes beyond the packed range (test_genes_beyond_the_packed_score_range, test_longest_genes_reach_the_packed_score_range),
gaps beyond 20 columns (test_joins_across_mid_size_indels_match_oracle, tests/test_gpu_cigar.py)."""

import numpy as np
import pytest

from kaptive_amd import _native
from tests import band_tasks_util as U
from tests import cigar_util as CU
from tests.test_gpu_parity import _same_records

pytestmark = pytest.mark.gpu
TASK_ORDER = list(_native.TASK_DTYPE.names)
MIN_DP = U.MIN_DP


@pytest.fixture(scope="module")
def built(oracle):
    return U.built(oracle)


@pytest.fixture(scope="module")
def ctx(built):
    c = _native.Context(0)
    c.load_genes(built["codes"], built["off"])
    yield c
    c.close()


_WANT: dict = {}


def _sorted_joins(j):
    return j[np.lexsort((j["lo"][:, 0], j["contig"], j["gs"]))] if len(j) else j


def _reported(built, pa, tasks, sw):
    """The oracle's rows carry the score of the best cell; the device's add the credit of gaps longer than KP_GAP_LONG = 20 columns
    (kp_spec.h: the two-piece gap cost), as the hits do.  Only a path with more than 20 gap columns in all can hold such a gap:
    its ops come from the yardstick of tests/cigar_util.py, which must agree with the oracle's row."""
    sw = sw.copy()
    gap_columns = 2 * sw[:, 6] - (sw[:, 2] - sw[:, 1]) - (sw[:, 4] - sw[:, 3])
    codes = None
    for k in np.flatnonzero((sw[:, 0] >= MIN_DP) & (gap_columns > 20)):
        codes = CU.assembly_codes(pa) if codes is None else codes
        out7, ops = CU.task_yardstick(built["codes"], built["off"], pa, codes, tasks[k])
        sw[k, 0] += sum(max((int(op) >> 4) - 20, 0) for op in ops if int(op) & 15 != CU.M)
        assert np.array_equal(out7, sw[k]), (tasks[k], out7, sw[k])  # (the yardstick reports the credited score)
    return sw


def _want(built, asm):
    """The oracle's side of one assembly, computed once for the three runs of its batch."""
    if asm.id not in _WANT:
        odb, pa = built["odb"], asm.packed()
        tasks = np.sort(odb.tasks(pa), order=TASK_ORDER)
        _WANT[asm.id] = dict(pa=pa, anchors=odb.anchors(pa), tasks=tasks, sw=_reported(built, pa, tasks, odb.sw(pa, tasks)),
                             joins=_sorted_joins(odb.joins(pa)), hits=odb.align(pa))  # fmt: skip
    return _WANT[asm.id]


def _run_and_compare(built, ctx, asms, what):
    want = [_want(built, a) for a in asms]
    batch = ctx.batch([w["pa"] for w in want])
    hits, off = batch.align()
    n_tasks = n_kept = 0
    for i, (asm, w) in enumerate(zip(asms, want)):
        where = f"{what}, {asm.id} (entry {i})"
        got = batch.anchors(i)
        assert np.array_equal(got, w["anchors"]), f"{where}: {len(got)} anchors, the oracle has {len(w['anchors'])}"
        tasks = batch.tasks(i)
        order = np.argsort(tasks, order=TASK_ORDER)
        _same_records(tasks[order], w["tasks"], f"{where}: tasks")
        res = batch.task_results(i)
        assert len(res) == len(tasks), f"{where}: {len(res)} result rows for {len(tasks)} tasks"
        res, sw = res[order], w["sw"]
        kept = sw[:, 0] >= MIN_DP
        bad = np.flatnonzero((res[:, 0] != sw[:, 0]) | (kept & (res != sw).any(axis=1)) | (~kept & res[:, 1:].any(axis=1)))
        assert len(bad) == 0, f"{where}: {len(bad)} fill results differ, the first: task {w['tasks'][bad[0]]} gives {res[bad[0]]}, the oracle {sw[bad[0]]}"
        joins = _sorted_joins(batch.joins(i))
        assert len(joins) == len(w["joins"]), f"{where}: {len(joins)} join records, the oracle has {len(w['joins'])}"
        for f in w["joins"].dtype.names:
            assert np.array_equal(joins[f], w["joins"][f]), f"{where}: join field {f}"
        _same_records(hits[off[i] : off[i + 1]], w["hits"], f"{where}: hits")
        n_tasks += len(tasks)
        n_kept += int(kept.sum())
    batch.close()
    return n_tasks, n_kept


def _three_runs(built, ctx, asms, what):
    """The batch, the batch again on the same context, and the batch in reverse order."""
    first = _run_and_compare(built, ctx, asms, what)
    assert _run_and_compare(built, ctx, asms, f"{what}, second pass") == first
    assert _run_and_compare(built, ctx, asms[::-1], f"{what}, reverse order") == first
    return first


def _asms(cases):
    return [a for c in cases for a in c.asms]


def test_which_cluster_becomes_a_task(built, ctx):
    """Group A: KP_MIN_ANCHORS, KP_MIN_SEED_SPAN, KP_MIN_CHAIN_SCORE and KP_CHAIN_DP_MAX from both sides, the insertion sort and the
    first maximum of chain_small -- every case alone in its assembly, and all of them as the contigs of one."""
    cases = built["groups"]["A"]
    mixed = U.asm_of("A_mixed", [np.frombuffer(c.asms[0].contigs[0].seq, np.uint8) for c in cases])
    n_tasks, n_kept = _three_runs(built, ctx, [mixed, *_asms(cases), mixed], "which cluster becomes a task")
    assert n_tasks >= 3 * 7 and n_kept >= 3 * 6


def test_every_anchor_count_of_the_chain_score_tile(built, ctx):
    """Group A: clusters of 3 .. 26 anchors on either strand in one class list: every bin of the tile's counting sort."""
    n_tasks, _ = _three_runs(built, ctx, _asms(built["groups"]["A_counts"]), "anchor counts")
    assert n_tasks == 2 * (U.DP_MAX + 3 - U.MIN_ANCHORS)


def test_run_cuts_and_band_widths(built, ctx):
    """Group B: KP_DIAG_GAP, the band rule at diagonal ranges 0, 1, 2, 33, 34 and 97 on both strands, KP_MAX_SPREAD and a run
    cut twice; a copy cut by a contig boundary and by an assembly boundary."""
    n_tasks, n_kept = _three_runs(built, ctx, _asms(built["groups"]["B"] + built["groups"]["B_cuts"]), "cuts and widths")
    assert n_kept >= 20


def test_rounds_of_64_anchors_and_wave_slices(built, ctx):
    """Group C: list positions that only the cluster logic of kp_chain_kernel tells apart (tests/occ_cut_util.py's group A walks
    a stretch through the rounds and slices themselves)."""
    n_tasks, _ = _three_runs(built, ctx, _asms(built["groups"]["C"]), "rounds and slices")
    assert n_tasks >= 10


def test_task_order_buckets(built, ctx):
    """Group D: tasks on both sides of a bucket edge and of the clamp of the task order, and a gene on either side of
    KP_FILL16_MAX_GENE_LEN in one class list: a task the scatter loses shows as a wrong result row."""
    n_tasks, n_kept = _three_runs(built, ctx, _asms(built["groups"]["D_order"]), "task order")
    assert n_tasks == n_kept == len(built["groups"]["D_order"]) + 2


@pytest.mark.parametrize("which", range(4))
def test_chain_score_tile_sizes(built, ctx, which):
    """Group D: class lists of KP_CS_TILE - 1, KP_CS_TILE, KP_CS_TILE + 1 and 2 KP_CS_TILE + 1 provisional tasks batch-wide."""
    c = built["groups"]["D_tile"][which]
    n_tasks, _ = _three_runs(built, ctx, list(c.asms), c.label)
    assert n_tasks == (U.TILE - 1, U.TILE, U.TILE + 1, 2 * U.TILE + 1)[which] - 1  # (one is rejected by its chain score)


@pytest.mark.parametrize("which", range(4))
def test_task_stage_sizes(built, ctx, which):
    """Group D: one block of kp_chain_kernel stages KP_CHAIN_STAGE - 1, KP_CHAIN_STAGE, KP_CHAIN_STAGE + 1 and, three classes
    mixed, twice that many tasks."""
    c = built["groups"]["D_stage"][which]
    n_tasks, _ = _three_runs(built, ctx, list(c.asms), c.label)
    assert n_tasks > 2 * U.STAGE


def test_fill_shapes(built, ctx):
    """Group E: steps around whole chunks and pieces for each width, rows that start behind the gene's first, contigs shorter
    than their band, copies at every residue mod 16, a short and a long task alone in a class."""
    n_tasks, n_kept = _three_runs(built, ctx, _asms(built["groups"]["E_shapes"]), "fill shapes")
    assert n_kept >= 2 * len(U.STEP_SHAPES) - 4


@pytest.mark.parametrize("which", range(5))
def test_class_populations(built, ctx, which):
    """Group E: classes of 1, 2, 2G - 1, 2G and 2G + 1 tasks batch-wide: the absent partner of a pair, the second quad."""
    c = built["groups"]["E_batches"][1 + which]
    n_tasks, _ = _three_runs(built, ctx, list(c.asms), c.label)
    g = {w: 64 // p for w, p in U.LANES.items()}
    assert n_tasks == sum((1, 2, 2 * x - 1, 2 * x, 2 * x + 1)[which] for x in g.values())


def test_first_and_last_base_of_a_batch(built, ctx):
    """Group E: a copy from base 0 of the batch's first assembly and one up to the last base of its last: the fill's window
    words before the first and behind the last word of the batch."""
    c = built["groups"]["E_batches"][0]
    assert _three_runs(built, ctx, list(c.asms), c.label) == (2, 2)


def test_scores_at_the_cut_off_and_ties(built, ctx):
    """Group E: best cells of 78, 79 and 80; maxima met again and beaten near a copy's end on both strands: the first maximum in
    (row, column) order is the one reported."""
    n_tasks, n_kept = _three_runs(built, ctx, _asms(built["groups"]["E_scores"]), "scores and ties")
    assert (n_tasks, n_kept) == (13, 11)
