"""What the inputs of tests/band_tasks_util.py are, by the CPU oracle alone: how many anchors a cluster has, how many query
bases and diagonals they cover and what their chain scores; how wide the band is and where it starts; which rows and how
many steps the fill takes; where a cluster lies in the sorted list against the rounds of 64 anchors and the wave slices of
kp_chain_kernel, how many tasks a block stages, how many a class list holds batch-wide.  Every size is derived from the
constants tests/band_tasks_util.py was built for, and the first test reads them out of include/kp_spec.h, csrc/kp_chain.hip,
csrc/kp_internal.h and csrc/kp_sw.hip: whoever changes one gets a failure here, not an edge that
tests/test_gpu_band_tasks.py quietly no longer meets.  The restated rules (clusters, chain, band, rows) are checked against
the oracle's task list on every assembly of every case."""

import numpy as np
import pytest

from tests import band_tasks_util as U


@pytest.fixture(scope="module")
def built(oracle):
    return U.built(oracle)


def _restated_tasks(m) -> list[tuple]:
    """The task list the restated rules give for the clusters measure() kept."""
    out = []
    for c, ch in zip(m["cl"], m["chains"]):
        if not c.provisional:
            continue
        if ch is None:
            out.append((c.gs, c.contig, c.lo, c.width, c.cnt, c.qmin, c.qmax, min(U.K * c.cnt, c.span)))
        elif ch.score >= U.MIN_CHAIN:
            out.append((c.gs, c.contig, c.lo, c.width, ch.n_anchors, c.qmin, c.qmax, ch.score))
    return sorted(out)


def _check(built, group, min_hits=True):
    """Every case of the group is what its label says, the restated rules give the oracle's tasks, no band is 32 diagonals
    wide, no walk back is cut before the chain's start, and a case that claims a reported task has a hit."""
    bad = []
    for c in built["groups"][group]:
        m = U.measured(built["odb"], c)
        ms = m if isinstance(m, list) else [m]
        for x in ms:
            got = sorted(tuple(int(v) for v in t) for t in x["tasks"])
            if _restated_tasks(x) != got:
                bad.append(f"{c.label}: the restated rules give {_restated_tasks(x)[:3]}, the oracle {got[:3]}")
            if 32 in x["tasks"]["width"] or any(k.width == 32 for k in x["all"]):
                bad.append(f"{c.label}: a band of 32 diagonals")
            if any(ch is not None and ch.cut_early for ch in x["chains"]):
                bad.append(f"{c.label}: a chain cut at a peak before its start")
        if c.holds is not None and not c.holds(m):
            bad.append(f"{c.label}: not what the label says: clusters (anchors, span, range, width, first) {[(k.cnt, k.span, k.spread, k.width, k.first) for x in ms for k in x['cl']][:8]}, "
                       f"tasks {[tuple(int(v) for v in t) for x in ms for t in x['tasks']][:4]}, rows {[r for x in ms for r in x['rows']][:4]}, steps {[s for x in ms for s in x['steps']][:4]}")  # fmt: skip
        if c.hit and min_hits:
            if not any(len(x["hits"]) for x in ms) or not any((x["sw"][:, 0] >= U.MIN_DP).any() for x in ms):
                bad.append(f"{c.label}: claims a task of at least {U.MIN_DP} and the oracle reports no hit")
    assert not bad, "\n".join(bad)
    return built["groups"][group]


def test_sizes_follow_the_constants_in_the_sources():
    assert U.kernel_constants() == U.EXPECTED_CONSTANTS, "a constant moved: rebuild the inputs of tests/band_tasks_util.py around it"
    # no diagonal range a cluster can have gives 32 diagonals: the 8-lane instantiations of the fill stay unreached
    widths = [U.band_of(r)[2] for r in range(U.SPREAD + 1)]
    assert 32 not in widths and widths[:3] == [16, 16, 64] and widths[33:35] == [64, 128] and widths[U.SPREAD] == U.C["KP_MAX_BAND"]
    assert [U.band_of(r)[0] for r in (1, 2)] == [U.C["KP_BAND_MARGIN_NARROW"], U.C["KP_BAND_MARGIN"]]
    assert [(U.band_of(r)[2] - U.band_of(r)[1]) % 2 for r in (0, 2, 33, 34)] == [1, 1, 0, 1]  # the odd (w - need) / 2 is met
    assert U.WIDTH_OF_RANGE == {r: U.band_of(r)[2] for r in U.STAIRS} and all(max(s, default=0) <= U.GAP and sum(s) == r for r, s in U.STAIRS.items())
    assert [U.length_bucket(r) for r in (31, 32, 63, 64, 2015, 2016, 2047, 2048, 2100)] == [63, 62, 62, 61, 1, 0, 0, 0, 0] and U.C["KP_ORDER_BUCKETS"] == U.C["BUCKET_CLAMP"] + 2
    assert U.slice_per(64 * U.SLICES) == 64 and U.slice_per(64 * U.SLICES + 1) == 128
    assert U.task_rows(-7, 16, 0, 100, 4002) == (0, 107) and U.task_rows(-1007, 16, 0, 100, 4002) == (992, 1107) and U.task_rows(50, 16, 0, 40, 4002) == (0, 0)
    assert sorted({s % U.C["CH"] for _, s in U.STEP_SHAPES}) == sorted(U.CHUNK_RESIDUES) and all(sum(w == k for k, _ in U.STEP_SHAPES) == 6 for w in U.LANES)
    assert U.CHAIN_PEN[:3] == [0, 0, 1] and len(U.CHAIN_PEN) == 512


def test_a_walk_back_always_reaches_the_chains_start():
    """peak_cut is not a case: every f is at least KP_K > 0, so the score counted from the chain's end, f[best] - f[i], stays below
    f[best], the value at the chain's start -- the cut of chain_small always falls there.  Shown on random anchor sets."""
    rng = np.random.default_rng(77)
    for _ in range(300):
        n = int(rng.integers(1, U.DP_MAX + 1))
        q = np.sort(rng.choice(400, n, replace=False)).astype(np.uint64)
        d = np.sort(rng.integers(0, U.SPREAD + 1, n)).astype(np.uint64) + np.uint64(U.DIAG_BIAS + 1000)
        keys = np.sort((np.uint64(5) << np.uint64(46)) | (d << np.uint64(16)) | rng.permutation(q))
        ch = U.chain_small(keys)
        assert not ch.cut_early and ch.n_anchors >= 1 and ch.score >= U.K


def test_which_cluster_becomes_a_task(built):
    """Group A: KP_MIN_ANCHORS (anchors_2 / anchors_3), KP_MIN_SEED_SPAN (span_39 / span_40), KP_MIN_CHAIN_SCORE with a penalty of
    0 and a larger one (chain_39 / chain_40), KP_CHAIN_DP_MAX (dp_24 / dp_25), the insertion sort of chain_small (reorder_del,
    reorder_tie) and two predecessors with the same f + sc (first_max, on chain_40_dd12)."""
    cases = _check(built, "A", min_hits=True)
    labels = " ".join(c.label for c in cases)
    for word in ("anchors_2", "anchors_3", "span_39", "span_40", "chain_39_dd1", "chain_40_dd1", "chain_39_dd20", "chain_40_dd12", "dp_24", "dp_25", "reorder_del", "reorder_tie", "first_max", "end_tie"):
        assert word in labels, f"the case {word} is gone"
    tie = next(c for c in cases if c.label.startswith("end_tie"))
    m = U.measured(built["odb"], tie)
    assert U.end_anchor_walks(m["keys"][m["cl"][0].first : m["cl"][0].first + m["cl"][0].cnt]) == (49, [7, 8]), "the end anchors of end_tie no longer tie"


def test_every_anchor_count_of_the_chain_score_tile(built):
    """Group A: one cluster of 3 .. 26 anchors on either strand: every bin of the counting sort of kp_chain_score_kernel."""
    cases = _check(built, "A_counts")
    got = sorted((U.measured(built["odb"], c)["cl"][0].cnt, U.measured(built["odb"], c)["cl"][0].gs & 1) for c in cases)
    assert got == [(n, s) for n in range(U.MIN_ANCHORS, U.DP_MAX + 3) for s in (0, 1)]


def test_where_a_run_is_cut_and_how_wide_its_band_is(built):
    """Group B: KP_DIAG_GAP (jump_32 / jump_33), KP_BAND_MARGIN_NARROW and KP_BAND_MARGIN with KP_MAX_BAND (ranges 0, 1, 2, 33, 34,
    97 on both strands, lo centred as the spec says), KP_MAX_SPREAD (spread_97 / spread_98, a run cut twice)."""
    cases = _check(built, "B")
    m = {c.label.split(":")[0]: U.measured(built["odb"], c) for c in cases}
    assert [len(m[k]["tasks"]) for k in ("jump_32", "jump_33")] == [1, 2]
    cut = m["spread_98"]["cl"][1]  # the soft cut falls in the middle of a merged piece: neither a round's first anchor nor a head
    assert cut.first % 64 not in (0, 63) and cut.d0 - m["spread_98"]["cl"][0].d0 == U.SPREAD + 1


def test_contig_and_assembly_boundaries_cut_a_copy(built):
    """Group B: a whole copy, cut by a contig boundary and by an assembly boundary 700 bases in and 15 and 14 bases before its
    end: the same diagonal on both sides, hits per contig, no column of the neighbour scored."""
    cases = _check(built, "B_cuts")
    assert sorted(c.label.split(":")[0] for c in cases) == sorted(f"{k}_cut_{x}" for k in ("contig", "assembly") for x in U.SPLITS)


def test_list_positions_against_rounds_and_slices(built):
    """Group C: heads on lanes 61, 62 and 63 of a run of KP_MIN_ANCHORS, a stray run that ends a round, a stray run KP_JOIN_BW,
    KP_JOIN_BW + 1 and many diagonals from the run before it and, independently, from the run after it, a stray run that only
    the run after it links (it opens a sequence of KP_JOIN_GROUP_MAX at 500 and is left out at 501), the soft cut on a round's
    first anchor, a round of 64 heads, a round without a head (lanes and rounds as the owning wave of kp_chain_kernel counts
    them, from where its walk starts), lists of 64, 65 and KP_CHAIN_SLICES * 64 + 1 anchors, a
    gene/strand over three whole slices.  The oracle's joins and tasks of every stray case are asserted."""
    cases = _check(built, "C")
    by = {c.label.split(":")[0]: c for c in cases}
    odb = built["odb"]
    for before, after in U.STRAY_GAPS:
        c = by[f"stray_bw_{before}_{after}"]
        joins, m = odb.joins(c.asms[0].packed()), U.measured(odb, c)
        bridged = before <= U.JOIN_BW and after <= U.JOIN_BW  # a member of a group either way it is linked; a chain runs through it only when both runs do
        assert [int(j["n_pieces"]) for j in joins] == ([3] if bridged else []) and len(m["tasks"]) == 2 and len(m["hits"]) == (1 if bridged else 2), c.label
    for gap, joined in ((U.JOIN_BW, True), (U.JOIN_BW + 1, False)):
        c = by[f"stray_after_only_{gap}"]
        joins, m = odb.joins(c.asms[0].packed()), U.measured(odb, c)
        pair = [j for j in joins if int(j["n_anchors"]) > 100]
        assert len(pair) == joined and (not joined or int(pair[0]["n_pieces"]) == 2), (c.label, joins[["n_pieces", "n_anchors"]])
        assert m["cl"][0].first == m["first"] and sum(k.provisional for k in m["cl"]) >= 2 and len(m["hits"]) == (1 if joined else 2), c.label
    for word in ("head_lane_61", "head_lane_62", "head_lane_63", "stray_lane_63", "spread_98_lane_0", "heads_64", "headless_round", "list_64", "list_65", "list_1025", "three_slices"):
        assert word in by, f"the case {word} is gone"


def test_order_tile_and_stage_sizes(built):
    """Group D: rows on both sides of a bucket edge and of the clamp of length_bucket, KP_FILL16_MAX_GENE_LEN; class lists on both
    sides of KP_CS_TILE; one block's stage on both sides of KP_CHAIN_STAGE -- pieces lone, not weak, no piece more than ten times."""
    _check(built, "D_order")
    _check(built, "D_tile")
    for c in _check(built, "D_stage"):
        m = U.measured(built["odb"], c)
        assert all(U.lone(m["all"])) and len(m["keys"]) == len(built["odb"].anchors(m["pa"], cut=False)), c.label
        per_gs = np.bincount([k.gs for k in m["all"]])
        assert per_gs.max() <= 10 and m["pa"].n_bases < 500_000, c.label


def test_fill_shapes(built):
    """Group E: steps of 0, 1, 8, 9, 56 and 57 beyond whole chunks of CH at the smallest size each width reaches (a task has at
    least KP_MIN_SEED_SPAN rows and a margin: 8 and 9 steps in all cannot be had), r_lo of 0, 8 and more, contigs shorter than
    their band, copies at every residue mod 16, a short and a long task alone in a class; class populations of 1, 2, 2G - 1, 2G
    and 2G + 1; the first and the last base of a batch."""
    cases = _check(built, "E_shapes")
    steps = {tuple(int(v) for v in c.label.split(":")[0][:-1].split("_")[1:]) for c in cases if c.label.startswith("steps_")}
    assert steps == set(U.STEP_SHAPES)
    assert min(s for x in (U.measured(built["odb"], c) for c in cases) for s in x["steps"]) >= U.MIN_SPAN + U.C["KP_BAND_MARGIN_NARROW"] + U.LANES[16] - 1
    _check(built, "E_batches")


def test_scores_at_the_cut_off_and_ties_of_the_best_cell(built):
    """Group E: best cells of KP_MIN_DP_SCORE - 2, - 1 and KP_MIN_DP_SCORE; a maximum met again two bases (a substitution) and three
    bases (a one-base gap either way) before the copy's end, and beaten three bases behind a substitution, on both strands: a
    plain fill shows the second cell, the oracle reports the first; tie_lanes_3's two cells lie in two lanes of the packed fill, the
    earlier in the lower one, tie_lanes_up_3's the earlier in the higher one."""
    cases = _check(built, "E_scores")
    assert sum(c.label.startswith(("tie_lanes_3", "tie_lanes_up_3")) for c in cases) == 4
    assert sorted(int(c.label.split(":")[0].split("_")[1]) for c in cases if c.label.startswith("score_")) == [U.MIN_DP - 2, U.MIN_DP - 1, U.MIN_DP]
