"""Piece summaries of the band trace (kaptive_amd/csrc/kp_walk.h: KpTraceBlock) against the CPU oracle (run with -m gpu on an MI355X).

Both fill kernels leave, per lane stream, cell and 8-step piece, one bit "this piece is not eight plain diagonal steps"; the band
walks (traceback, CIGARs) take runs of plain pieces from those bits without fetching them.  Every case here is a hand-built gene
with a hand-built contig around one feature of a path -- where it ends, where it starts, where a gap's cell falls within a piece
and within a 64-step summary word, which band class and which fill kernel -- on the smallest shape that reaches it.  Each case
asserts that the hit table is the oracle's, that the per-task SW rows are the oracle's, and that hits and CIGAR ops of a context
created with KAPTIVE_AMD_TRACE_SUMMARY=0 (the walks then fetch every piece, as before the summaries) equal those of one created
without it.

"step" below is r - q0 + (bi >> 2) of a cell (row r, band index bi): the step of the fill at which the cell's lane computes it,
hence the piece (step / 8) and the summary word (step / 64) that hold it.
"""

from __future__ import annotations

import os

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.core.genome import GenomeAssembly
from kaptive_amd.core.seq import SeqRecord, Sequences
from kaptive_amd.pack import pack_sequences_flat
from kaptive_amd.synth import random_dna
from tests import cigar_util as U
from tests.test_gpu_parity import _same_records

pytestmark = pytest.mark.gpu

FLANK = 300
MIN_DP_SCORE = 80  # KP_MIN_DP_SCORE: tasks below it are not traced back
_COMPLEMENT = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}


def _other(base: int) -> int:
    return _COMPLEMENT[int(base)]


class Case:
    """A gene and the contig(s) that hold its edited copy; `edit(gene) -> copy` and the flanks make the contig."""

    def __init__(self, name, length, edit=None, left=FLANK, right=FLANK, cut_left=0, cut_right=0, n_at=None, distinct=(), expect=None):
        self.name, self.length, self.edit, self.left, self.right, self.distinct = name, length, edit, left, right, distinct
        self.cut_left, self.cut_right, self.n_at, self.expect = cut_left, cut_right, n_at, expect or {}

    def build(self, rng):
        self.gene = random_dna(rng, self.length, 0.5)
        for p in self.distinct:  # a gene base that differs from both its neighbours: a 1-base gap over it cannot slide
            self.gene[p] = next(c for c in b"ACGT" if c not in (self.gene[p - 1], self.gene[p + 1]))
        copy = self.gene.copy() if self.edit is None else self.edit(self.gene, rng)
        copy = copy[self.cut_left : len(copy) - self.cut_right]
        if self.n_at is not None:
            copy = copy.copy()
            copy[self.n_at] = ord("N")
        self.contig = np.concatenate([random_dna(rng, 0 if self.cut_left else self.left, 0.5), copy,
                                      random_dna(rng, 0 if self.cut_right else self.right, 0.5)])  # fmt: skip
        return self


def sub(*positions):
    def edit(g, rng):
        out = g.copy()
        for p in positions:
            out[p] = _other(out[p])
        return out

    return edit


def head_mismatch(n):  # the first n bases differ: the local path starts at row n
    return sub(*range(n))


def tail_mismatch(n):  # the last n bases differ: the path ends at row len - n - 1
    def edit(g, rng):
        return sub(*range(len(g) - n, len(g)))(g, rng)

    return edit


def indels(*events):
    """events: (kind, size, gene offset); "ins" = bases the contig has and the gene lacks, "del" = gene bases the contig lacks"""

    def edit(g, rng):
        parts, at = [], 0
        for kind, size, x in sorted(events, key=lambda e: e[2]):
            parts.append(g[at:x])
            if kind == "ins":  # (its ends differ from the gene bases beside them: the gap cannot slide)
                new = random_dna(rng, size, 0.5)
                new[0] = next(c for c in b"ACGT" if c not in (g[x], g[x - 1] if size == 1 else g[x]))
                new[-1] = next(c for c in b"ACGT" if c not in (g[x - 1], g[x] if size == 1 else g[x - 1]))
                parts.append(new)
                at = x
            else:
                at = x + size
        parts.append(g[at:])
        return np.concatenate(parts)

    return edit


# Where the features fall (checked on the oracle's tasks and the yardstick's paths by test_cases_reach_what_they_are_for): a copy
# planted behind a flank gets a 16-diagonal band whose path runs on band index 7 or 8, so a cell of row r lies on step r + 1 or
# r + 2, and the last cell of a 1-base gap after gene offset x on step x + 1.
def _one_base_cases():
    out = []
    for step in (64 * 5 + 7, 64 * 5, 63, 64):  # = 7, 0, 63 and 64 (mod 64); the last two on the first boundary between summary words
        for kind in ("ins", "del"):
            out.append(Case(f"{kind}1_step{step}", 600, indels((kind, 1, step - 1)), distinct=(step - 1,), expect=dict(gap_steps=[step])))
    return out


CASES = [
    Case("exact_1100", 1100, expect=dict(plain_words=16, whole=True)),
    *[Case(f"exact_{n}", n, expect=dict(whole=True)) for n in (61, 64, 65, 120, 128, 129)],
    *[Case(f"sub_{n}", n, sub(n // 2)) for n in (61, 64, 65, 120, 128, 129)],
    *_one_base_cases(),
    Case("ins3_lane", 600, indels(("ins", 3, 300)), expect=dict(lane_change=True, n_gaps=1)),
    Case("del3_lane", 600, indels(("del", 3, 300)), expect=dict(lane_change=True, n_gaps=1)),
    Case("off_contig_start", 900, cut_left=400, expect=dict(q0_positive=True)),
    Case("off_contig_end", 900, cut_right=350, expect=dict(ends_at_contig_end=True)),
    Case("head_mismatch_10", 500, head_mismatch(10), expect=dict(start_mid_piece=True)),
    Case("start_first_step", 500, head_mismatch(15), expect=dict(start_step_mod8=0)),
    Case("start_last_step", 500, head_mismatch(14), expect=dict(start_step_mod8=7)),
    Case("end_step_7", 500, tail_mismatch(13), expect=dict(end_step_mod8=7)),
    Case("end_step_2", 500, tail_mismatch(10), expect=dict(end_step_mod8=2)),
    Case("n_in_window", 500, n_at=250, expect=dict(n_on_path=True)),
    # The band rule (kp_spec.h: a cluster's diagonal range + 2 x 15, rounded up) gives 64 diagonals to any range of 2 to 33 and
    # never 32; a jump of 60 diagonals cuts the cluster in two, and the hit is a joined one.  The 128-diagonal class (32 lanes,
    # wave shifts) takes two indels of 30.
    Case("ins10_wide", 1500, indels(("ins", 10, 700)), expect=dict(width=64, n_gaps=1)),
    Case("del10_wide", 1500, indels(("del", 10, 700)), expect=dict(width=64, n_gaps=1)),
    Case("ins25_wide", 1500, indels(("ins", 25, 700)), expect=dict(width=64, n_gaps=1)),
    Case("del25_wide", 1500, indels(("del", 25, 700)), expect=dict(width=64, n_gaps=1)),
    Case("ins60_wide", 1500, indels(("ins", 60, 700))),
    Case("del60_wide", 1500, indels(("del", 60, 700))),
    Case("ins30x2_widest", 1500, indels(("ins", 30, 500), ("ins", 30, 1000)), expect=dict(width=128, n_gaps=2)),
    Case("del30x2_widest", 1500, indels(("del", 30, 500), ("del", 30, 1000)), expect=dict(width=128, n_gaps=2)),
    Case("long_gene", 16000, indels(("ins", 2, 5000), ("del", 3, 11000)), expect=dict(long=True, n_gaps=2)),
]
IDS = [c.name for c in CASES]


def _assembly(case):
    return GenomeAssembly(case.name, Sequences.from_records([SeqRecord("c0", case.contig.tobytes())]))


def _run(genes, packed, summary: bool, cigar=1, **options):
    """(hits, hit offsets, ops, op offsets, per-assembly tasks, per-assembly SW rows, stats) of one batch on a context of its own"""
    before = os.environ.pop("KAPTIVE_AMD_TRACE_SUMMARY", None)
    if not summary:
        os.environ["KAPTIVE_AMD_TRACE_SUMMARY"] = "0"
    try:
        ctx = _native.Context(0)  # (the environment is read here, once per context)
    finally:
        os.environ.pop("KAPTIVE_AMD_TRACE_SUMMARY", None)
        if before is not None:
            os.environ["KAPTIVE_AMD_TRACE_SUMMARY"] = before
    ctx.load_genes(*genes)
    for k, v in options.items():
        ctx.set_option(k, v)
    ctx.set_option("cigar", cigar)
    batch = ctx.batch(packed)
    hits, hoff = batch.align()
    ops, coff = batch.cigars() if cigar else (None, None)
    out = dict(hits=hits, hoff=hoff, ops=ops, coff=coff, tasks=[batch.tasks(i) for i in range(len(packed))],
               rows=[batch.task_results(i) for i in range(len(packed))], stats=batch.stats())  # fmt: skip
    batch.close()
    ctx.close()
    return out


class World:
    """Every case's gene in one database; an assembly per case, or -- one_assembly -- all contigs end to end in a single one"""

    def __init__(self, oracle, cases, seed, one_assembly=None):
        rng = np.random.default_rng(seed)
        self.cases = [c.build(rng) for c in cases]
        self.genes = pack_sequences_flat(Sequences.from_records([SeqRecord(c.name, c.gene.tobytes()) for c in self.cases]))
        if one_assembly:
            whole = Case(one_assembly, 0)
            whole.contig = np.concatenate([c.contig for c in self.cases])
            self.cases = [whole]
        self.packed = [_assembly(c).packed() for c in self.cases]
        self.odb = oracle.OracleDB(*self.genes)
        self.want_hits = [self.odb.align(pa) for pa in self.packed]

        self.credit, self._codes = {}, {}

    def asm_codes(self, i):
        if i not in self._codes:
            self._codes[i] = U.assembly_codes(self.packed[i])
        return self._codes[i]

    def want_rows(self, i, tasks):
        return self.odb.sw(self.packed[i], tasks)


@pytest.fixture(scope="module")
def world(oracle):
    return World(oracle, CASES, 20261)


@pytest.fixture(scope="module")
def on(world):
    return _run(world.genes, world.packed, summary=True)


@pytest.fixture(scope="module")
def off(world):
    return _run(world.genes, world.packed, summary=False)


def _long_gap_credit(world, i, task):
    """n - KP_GAP_LONG for every gap of n > KP_GAP_LONG = 20 columns on the task's path (kp_spec.h: the two-piece gap cost), from
    the yardstick of tests/cigar_util.py"""
    key = (i, int(task["gs"]), int(task["contig"]), int(task["lo"]), int(task["width"]))
    if key not in world.credit:
        _, ops = U.task_yardstick(*world.genes, world.packed[i], world.asm_codes(i), task)
        world.credit[key] = sum(max((int(op) >> 4) - 20, 0) for op in ops if int(op) & 15 != U.M)
    return world.credit[key]


def _check_case(world, run, i, label):
    name = world.cases[i].name
    _same_records(run["hits"][run["hoff"][i] : run["hoff"][i + 1]], world.want_hits[i], f"{name}: hits, {label}")
    tasks, got = run["tasks"][i], run["rows"][i]
    want = world.want_rows(i, tasks)
    assert len(tasks) == len(got) == len(want)
    kept = want[:, 0] >= MIN_DP_SCORE
    # (the oracle's rows carry the score of the best cell; the device's add the credit of gaps longer than 20 columns, as the hits do)
    want[kept, 0] += [_long_gap_credit(world, i, t) for t in tasks[kept]]
    assert np.array_equal(got[kept], want[kept]), f"{name}: SW rows of the traced tasks, {label}\n{got[kept]}\n{want[kept]}"
    assert np.array_equal(got[~kept][:, 0], want[~kept][:, 0]) and not got[~kept][:, 1:].any(), f"{name}: tasks below the cut-off, {label}"


def _same_as_without(on, off, i, name):
    a, b = slice(on["hoff"][i], on["hoff"][i + 1]), slice(off["hoff"][i], off["hoff"][i + 1])
    assert on["hits"][a].tobytes() == off["hits"][b].tobytes(), f"{name}: hits with and without the summaries"
    assert np.array_equal(np.diff(on["coff"][a.start : a.stop + 1]), np.diff(off["coff"][b.start : b.stop + 1])), f"{name}: op counts"
    assert np.array_equal(on["ops"][on["coff"][a.start] : on["coff"][a.stop]], off["ops"][off["coff"][b.start] : off["coff"][b.stop]]), f"{name}: CIGAR ops"


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_case_matches_oracle_and_the_walk_without_summaries(world, on, off, i):
    _check_case(world, on, i, "summaries used")
    _check_case(world, off, i, "summaries ignored")
    _same_as_without(on, off, i, world.cases[i].name)
    assert np.array_equal(on["rows"][i], off["rows"][i])


def _task_rows(task, pa, qlen):
    """kp_task_rows: (q0, r_hi) of a TASK_DTYPE row"""
    cstart = int(pa.ctg_start[task["contig"]])
    cend = cstart + int(pa.ctg_len[task["contig"]])
    lo, width = int(task["lo"]), int(task["width"])
    a = max(cstart - lo - (width - 1), 0) & ~7
    z = max(min(cend - lo, qlen), a)
    return a, z


def _main_task(world, i):
    """(task, oracle row, q0) of the forward-strand task of the case's own gene with the best score"""
    pa = world.packed[i]
    tasks = world.odb.tasks(pa)
    rows = world.odb.sw(pa, tasks)
    mine = [k for k in range(len(tasks)) if int(tasks[k]["gs"]) == 2 * i]
    assert mine, f"{world.cases[i].name}: no band task for the gene"
    k = max(mine, key=lambda k: int(rows[k][0]))
    return tasks[k], rows[k], _task_rows(tasks[k], pa, world.cases[i].length)[0]


def _path(world, i):
    """The path of the case's main task from the yardstick (tests/cigar_util.py): (task, q0, first cell, last cell, the last
    cell of every gap, lane changed across a gap), cells as (row, band index, step)"""
    task, row, q0 = _main_task(world, i)
    out7, ops = U.task_yardstick(*world.genes, world.packed[i], world.asm_codes(i), task)
    assert np.array_equal(out7[1:], row[1:]) and out7[0] == row[0] + _long_gap_credit(world, i, task)
    lo = int(task["lo"])
    cell = lambda r, t: (r, t - lo - r, r - q0 + ((t - lo - r) >> 2))  # noqa: E731
    r, t = int(row[1]), int(row[3])  # the next cell of the path
    first, gaps, lane_change = cell(r, t), [], False
    for op in ops:
        kind, n = int(op) & 15, int(op) >> 4
        if kind == U.M:
            r, t = r + n, t + n
        else:  # I: n cells down the column of the last cell; D: n cells along its row
            before = cell(r - 1, t - 1)
            r, t = (r + n, t) if kind == U.I else (r, t + n)
            gaps.append(cell(r - 1, t - 1))
            lane_change |= before[1] >> 2 != gaps[-1][1] >> 2
    assert (r, t) == (int(row[2]), int(row[4]))
    return task, q0, first, cell(r - 1, t - 1), gaps, lane_change


@pytest.mark.parametrize("i", [k for k, c in enumerate(CASES) if c.expect], ids=[c.name for c in CASES if c.expect])
def test_cases_reach_what_they_are_for(world, i):
    """The oracle's tasks and the yardstick's paths say where each case's path ends, starts and bends: the steps, band class and
    lanes the case is named for.  (CPU work on the shapes above; marked gpu so that it runs with the cases it vouches for.)"""
    case, e = world.cases[i], world.cases[i].expect
    task, q0, first, last, gaps, lane_change = _path(world, i)
    assert int(task["width"]) == e.get("width", 64 if "long" in e or "lane_change" in e else 16), (case.name, int(task["width"]))
    if "whole" in e:
        assert first[0] == 0 and last[0] == case.length - 1 and not gaps
    if "plain_words" in e:  # the skip crosses more than 15 summary words and ends in the piece of row 0
        assert (last[2] >> 6) - (first[2] >> 6) > 15 and first[2] >> 3 == 0
    if "q0_positive" in e:
        assert q0 > 0 and first[0] >= q0
    if "start_mid_piece" in e:
        assert first[0] > 0 and first[2] % 8 not in (0, 7)
    if "start_step_mod8" in e:
        assert first[2] % 8 == e["start_step_mod8"], (case.name, first)
    if "end_step_mod8" in e:
        assert last[2] % 8 == e["end_step_mod8"], (case.name, last)
    if "gap_steps" in e:
        assert [g[2] for g in gaps] == e["gap_steps"], (case.name, gaps)
    if "n_gaps" in e:
        assert len(gaps) == e["n_gaps"], (case.name, gaps)
    if "lane_change" in e:
        assert lane_change, (case.name, gaps)
    if "long" in e:
        assert case.length > 15800
    lo, pa = int(task["lo"]), world.packed[i]
    if "ends_at_contig_end" in e:  # the band's last rows lie past the contig: the fill stops at the contig's end, and so does the path
        assert lo + last[0] + last[1] == int(pa.ctg_start[0]) + int(pa.ctg_len[0]) - 1 and last[0] < case.length - 1
    if "n_on_path" in e:  # an N between the path's ends: the fill flags the task and the walk counts matches base by base, never skipping
        assert (world.asm_codes(i)[lo + first[0] + first[1] : lo + last[0] + last[1]] == 4).sum() == 1


def test_unequal_pair_shares_a_register(oracle):
    """Two tasks only, a long and a short one: the length order pairs them into one register of the packed fill (task X and
    task Y with different numbers of pieces and of summary words)."""
    world = World(oracle, [Case("long_of_pair", 1100, indels(("del", 1, 900))), Case("short_of_pair", 130, sub(40))], 20262, one_assembly="pair")
    on, off = (_run(world.genes, world.packed, summary=s) for s in (True, False))
    # the batch's only two tasks, both of the 16-diagonal class: the first pair of that class's length order, whatever the order
    assert len(on["tasks"][0]) == 2 and (on["tasks"][0]["width"] == 16).all(), on["tasks"][0]
    _check_case(world, on, 0, "summaries used")
    _check_case(world, off, 0, "summaries ignored")
    _same_as_without(on, off, 0, "pair")
    assert len(on["hits"]) == 2


def test_trace_overflow_reruns_to_the_same_results(world, on):
    """The trace buffer started at 1 KiB per assembly: every task's block (pieces and summaries) is counted without being
    stored, the host grows the buffer by what the pass counted and the rerun equals the first run of a roomy buffer."""
    tight = _run(world.genes, world.packed, summary=True, trace_kb_per_asm=1)
    assert tight["stats"]["retries"] >= 1, tight["stats"]
    assert on["stats"]["retries"] == 0, on["stats"]
    assert np.array_equal(tight["hoff"], on["hoff"]) and tight["hits"].tobytes() == on["hits"].tobytes()
    assert np.array_equal(tight["coff"], on["coff"]) and np.array_equal(tight["ops"], on["ops"])
    for i in range(len(world.packed)):
        assert np.array_equal(tight["rows"][i], on["rows"][i]), world.cases[i].name
