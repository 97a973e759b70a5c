"""Every grow-and-rerun path of an alignment pass against the CPU oracle (run with -m gpu on an MI355X).

A pass writes into seven device lists whose sizes it guesses: scan candidates, anchor sub-slices, occurrence-cut tables,
band tasks, groups, joins (per band class) and the direction-bit trace.  A list that overflows keeps counting without
storing; kp_batch_wait then grows it, reruns the whole pass, and the context remembers the size for later batches.  Here
each list is started at 1 on its own (every other list generously), then all seven at once, then inside a pipelined
window of batches, and every stage -- anchors after the occurrence cut, band tasks, join records, hit tables -- must equal
the oracle's after the rerun.  A second batch on the same context must need no rerun: the context learnt the size.
"""

import re

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.core.genome import GenomeAssembly
from kaptive_amd.core.seq import SeqRecord, Sequences
from kaptive_amd.pack import pack_sequences_flat
from kaptive_amd.serotyping.core import Serotyper
from kaptive_amd.synth import make_assembly, make_db, random_dna
from tests.test_gpu_parity import _join_assemblies, _repeats, _same_records

pytestmark = pytest.mark.gpu

LISTS = ("anchor_cap", "tasks_per_asm", "cand_cap", "trace_kb_per_asm", "group_cap", "join_cap", "occ_slots")
# room for everything the workload below needs in one pass (test_generous_sizes_need_no_rerun checks that), so that a rerun
# in the cases below is the doing of the one list started at 1
GENEROUS = dict(anchor_cap=1 << 17, tasks_per_asm=4096, cand_cap=1 << 22, trace_kb_per_asm=4096, group_cap=1 << 14,
                join_cap=1 << 12, occ_slots=16, hit_cap=1 << 14)  # fmt: skip
TASK_FIELDS = list(_native.TASK_DTYPE.names)
STATS_LINE = re.compile(r"\[kp_batch_wait\] (\d+) assemblies: (\d+) groups, joins per band class (\d+) (\d+) (\d+) (\d+), "
                        r"(\d+) assemblies needed their mid_occ")  # fmt: skip


@pytest.fixture(scope="module")
def small_db():
    return make_db("kpsc_k", seed=7, n_loci=9)


def _flagged_assemblies(db):
    """Assemblies in which a gene has seeds beyond the occurrence floor, so that each claims a counting table of its own
    (the repeat builder of test_occurrence_cut_matches_oracle): a stretch of a gene in 12 and 30 copies, the first 700
    bases of another in 14, each beside some background, and 30 copies with none.  Only the 2.4 Mbp background of the 30
    copies holds the assembly's mid_occ at the floor, so that the cut drops their seeds."""
    rng = np.random.default_rng(5151)
    pad = lambda n: random_dna(rng, n, 0.5)  # noqa: E731
    g3, g7 = np.frombuffer(db.genes[3].seq, np.uint8), np.frombuffer(db.genes[7].seq, np.uint8)
    gene = lambda g: SeqRecord("gene", np.concatenate([pad(500), g, pad(300)]).tobytes())  # noqa: E731
    asms = []
    for copies, background in ((12, 400_000), (30, 2_400_000)):
        recs = [gene(g3), SeqRecord("copies", _repeats(rng, g3[200:420], copies - 1).tobytes()), SeqRecord("other", np.concatenate([pad(200), g7, pad(100)]).tobytes()),
                SeqRecord("background", pad(background).tobytes())]  # fmt: skip
        asms.append(GenomeAssembly(f"repeat_x{copies}", Sequences.from_records(recs)))
    asms.append(GenomeAssembly("whole_gene_x14", Sequences.from_records([SeqRecord("c", _repeats(rng, g7[:700], 14).tobytes()),
                                                                         SeqRecord("background", pad(300_000).tobytes())])))  # fmt: skip
    asms.append(GenomeAssembly("tiny_x30", Sequences.from_records([gene(g3), SeqRecord("copies", _repeats(rng, g3[200:420], 29).tobytes())])))
    return asms


def _workload(db):
    """One small mixed batch that reaches every stage: joins across mid-size indels, assemblies that need their own mid_occ,
    wide band tasks (an indel every ~60 bases; diverged relatives of database genes) and plain assemblies."""
    small = dict(length=90_000, median_contigs=5, min_contig=200)
    wide = [make_assembly(db, seed=8100, length=120_000, median_contigs=4, min_contig=200, indel_rate=0.016, p_is=0.0),
            make_assembly(db, seed=8101, length=200_000, median_contigs=4, min_contig=200, background="paralog")]  # fmt: skip
    plain = [make_assembly(db, seed=s, **small) for s in (11, 13)]
    return _join_assemblies(db) + _flagged_assemblies(db) + wide + plain


@pytest.fixture(scope="module")
def workload(oracle, small_db):
    """(assemblies, packed, oracle stages of every assembly), the oracle's work done once for all cases"""
    asms = _workload(small_db)
    packed = [a.packed() for a in asms]
    odb = oracle.OracleDB(*pack_sequences_flat(small_db.genes))
    want = [dict(anchors=odb.anchors(pa), tasks=np.sort(odb.tasks(pa), order=TASK_FIELDS), joins=_sorted_joins(odb.joins(pa)),
                 hits=odb.align(pa)) for pa in packed]  # fmt: skip
    return asms, packed, want


def _sorted_joins(j):
    return j[np.lexsort((j["lo"][:, 0], j["contig"], j["gs"]))] if len(j) else j


def _context(db, **options):
    c = _native.Context(0)
    c.load_genes(*pack_sequences_flat(db.genes))
    for name, v in {**GENEROUS, **options}.items():
        c.set_option(name, v)
    return c


def _check_stages(batch, workload):
    """anchors (after the cut), sorted band tasks, sorted join records field by field and hit tables of every assembly"""
    asms, packed, want = workload
    hits, off = batch.align()
    for i, w in enumerate(want):
        name = asms[i].id
        got_a = batch.anchors(i)
        assert np.array_equal(got_a, w["anchors"]), f"anchors of {name}: {len(got_a)} vs {len(w['anchors'])}"
        _same_records(np.sort(batch.tasks(i), order=TASK_FIELDS), w["tasks"], f"tasks of {name}")
        got_j = _sorted_joins(batch.joins(i))
        assert len(got_j) == len(w["joins"]), (name, len(got_j), len(w["joins"]))
        for f in w["joins"].dtype.names:
            assert np.array_equal(got_j[f], w["joins"][f]), (name, f, got_j[f][:2], w["joins"][f][:2])
        _same_records(hits[off[i] : off[i + 1]], w["hits"], f"hits of {name}")
    return batch.stats()


def _two_batches(c, workload):
    """first batch: at least one rerun, every stage equals the oracle; second batch of the same assemblies on the same
    context: no rerun (the context learnt the sizes), every stage again"""
    packed = workload[1]
    first = c.batch(packed)
    stats = _check_stages(first, workload)
    assert stats["retries"] >= 1, f"no rerun: {stats}"
    first.close()
    second = c.batch(packed)
    stats2 = _check_stages(second, workload)
    assert stats2["retries"] == 0, f"the context did not keep what it learnt: {stats2}"
    second.close()
    return stats


def test_generous_sizes_need_no_rerun(small_db, workload, monkeypatch, capfd):
    """The sizes the per-list cases start every other list with are enough for the workload in one pass, and the
    workload reaches every list: groups, joins, assemblies that need their own mid_occ, wide band tasks."""
    monkeypatch.setenv("KAPTIVE_AMD_JOIN_STATS", "1")
    c = _context(small_db)
    batch = c.batch(workload[1])
    stats = _check_stages(batch, workload)
    batch.close()
    c.close()
    assert stats["retries"] == 0, stats
    lines = STATS_LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1, lines
    n_asm, n_group, *joins, n_occ = map(int, lines[0])
    assert n_asm == len(workload[1]) and n_group >= 2 and max(joins) >= 2 and n_occ >= 3, lines[0]
    wide = sum(int((w["tasks"]["width"] > 16).sum()) for w in workload[2])
    assert wide >= 50 and sum(len(w["joins"]) for w in workload[2]) >= 25 and stats["hits"] > 500, (wide, stats)


@pytest.mark.parametrize("name", LISTS)
def test_one_list_started_at_one_reruns_and_matches_oracle(small_db, workload, name):
    c = _context(small_db, **{name: 1})
    _two_batches(c, workload)
    c.close()


def test_anchor_rerun_under_library_sort_matches_oracle(small_db, workload):
    """Compaction of truncated sub-slices (kp_anchor_compact) before the library's radix sort: a path of its own."""
    c = _context(small_db, anchor_cap=1, library_sort=1)
    _two_batches(c, workload)
    c.close()


def test_every_list_started_at_one_cascades_to_the_oracle(small_db, workload):
    """All seven lists at 1 at once: a pass behind an overflow runs on truncated input and can uncover the next overflow
    only in the pass after, so this takes several reruns -- as many as it needs, each growing a list."""
    c = _context(small_db, **{n: 1 for n in LISTS})
    stats = _two_batches(c, workload)
    assert stats["retries"] >= 2, stats
    c.close()


def test_reruns_inside_a_pipelined_window_match_single_calls(small_db, workload):
    """Engine.type_batches over 2 * WORK_SLOTS + 1 batches of a context whose lists all start at 1: the first WORK_SLOTS
    passes are enqueued before the first of them is read, so each reruns while the others are in flight.  Every batch's
    rows equal those of the same batch typed alone by a context with the default sizes."""
    from kaptive_amd.engine import Engine

    asms = workload[0]
    n = 2 * _native.WORK_SLOTS + 1
    groups = [[asms[(5 * b + k) % len(asms)] for k in range(2 + b % 3)] for b in range(n)]
    typer = Serotyper(small_db)
    eng = Engine(small_db)
    for name in LISTS:
        eng.ctx.set_option(name, 1)
    batches = [eng.ctx.batch([g.packed() for g in grp]) for grp in groups]
    retries = {}
    for i, b in enumerate(batches):  # the stats of a pass, read as soon as it is finalised (later passes take its work set)
        def score(*args, _i=i, _b=b, _score=b.score):
            out = _score(*args)
            retries[_i] = _b.stats()["retries"]
            return out

        b.score = score
    ids = [[g.id for g in grp] for grp in groups]
    got = eng.type_batches(typer, batches, ids)
    assert len(got) == n and all(retries[i] >= 1 for i in range(_native.WORK_SLOTS)), retries
    ref = Engine(small_db)
    for b, grp in enumerate(groups):
        one = ref.ctx.batch([g.packed() for g in grp])
        want = ref.type_batch(typer, one, ids[b])
        assert want.rows() == got[b].rows(), f"batch {b}"
        assert want.sums.tobytes() == got[b].sums.tobytes(), f"batch {b}"
        one.close()
    for b in batches:
        b.close()
    ref.close()
    eng.close()
