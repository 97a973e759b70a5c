"""The typing window of ``Engine`` (kaptive_amd/engine.py) on stub batches: which call follows which, without a device.

A context keeps ``_native.WORK_SLOTS`` alignment results, so the order in which the engine enqueues alignment passes, reads
scores, enqueues reductions and collects records is part of its correctness.  Every stub appends to one event list; the
expected lists below are what the public methods did before the window had a single statement, and what they do now.

One thing the lists pin that a reader may not expect: the batch the window is working on when it ends -- its scores raised, or
the consumer stopped at the yield that follows its reduction -- is neither waiting nor pending, and the window leaves it to its
context's ``close()``.  What waits (aligned, not scored) and what is pending (reduced, not collected) is closed, in that order."""

from types import SimpleNamespace

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.engine import Engine

W = _native.WORK_SLOTS
SCORES = np.array([[1.0, 3.0], [2.0, 0.5]])  # two assemblies, two loci
COUNTS = np.array([[1, 2], [2, 1]])
BEST = [1, 0]  # argmax of SCORES * (COUNTS / 2) ** 3, row by row


class _Engine(Engine):
    """An engine without a context: ``n_dbs`` databases, seen as database ``group``."""

    def __init__(self, events: list, n_dbs: int = 1, group: int = 0) -> None:
        self.events = events
        self.dbs = [SimpleNamespace(genes=()) for _ in range(n_dbs)]
        self.db, self.group = self.dbs[group], group
        for r in _native.REPORTS:
            setattr(self, r.name, False)
        self.typing_params = self.typing_params  # (``view`` makes a plain Engine of this one's attributes: it takes the stub along)

    def typing_params(self, typer):
        return ("params", typer.name)

    def _collect(self, typer, batch, ids, scores, best, genomes=None, group=None):
        group = self.group if group is None else group
        assert scores is SCORES and best.tolist() == BEST
        self.events.append(("collect", batch.i, group))
        return ("typing", batch.i, group, typer.name, ids, genomes)


class _Batch:
    def __init__(self, i: int, events: list, score_raises: bool = False) -> None:
        self.i, self.events, self.score_raises = i, events, score_raises

    def align_async(self) -> None:
        self.events.append(("align", self.i))

    def score(self, min_cov, group):
        self.events.append(("score", self.i, group))
        assert min_cov == 0.25
        if self.score_raises:
            raise RuntimeError(f"scores of batch {self.i}")
        return SCORES, COUNTS

    def reduce_async(self, best, params, group) -> None:
        assert best.tolist() == BEST
        self.events.append(("reduce", self.i, group, params))

    def close(self) -> None:
        self.events.append(("close", self.i))


def _typer(name: str):
    return SimpleNamespace(name=name, min_gene_coverage=0.25, _expected_genes_per_locus=np.array([2.0, 2.0], np.float32))


class _Source:
    """``(batch, ids, genomes)`` per batch; every item handed out is an event."""

    def __init__(self, batches, events: list) -> None:
        self.it, self.events = iter(batches), events

    def __iter__(self):
        return self

    def __next__(self):
        b = next(self.it)
        self.events.append(("pull", b.i))
        return b, [f"asm{b.i}"], None


class _NeverReady(_Source):
    def ready(self) -> bool:
        self.events.append(("ready?",))
        return False


def _batches(n: int, events: list, raises_at: "int | None" = None) -> list:
    return [_Batch(i, events, score_raises=(i == raises_at)) for i in range(n)]


P = ("params", "t")
# 2 * W + 1 = 7 batches through the window of W = 3 work sets (source events left out: a list has none)
SEVEN = [
    ("align", 0), ("align", 1), ("align", 2),
    ("score", 0, 0), ("reduce", 0, 0, P),
    ("score", 1, 0), ("reduce", 1, 0, P), ("collect", 0, 0),
    ("align", 3), ("score", 2, 0), ("reduce", 2, 0, P), ("collect", 1, 0),
    ("align", 4), ("score", 3, 0), ("reduce", 3, 0, P), ("collect", 2, 0),
    ("align", 5), ("score", 4, 0), ("reduce", 4, 0, P), ("collect", 3, 0),
    ("align", 6), ("score", 5, 0), ("reduce", 5, 0, P), ("collect", 4, 0),
    ("score", 6, 0), ("reduce", 6, 0, P), ("collect", 5, 0),
    ("collect", 6, 0),
]  # fmt: skip


def _without_pulls(events: list) -> list:
    return [e for e in events if e[0] != "pull"]


def test_work_slots_is_what_the_lists_were_recorded_for():
    assert W == 3


def test_stream_slides_the_window_over_more_batches_than_work_slots():
    events: list = []
    eng, typer, batches = _Engine(events), _typer("t"), _batches(2 * W + 1, events)
    got = list(eng.type_stream(typer, _Source(batches, events)))
    assert got == [(("typing", i, 0, "t", [f"asm{i}"], None), batches[i]) for i in range(2 * W + 1)]
    assert events == [
        ("pull", 0), ("align", 0), ("pull", 1), ("align", 1), ("pull", 2), ("align", 2),
        ("score", 0, 0), ("reduce", 0, 0, P),
        ("score", 1, 0), ("reduce", 1, 0, P), ("collect", 0, 0),
        ("pull", 3), ("align", 3), ("score", 2, 0), ("reduce", 2, 0, P), ("collect", 1, 0),
        ("pull", 4), ("align", 4), ("score", 3, 0), ("reduce", 3, 0, P), ("collect", 2, 0),
        ("pull", 5), ("align", 5), ("score", 4, 0), ("reduce", 4, 0, P), ("collect", 3, 0),
        ("pull", 6), ("align", 6), ("score", 5, 0), ("reduce", 5, 0, P), ("collect", 4, 0),
        ("score", 6, 0), ("reduce", 6, 0, P), ("collect", 5, 0),
        ("collect", 6, 0),
    ]  # fmt: skip
    assert _without_pulls(events) == SEVEN
    in_window = 0
    for e in events:  # never more than WORK_SLOTS batches between "alignment enqueued" and "records collected"
        in_window += {"align": 1, "collect": -1}.get(e[0], 0)
        assert 0 <= in_window <= W
    for i in range(2 * W):  # batch i's records are collected after batch i + 1's reduction was enqueued
        assert events.index(("collect", i, 0)) > events.index(("reduce", i + 1, 0, P))


def test_a_source_that_is_not_ready_is_only_waited_for_with_an_empty_window():
    events: list = []
    eng, typer = _Engine(events), _typer("t")
    got = list(eng.type_stream(typer, _NeverReady(_batches(3, events), events)))
    assert [bt[1] for bt, _ in got] == [0, 1, 2]
    one = lambda i: [("pull", i), ("align", i), ("ready?",), ("score", i, 0), ("reduce", i, 0, P), ("ready?",), ("collect", i, 0)]  # noqa: E731
    # (pulled without asking while the window is empty; with a batch in it the source is asked, and the pending batch is
    # collected before the next pull)
    assert events == one(0) + one(1) + one(2)


def test_a_consumer_that_stops_early_leaves_no_waiting_batch_open():
    events: list = []
    eng, typer, batches = _Engine(events), _typer("t"), _batches(2 * W + 1, events)
    stream = eng.type_stream(typer, _Source(batches, events))
    bt, batch = next(stream)
    assert bt[1] == 0 and batch is batches[0]
    stream.close()
    assert events == [
        ("pull", 0), ("align", 0), ("pull", 1), ("align", 1), ("pull", 2), ("align", 2),
        ("score", 0, 0), ("reduce", 0, 0, P),
        ("score", 1, 0), ("reduce", 1, 0, P), ("collect", 0, 0),
        ("close", 2),
    ]  # fmt: skip


def test_an_error_closes_what_waits_and_then_what_is_pending_once_each():
    events: list = []
    eng, typer, batches = _Engine(events), _typer("t"), _batches(2 * W + 1, events, raises_at=2)
    got = []
    with pytest.raises(RuntimeError, match="scores of batch 2"):
        for bt, _ in eng.type_stream(typer, _Source(batches, events)):
            got.append(bt[1])
    assert got == [0]  # (handed to the consumer: not the window's to close)
    assert events == [
        ("pull", 0), ("align", 0), ("pull", 1), ("align", 1), ("pull", 2), ("align", 2),
        ("score", 0, 0), ("reduce", 0, 0, P),
        ("score", 1, 0), ("reduce", 1, 0, P), ("collect", 0, 0),
        ("pull", 3), ("align", 3), ("score", 2, 0),
        ("close", 3), ("close", 1),
    ]  # fmt: skip


def test_every_group_is_scored_before_any_group_is_reduced():
    events: list = []
    eng, typers, batches = _Engine(events, n_dbs=2), (_typer("k"), _typer("o")), _batches(W + 1, events)
    got = list(eng.type_stream_groups(typers, _Source(batches, events)))
    assert got == [((("typing", i, 0, "k", [f"asm{i}"], None), ("typing", i, 1, "o", [f"asm{i}"], None)), batches[i]) for i in range(W + 1)]
    K, O = ("params", "k"), ("params", "o")
    stage = lambda i: [("score", i, 0), ("score", i, 1), ("reduce", i, 0, K), ("reduce", i, 1, O)]  # noqa: E731
    collect = lambda i: [("collect", i, 0), ("collect", i, 1)]  # noqa: E731
    assert events == [
        ("pull", 0), ("align", 0), ("pull", 1), ("align", 1), ("pull", 2), ("align", 2),
        *stage(0),
        *stage(1), *collect(0),
        ("pull", 3), ("align", 3), *stage(2), *collect(1),
        *stage(3), *collect(2),
        *collect(3),
    ]  # fmt: skip


def test_a_wrong_number_of_typers_is_refused_before_the_source_is_touched():
    events: list = []
    eng = _Engine(events, n_dbs=2)
    with pytest.raises(ValueError, match="1 typers for an engine of 2 databases"):
        next(eng.type_stream_groups([_typer("k")], _Source(_batches(2, events), events)))
    assert events == []


def test_a_view_types_its_own_group():
    events: list = []
    eng, typer, batches = _Engine(events, n_dbs=2, group=1), _typer("t"), _batches(2, events)
    got = list(eng.type_stream(typer, _Source(batches, events)))
    assert got == [(("typing", i, 1, "t", [f"asm{i}"], None), batches[i]) for i in range(2)]
    assert events == [
        ("pull", 0), ("align", 0), ("pull", 1), ("align", 1),
        ("score", 0, 1), ("reduce", 0, 1, P),
        ("score", 1, 1), ("reduce", 1, 1, P), ("collect", 0, 1),
        ("collect", 1, 1),
    ]  # fmt: skip


def test_a_list_goes_through_the_same_window_and_is_not_closed():
    events: list = []
    eng, typer, batches = _Engine(events), _typer("t"), _batches(2 * W + 1, events)
    got = eng.type_batches(typer, batches, [[f"asm{i}"] for i in range(2 * W + 1)])
    assert got == [("typing", i, 0, "t", [f"asm{i}"], None) for i in range(2 * W + 1)]
    assert events == SEVEN


def test_a_list_aligned_by_the_caller_is_not_aligned_again():
    events: list = []
    eng, typer, batches = _Engine(events), _typer("t"), _batches(W, events)
    got = eng.type_batches(typer, batches, [[f"asm{i}"] for i in range(W)], aligned=True)
    assert [bt[1] for bt in got] == [0, 1, 2]
    assert events == [
        ("score", 0, 0), ("reduce", 0, 0, P),
        ("score", 1, 0), ("reduce", 1, 0, P), ("collect", 0, 0),
        ("score", 2, 0), ("reduce", 2, 0, P), ("collect", 1, 0),
        ("collect", 2, 0),
    ]  # fmt: skip


def test_more_aligned_batches_than_work_slots_are_refused_before_any_call():
    events: list = []
    eng, typer, batches = _Engine(events), _typer("t"), _batches(W + 1, events)
    with pytest.raises(ValueError, match="WORK_SLOTS"):
        eng.type_batches(typer, batches, [[f"asm{i}"] for i in range(W + 1)], aligned=True)
    assert events == []


def test_the_two_halves_the_benchmark_drives():
    events: list = []
    eng, typer, (b,) = _Engine(events), _typer("t"), _batches(1, events)
    staged = eng.reduce_batches(typer, [b], aligned=True)
    assert events == [("score", 0, 0), ("reduce", 0, 0, P)]
    assert eng.collect_batches(typer, [b], [["asm0"]], staged) == [("typing", 0, 0, "t", ["asm0"], None)]
    assert events == [("score", 0, 0), ("reduce", 0, 0, P), ("collect", 0, 0)]
    # ... and with the scores of every batch read before any reduction is enqueued (several databases, one engine each)
    del events[:]
    two = _batches(2, events)
    scored = eng.score_batches(typer, two)
    assert events == [("score", 0, 0), ("score", 1, 0)]
    assert eng.enqueue_reductions(typer, two, scored) is scored
    assert events == [("score", 0, 0), ("score", 1, 0), ("reduce", 0, 0, P), ("reduce", 1, 0, P)]
    with pytest.raises(ValueError, match="WORK_SLOTS"):
        eng.reduce_batches(typer, _batches(W + 1, events))
    assert len(events) == 4
