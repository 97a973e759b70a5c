"""The host stage in front of the device (``kaptive_amd/pipeline.py``), without a device: the pin pool's rules, the two kinds
of chunk reads behind one interface, the options the command line makes, and what the module may import."""

import dataclasses
import gzip
import subprocess
import sys
import threading
from concurrent.futures import Future, ThreadPoolExecutor
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd import pipeline as P
from kaptive_amd.core.genome import GenomeAssembly
from kaptive_amd.synth import make_assembly, make_db

ROOT = Path(__file__).resolve().parent.parent


class StubBuffer:
    """What the pool needs of a ``PinnedBuffer``: ``array``, ``lock``, ``close``."""

    closed: list = []  # (reset by the fixture below)

    def __init__(self, n_items, dtype=np.uint32, lazy=False, refuse_lock=False) -> None:
        self.array, self.lazy, self.refuse_lock = np.zeros(n_items, dtype), lazy, refuse_lock

    def lock(self) -> None:
        if self.refuse_lock:
            raise _native.NativeError("kp_host_lock failed")

    def close(self) -> None:
        StubBuffer.closed.append(self)


class StubBatch:
    def __init__(self, **fields) -> None:
        self.__dict__.update(fields)


class StubPool(P.PinPool):
    """A pool of stub buffers that registers nothing."""

    def take(self, n_words):
        return StubBuffer(n_words)

    def locked(self, pb, n_words):
        return pb


@pytest.fixture(autouse=True)
def _no_closes_yet():
    StubBuffer.closed = []


def _settled(pool) -> list:
    """The buffers closed so far, the janitor's included."""
    pool.janitor.shutdown(wait=True)
    return StubBuffer.closed


def test_pin_pool_keeps_at_most_prefetch_plus_one_when_nothing_is_left_to_read():
    pool = P.PinPool(prefetch=2)
    assert pool.unread == 0
    buffers = [StubBuffer(100) for _ in range(4)]
    for pb in buffers:
        pool.give_back(pb)
    assert pool.kept == buffers[:3] and _settled(pool) == [buffers[3]]


def test_pin_pool_holds_one_more_while_chunks_are_still_to_be_read():
    pool = P.PinPool(prefetch=2)
    pool.unread = 5  # min(PREFETCH + 2, unread + PREFETCH + 1) = 4
    buffers = [StubBuffer(100) for _ in range(5)]
    for pb in buffers:
        pool.give_back(pb)
    assert pool.kept == buffers[:4] and _settled(pool) == [buffers[4]]
    for _ in range(5):
        pool.chunk_started()
    assert pool.unread == 0


def test_pin_pool_closes_a_buffer_smaller_than_the_largest_request():
    pool = P.PinPool(prefetch=2)
    big = pool.take(1000)
    try:
        assert len(big.array) == 1000 + 1000 // 8 and not big.locked  # a fresh lazy buffer, with head-room
        small = StubBuffer(999)
        pool.give_back(small)
        pool.give_back(big)
        assert pool.kept == [big]
        assert pool.take(1200) is not big  # (does not fit: 1125 words)
        assert pool.take(1100) is big and pool.kept == []  # a kept buffer that fits goes before a new one
        assert _settled(pool) == [small]
    finally:
        big.close()


def test_pin_pool_takes_the_first_kept_buffer_that_fits():
    pool = P.PinPool(prefetch=2)
    a, b, c = StubBuffer(10), StubBuffer(30), StubBuffer(40)
    pool.kept = [a, b, c]
    assert pool.take(20) is b and pool.kept == [a, c] and pool.need == 20


def test_pin_pool_copies_into_an_eager_block_when_registering_is_refused(monkeypatch):
    monkeypatch.setattr(P._native, "PinnedBuffer", StubBuffer)
    pool = P.PinPool(prefetch=2)
    lazy = StubBuffer(16, refuse_lock=True)
    lazy.array[:] = np.arange(16)
    got = pool.locked(lazy, 10)
    assert got is not lazy and not got.lazy and len(got.array) == 16 and np.array_equal(got.array[:10], np.arange(10))
    assert StubBuffer.closed == [lazy]
    fine = StubBuffer(16)
    assert pool.locked(fine, 10) is fine and StubBuffer.closed == [lazy]


def test_pin_pool_gives_a_batchs_buffer_back_once_and_closes_what_is_left():
    waits = []
    batch, other = StubBatch(upload_wait=lambda: waits.append(1)), StubBatch()
    pool = P.PinPool(prefetch=2)
    pb, pb2 = StubBuffer(8), StubBuffer(8)
    pool.held = {batch: pb, other: pb2}
    pool.release(batch, wait=True)
    pool.release(batch, wait=True)  # (nothing held any more: no wait, nothing given back twice)
    assert waits == [1] and pool.kept == [pb] and pool.held == {other: pb2}
    pool.close()
    assert StubBuffer.closed == [pb, pb2] and pool.kept == [] and pool.held == {} and pool.janitor._shutdown


@pytest.fixture(scope="module")
def fasta_files(tmp_path_factory):
    """Three small assemblies as files, the second gzip-compressed."""
    root = tmp_path_factory.mktemp("pipeline_cpu")
    db = make_db("kpsc_k", seed=7, n_loci=3)
    paths = []
    for i in range(3):
        data = make_assembly(db, seed=70 + i, length=90_000 + 5_000 * i, median_contigs=3 + i, n_run=4 * i).contigs.to_fasta()
        p = root / f"asm{i}.fasta{'.gz' if i == 1 else ''}"
        p.write_bytes(gzip.compress(data) if i == 1 else data)
        paths.append(str(p))
    return paths


class StubContext:
    def batch(self, packed, pinned_words=None, tables=None):
        return StubBatch(packed=packed, words=pinned_words.copy(), tables=tables)


def test_both_chunk_kinds_give_the_same_chunk(fasta_files):
    pool = StubPool(prefetch=2)
    with ThreadPoolExecutor(3) as readers, ThreadPoolExecutor(1) as shard_readers, ThreadPoolExecutor(2) as copiers:
        reads = (P.ChunkRead.per_file(fasta_files, readers, copiers, False), P.ChunkRead.shard(fasta_files, shard_readers, 2, pool, copiers),
                 P.ChunkRead.per_file(fasta_files, readers, copiers, True))  # fmt: skip
        per_file, shard, kept = (r.result() for r in reads)
        assert all(r.done() for r in reads)
        assert isinstance(per_file, P.FileChunk) and isinstance(shard, P.ShardChunk) and isinstance(kept, P.FileChunk)
        assert per_file.ids == shard.ids == kept.ids == ["asm0", "asm1", "asm2"]
        assert per_file.genomes is None and shard.genomes is None and [g.id for g in kept.genomes] == kept.ids
        ctx = StubContext()
        a, b = per_file.batch(ctx, pool), shard.batch(ctx, pool)
    assert len(a.words) and np.array_equal(a.words, b.words)  # the same packed words, back to back
    assert a.tables is None and len(a.packed) == 3 and b.packed is None
    assert np.array_equal(b.tables[0], np.concatenate([[0], np.cumsum([len(pa.words) for pa in a.packed])]))  # asm_word_off
    assert set(pool.held) == {a, b} and shard.buffer is None  # recorded by the code that made the batches
    shard.close()
    assert StubBuffer.closed == []  # (the batch's now: not the chunk's to free)


def test_a_chunk_read_is_done_only_when_all_its_reads_are_through():
    futures = [Future(), Future()]
    read = P.ChunkRead(futures, lambda results: results)
    assert not read.done()
    futures[1].set_result("b")
    assert not read.done()
    futures[0].set_result("a")
    assert read.done() and read.result() == ["a", "b"]


def test_abandon_frees_a_finished_shard_read_and_cancels_an_unfinished_one(fasta_files):
    pool, gate = StubPool(prefetch=2), threading.Event()
    with ThreadPoolExecutor(1) as shard_readers, ThreadPoolExecutor(1) as copiers:
        finished = P.ChunkRead.shard(fasta_files, shard_readers, 2, pool, copiers)
        buffer = finished.result().buffer
        shard_readers.submit(gate.wait, 5)  # the one reader is busy: what follows stays queued
        queued = P.ChunkRead.shard(fasta_files, shard_readers, 2, pool, copiers)
        assert finished.done() and not queued.done() and StubBuffer.closed == []
        finished.abandon()
        queued.abandon()
        gate.set()
    assert StubBuffer.closed == [buffer] and all(f.cancelled() for f in queued.futures)


def test_a_shard_with_a_file_the_library_refuses_goes_the_per_file_way(fasta_files, tmp_path):
    """The truncated gzip of test_from_files_equals_from_file: the shard reader raises a ``ValueError`` as ``GenomeAssembly.from_files``
    does -- the one of the per-file reader it fell back to, which names the file."""
    bad = tmp_path / "cut.fasta.gz"
    bad.write_bytes(gzip.compress(b">x\nACGT\n")[:12])
    paths = [fasta_files[0], str(bad)]
    with pytest.raises(ValueError) as of_files:
        GenomeAssembly.from_files(paths)
    with pytest.raises(ValueError) as of_file:
        GenomeAssembly.from_file(bad)
    with ThreadPoolExecutor(1) as copiers, pytest.raises(ValueError) as got:
        P._read_shard(paths, 2, StubPool(prefetch=2), copiers)
    assert type(got.value) is type(of_files.value) is ValueError and str(got.value) == str(of_file.value) and str(bad) in str(got.value)
    assert StubBuffer.closed == []  # (no buffer was taken for the chunk)


def _options(*flags):
    from kaptive_amd.cli import build_parser, pipeline_options

    return pipeline_options(build_parser().parse_args(["assembly", "db.npz", "g.fasta", *flags]))


def test_every_output_flag_sets_exactly_its_fields():
    from kaptive_amd.cli import PAIR_TABLES

    base = _options()
    assert base == P.PipelineOptions(tsv=True)  # (-o defaults to stdout)
    assert P.PipelineOptions() == P.PipelineOptions(tsv=False, reports=frozenset(), locus_rows=False, loci=None)  # defaults mean "off"
    cases = [
        (["-o", "r.tsv"], {}),
        (["--pha4ge", "r.pha4ge"], {"pha4ge": True}),
        (["-j", "r.jsonl"], {"json": True}),
        (["-l", "loci"], {"loci": Path("loci")}),
        (["-g", "genes"], {"genes": Path("genes")}),
        (["-p", "prot"], {"proteins": Path("prot")}),
        (["--paf", "r.paf"], {"paf": True}),
        (["--paf", "r.paf", "--cs"], {"paf": True, "cs": True}),
        (["--paf", "r.paf", "--eqx"], {"paf": True, "eqx": True}),
        (["--rescue", "r", "--rescue-flank", "0", "--rescue-min-score", "70"], {"reports": frozenset({"rescue"}), "rescue_flank": 0, "rescue_min_score": 70}),
        (["-t", "5", "--max-other-genes", "2", "--min-completeness", "0.7", "--below-threshold", "--partial-edge-tolerance", "9"],
         {"threads": 5, "max_other_genes": 2, "min_completeness": 0.7, "below_threshold": True, "partial_edge_tolerance": 9}),
        *[([f"--{r.name}", "table.tsv"], {"reports": frozenset({r.name})}) for r in _native.REPORTS],
        *[([f"--{name.replace('_', '-')}", "table.tsv"], {"locus_rows": True}) for name in PAIR_TABLES],
    ]  # fmt: skip
    assert len(cases) == 11 + len(_native.REPORTS) + len(PAIR_TABLES)
    for flags, fields in cases:
        assert _options(*flags) == dataclasses.replace(base, **fields), flags


def test_the_library_path_asks_for_what_dash_o_alone_asks_for(monkeypatch):
    from kaptive_amd.serotyping.core import _tsv_chunks

    made = []

    class Recorder:
        def __init__(self, options, device, typer=None) -> None:
            made.append((options, device, typer))

        def run(self, chunks):
            return iter(())

        def close(self) -> None:
            made.append("closed")

    monkeypatch.setattr(P, "TypingPipeline", Recorder)
    typer = SimpleNamespace(_device=3)
    assert list(_tsv_chunks(typer, ["a.fasta"], 2, 0)) == []
    assert made == [(_options("-o", "-"), 3, typer), "closed"]


def test_the_pipeline_and_the_library_do_not_import_the_command_line():
    code = ("import sys, kaptive_amd.pipeline, kaptive_amd.serotyping.core\n"
            "assert 'kaptive_amd.cli' not in sys.modules, 'the library imports the command line'\n"
            "assert not hasattr(kaptive_amd.pipeline, 'argparse'), 'the pipeline imports argparse'\n")  # fmt: skip
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(ROOT), timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_failing_pipeline_start_cancels_its_queued_reads(tmp_path, monkeypatch):
    """A bad database (or no device) after the early reads were queued: the constructor shuts its reader pools down and
    cancels what is queued, so that the error is reported at once instead of after every queued FASTA was read by the
    interpreter's exit hook (advisor finding, round 5)."""
    from kaptive_amd.cli import build_parser, pipeline_options

    gate, started = threading.Event(), []

    def slow_shard(paths, *_):
        started.append(paths)
        gate.wait(5)
        raise RuntimeError("reader let go")

    monkeypatch.setattr(P, "_read_shard", slow_shard)
    monkeypatch.setattr(P.TypingPipeline, "PREFETCH", 0)  # one shard reader: every chunk but the first stays queued
    files = []
    for i in range(6):
        f = tmp_path / f"g{i}.fasta"
        f.write_text(">c\nACGT\n")
        files.append(str(f))
    args = build_parser().parse_args(["assembly", str(tmp_path / "missing_db.npz"), *files, "-o", str(tmp_path / "o.tsv")])
    monkeypatch.setenv("KAPTIVE_AMD_READ_AHEAD_GB", "1")
    pipe = P.TypingPipeline.__new__(P.TypingPipeline)
    chunks = [(k, [p]) for k, p in enumerate(files)]
    with pytest.raises((FileNotFoundError, OSError)):
        pipe.__init__(pipeline_options(args), 0, databases=[args.database], chunks=chunks)
    gate.set()
    for pool in (pipe.readers, pipe.shard_readers, pipe.copiers, pipe.formatters, pipe.pins.janitor):
        assert pool._shutdown
        pool.shutdown(wait=True)  # returns at once: nothing is left to drain
    assert len(started) <= 1 and pipe._early == []  # the five queued chunks were cancelled, not read
