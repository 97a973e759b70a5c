"""The host stage that feeds one device: files -> reader threads -> packed chunk -> page-locked buffer -> ``Batch`` -> the
engine's typing window -> formatted bytes (``TypingPipeline``).  The command line (``kaptive_amd/cli.py``) and the library
(``Serotyper.tsv_from_files``) both drive it, each with its ``PipelineOptions``.

A chunk with the reader threads is a ``ChunkRead`` whichever way it is read -- a whole chunk in one native call
(``ChunkRead.shard``: TSV / PHA4GE only) or file by file (``ChunkRead.per_file``: the texts are kept) -- and its result is a
``ParsedChunk`` that knows how to become a batch.  Page-locked buffers belong to the ``PinPool``: a chunk takes one, the batch
made of it holds it (``PinPool.held``, recorded by ``ParsedChunk.batch``), and ``PinPool.release`` takes it off again."""

from __future__ import annotations

import os
import threading
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from kaptive_amd import _native
from kaptive_amd._native import REPORTS  # the tables derived from the kept lists: one row per report, every loop below goes over it

FILE_SUFFIX = "kaptive_results"
LOCUS_ROWS_KEY = "locus_rows"  # a chunk's outputs: the ``LocusRows.state()`` of its assemblies (the pair tables); never written to a file


@dataclass(frozen=True)
class PipelineOptions:
    """What a pipeline reads, as data; every default means "off" (the thresholds': those of ``Serotyper``)."""

    threads: int = 0  # reader threads (0 = the CPUs this process is granted)
    read_ahead_share: int = 1  # the device processes of one run share the read-ahead memory: this one gets 1 / share of it
    tsv: bool = False
    pha4ge: bool = False
    json: bool = False
    loci: "Path | None" = None  # directories of the per-assembly fasta files
    genes: "Path | None" = None
    proteins: "Path | None" = None
    paf: bool = False  # every hit with its CIGAR: the alignment passes of this run leave them
    cs: bool = False  # ... and its cs string
    eqx: bool = False
    reports: frozenset = frozenset()  # names of REPORTS: the reductions of this run leave their records
    locus_rows: bool = False  # the run's locus rows: every chunk's go with its outputs (LOCUS_ROWS_KEY)
    max_other_genes: int = 1
    min_completeness: float = 0.5
    below_threshold: bool = False
    partial_edge_tolerance: int = 5
    rescue_flank: "int | None" = None
    rescue_min_score: "int | None" = None


def load_database(path: str):
    from kaptive_amd.db import Database

    p = Path(path)
    if p.suffix in (".gbk", ".gb", ".genbank"):
        from kaptive_amd.db.genbank import database_from_genbank

        return database_from_genbank(p)
    return Database.load(p)


class PinPool:
    """The page-locked buffers of one pipeline: those kept for the chunks still to be read, and the one every batch holds
    until its upload is through.  Reader threads take buffers, the driving thread gives them back."""

    def __init__(self, prefetch: int) -> None:
        self.prefetch = prefetch
        self.kept: list = []  # recycled page-locked buffers
        self.held: dict = {}  # batch -> the buffer its words are uploaded from (the driving thread's alone)
        self.lock = threading.Lock()
        self.need = 0  # the largest buffer asked for so far: smaller ones are not worth keeping
        self.unread = 0  # chunks that have not been handed to the readers yet
        self.janitor = ThreadPoolExecutor(max_workers=1)  # gives page-locked buffers back to the system while the run goes on

    def take(self, n_words: int):
        with self.lock:
            self.need = max(self.need, n_words)
            for i, pb in enumerate(self.kept):
                if len(pb.array) >= n_words:
                    return self.kept.pop(i)
        return _native.PinnedBuffer(n_words + n_words // 8, np.uint32, lazy=True)  # page-locked by ``locked``, once it is full

    def locked(self, pb, n_words: int):
        """``pb`` page-locked -- or, on a host that refuses to register it, a block of the runtime's own with the same words."""
        try:
            pb.lock()
            return pb
        except _native.NativeError:
            eager = _native.PinnedBuffer(len(pb.array), np.uint32)
            eager.array[:n_words] = pb.array[:n_words]
            pb.close()
            return eager

    def chunk_started(self) -> None:
        self.unread -= 1

    def release(self, batch, wait: bool = False) -> None:
        """The batch's page-locked words back to the pool: its upload is through (``wait``: once it is)."""
        pb = self.held.pop(batch, None)
        if pb is None:
            return
        try:
            if wait:
                batch.upload_wait()
        finally:
            self.give_back(pb)

    def give_back(self, pb) -> None:
        """A buffer whose upload is through: kept for one of the chunks still to be read (if it is large enough for
        them), otherwise unlocked and unmapped now, beside the run, rather than by the exiting process (30 ms per 0.8 GB
        either way, but the exit is on the command's clock)."""
        with self.lock:
            if len(pb.array) >= self.need and len(self.kept) < min(self.prefetch + 2, self.unread + self.prefetch + 1):
                self.kept.append(pb)
                return
        try:
            self.janitor.submit(pb.close)
        except RuntimeError:  # (shut down already: the process is ending)
            pass

    def close(self, fast: bool = False) -> None:
        """``fast``: the process is about to exit, which gives every buffer back sooner than closing them one by one."""
        self.janitor.shutdown(wait=not fast, cancel_futures=True)
        if not fast:
            for pb in (*self.kept, *self.held.values()):
                pb.close()
            self.kept, self.held = [], {}


class ParsedChunk:
    """A chunk the readers are through with: ``ids``, ``genomes`` (``None`` when the texts are not kept), and ``batch``."""

    ids: list
    genomes: "list | None" = None

    def batch(self, ctx, pins: PinPool):
        """The chunk on the device (upload enqueued); its page-locked words are the batch's until ``pins.release``."""
        pb, n_words, packed, tables = self._filled(pins)
        pb = pins.locked(pb, n_words)
        batch = ctx.batch(packed, pinned_words=pb.array[:n_words], tables=tables)
        pins.held[batch] = pb
        return batch

    def close(self) -> None:
        """Frees what a chunk that will not become a batch holds."""


class ShardChunk(ParsedChunk):
    """A whole chunk from one native call: the batch's tables and its words in a buffer of the pool, no object per file."""

    def __init__(self, ids, tables, n_words: int, buffer) -> None:
        self.ids, self.tables, self.n_words, self.buffer = ids, tables, n_words, buffer

    def _filled(self, pins):
        pb, self.buffer = self.buffer, None
        return pb, self.n_words, None, self.tables

    def close(self) -> None:
        if self.buffer is not None:
            self.buffer.close()
            self.buffer = None


class FileChunk(ParsedChunk):
    """A chunk read file by file: ``GenomeAssembly`` objects, whose packed words ``copiers`` gathers into a buffer of the pool."""

    def __init__(self, genomes, keep: bool, copiers) -> None:
        self.ids, self.genomes, self._all, self.copiers = [g.id for g in genomes], genomes if keep else None, genomes, copiers

    def _filled(self, pins):
        packed = [g.packed() for g in self._all]
        offs = np.concatenate([[0], np.cumsum([len(pa.words) for pa in packed])]).astype(np.int64)
        pb = pins.take(int(offs[-1]))

        def copy(i):
            pb.array[offs[i] : offs[i + 1]] = packed[i].words

        list(self.copiers.map(copy, range(len(packed))))  # (numpy copies of this size run without the interpreter lock; an executor of their own: the readers' queue holds the next chunks' files)
        return pb, int(offs[-1]), packed, None


def _read_file(path, keep_text: bool):
    from kaptive_amd.core.genome import GenomeAssembly

    g = GenomeAssembly.from_file(path, keep_text=keep_text)
    g.packed()
    return g


def _read_shard(paths, threads: int, pins: PinPool, copiers) -> ParsedChunk:
    """A whole chunk in one native call (TSV-only runs: nothing but the packed form and the assembly names is needed):
    the library's threads map, parse and pack the files and lay out the batch's tables (kp_fasta_ingest_shard); the
    interpreter does nothing per file but derive the assembly's name from the path.  A chunk with a file the library
    could not take goes the per-file way, which knows the fall-backs and raises the reference's errors."""
    from kaptive_amd.core.genome import _FASTA_NAME

    ids, comps = [], []
    for path in paths:
        name = os.path.basename(os.fspath(path))
        m = _FASTA_NAME.search(name)
        if not m:
            raise NotImplementedError(f"Unsupported format: {path}")
        ids.append(name.removesuffix(m.group()))
        comps.append(m.group("compression"))
    shard = _native.FastaShard(paths, comps, threads)
    if shard.failed:
        shard.close()
        return FileChunk([_read_file(path, False) for path in paths], False, copiers)
    # the words go to page-locked memory here, on the reader's side of the pipeline (the driving thread only creates the
    # batch): 0.6 GB per chunk of 512 assemblies, copied by the library's threads
    pb = pins.take(shard.total_words)
    shard.words_into(pb.array, threads)
    chunk = ShardChunk(ids, tuple(np.array(t) for t in shard.tables()), shard.total_words, pb)
    shard.close()
    return chunk


class ChunkRead:
    """One chunk with the reader threads: the futures of its reads, however many, and how their results become the chunk."""

    def __init__(self, futures: list, join) -> None:
        self.futures, self.join = futures, join

    @classmethod
    def per_file(cls, paths, readers, copiers, keep_text: bool) -> "ChunkRead":
        return cls([readers.submit(_read_file, p, keep_text) for p in paths], lambda genomes: FileChunk(genomes, keep_text, copiers))

    @classmethod
    def shard(cls, paths, shard_readers, threads: int, pins: PinPool, copiers) -> "ChunkRead":
        return cls([shard_readers.submit(_read_shard, paths, threads, pins, copiers)], lambda chunks: chunks[0])

    def done(self) -> bool:
        return all(f.done() for f in self.futures)

    def result(self) -> ParsedChunk:
        return self.join([f.result() for f in self.futures])

    def abandon(self) -> None:
        """Cancels what is queued; what a read that is through holds (a shard's buffer) is freed."""
        if not any([f.cancel() for f in self.futures]) and all(f.done() and f.exception() is None for f in self.futures):
            self.result().close()


def _read_ahead_bytes() -> int:
    """How much packed input the readers may hold before the device has taken any (KAPTIVE_AMD_READ_AHEAD_GB; default: a
    quarter of what the machine / the cgroup has available, at most 12 GB)."""
    if v := os.environ.get("KAPTIVE_AMD_READ_AHEAD_GB"):
        return int(float(v) * 2**30)
    avail = 64 * 2**30
    try:
        with open("/proc/meminfo") as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    avail = int(line.split()[1]) * 1024
                    break
        for name in ("/sys/fs/cgroup/memory.max", "/sys/fs/cgroup/memory/memory.limit_in_bytes"):
            if os.path.exists(name):
                with open(name) as f:
                    text = f.read().strip()
                if text.isdigit():
                    avail = min(avail, int(text))
                break
    except (OSError, ValueError):
        pass
    return min(12 * 2**30, avail // 4)


class TypingPipeline:
    """One device's share of ``kaptive assembly``: files -> reader pool -> pinned shard -> the engine's typing window -> bytes.

    The stages run beside each other: while the GPU types chunk k, the reader threads parse and pack chunk k + 1 .. k + 2
    (``kp_fasta_ingest`` releases the interpreter lock), their packed words are copied into page-locked memory and
    uploaded on the copy stream, and chunk k - 1's rows are formatted.  When only the TSV and / or PHA4GE reports are asked for,
    no per-assembly object is ever built: the rows come from ``BatchTyping.tsv()`` (``kp_format_rows``, byte for byte what
    ``KaptiveRow.from_result`` gives) and ``BatchTyping.pha4ge()``, and the files' sequence text is not even kept.  The
    JSON lines (``-j``) come from ``BatchTyping.jsonl()`` (``kp_format_json``) and the records of the per-assembly fasta files
    (``-l``, ``-g``, ``-p``) from ``BatchTyping.fasta()`` (``kp_format_fasta``): they need the files' text but no objects either
    (the reference's writers work on one ``SerotypingResult`` at a time, src/kaptive/serotyping/cli.py:20-114).  The readers
    start with the process: their buffers are plain huge-page memory (``kp_host_reserve``) until a batch is made of them."""

    PREFETCH = 2  # chunks being read / uploaded ahead of the one whose alignment pass is enqueued next

    def __init__(self, options: PipelineOptions, device: int, typer=None, databases=(), chunks=None) -> None:
        """``typer``: a ``Serotyper`` the caller already holds (``Serotyper.tsv_from_files``); otherwise one is made of the
        files ``databases`` (one: a ``Serotyper``, several: a ``MultiSerotyper``) and the options' thresholds.  ``chunks``:
        what ``run`` will be given -- the first of them are handed to the reader threads before the database is loaded and
        the device context created (0.3 s in which nothing else would read a file)."""
        from kaptive_amd import usable_cpus
        from kaptive_amd.serotyping.core import MultiSerotyper, Serotyper

        self.options = o = options
        self.marks = {"pipeline_start": time.perf_counter()}  # (KAPTIVE_AMD_CLI_TIMING: where the time before the first rows goes)
        self.fasta_dirs = {flag: (Path(d), ext) for flag, ext in (("loci", "fna"), ("genes", "ffn"), ("proteins", "faa")) if (d := getattr(o, flag))}
        self.objects = bool(o.json or self.fasta_dirs or o.paf or o.reports)  # the files' text (and contig names) are kept
        self.threads = max(1, o.threads or usable_cpus())  # (the cgroup's quota, not the 256 CPUs a container may see)
        # PREFETCH + 1 chunks are being parsed at any time, each by one native call: the thread budget is shared out among them
        # (measured on the 16-CPU box, threads per call 4 / 6 / 8 / 12 / 16 / 24 / 32: 12.5 / 15.2 / 12.1 / 11.0 / 11.0 / 7.4 / 6.5 k
        # assemblies/s -- a cgroup throttles what oversubscribes its quota)
        self.shard_threads = int(os.environ.get("KAPTIVE_AMD_SHARD_THREADS", 0)) or max(1, -(-self.threads // (self.PREFETCH + 1)))
        self.readers = ThreadPoolExecutor(max_workers=self.threads)
        # whole chunks (TSV-only runs) are parsed PREFETCH + 1 at a time, each by shard_threads native threads, in input order
        self.shard_readers = ThreadPoolExecutor(max_workers=self.PREFETCH + 1)
        self.formatters = ThreadPoolExecutor(max_workers=2)  # a chunk's rows and JSON lines, beside the driving thread
        self.copiers = ThreadPoolExecutor(max_workers=min(4, self.threads))  # object mode: copies into pinned memory (not queued behind reads)
        self.pins = PinPool(self.PREFETCH)
        self._early: list = []  # (k, ChunkRead)
        self._order: list = []
        if chunks is not None:
            chunks = list(chunks)
            # The readers start before the database is loaded and the device context exists (0.4-1 s), and they keep going for
            # as long as the read-ahead budget lasts: the words land in plain huge-page memory (kp_host_reserve: no device
            # runtime involved) that is page-locked when its batch is created.  A run is then as long as reading its files
            # takes, plus what the last chunk needs on the device.
            budget, ahead, sizes = _read_ahead_bytes() // max(1, o.read_ahead_share), 0, {}
            for n, (k, paths) in enumerate(chunks):
                if n >= self.PREFETCH + 1:
                    if self.objects or any(str(p).endswith((".gz", ".bz2", ".xz")) for p in paths):
                        break  # (texts are kept / sizes unknown: no deeper than the steady state reads ahead)
                    try:
                        for p in paths:
                            if p not in sizes:
                                sizes[p] = os.stat(p).st_size
                    except OSError:
                        break
                    ahead += int(sum(sizes[p] for p in paths) * 0.3)  # 2 bits per base and the tables, with head-room
                    if ahead > budget:
                        break
                self._early.append((k, self.submit_read(paths)))
            self.pins.unread = len(chunks) - len(self._early)
        self._own_typer = typer is None
        self._ctx_pool = None
        try:
            if typer is None:
                # the HIP runtime and the device context come up on a thread of their own (0.2 s, interpreter lock released) while this
                # one reads and unpacks the database file (0.12 s): the context is waiting when the typer's engine asks for it
                self._ctx_pool = ThreadPoolExecutor(max_workers=1)
                early_ctx = self._ctx_pool.submit(_native.Context, device)
                dbs = [load_database(p) for p in databases]
                self.marks["database_loaded"] = time.perf_counter()
                kw = dict(max_other_genes=o.max_other_genes, min_completeness=o.min_completeness, allow_below_threshold=o.below_threshold,
                          partial_edge_tolerance=o.partial_edge_tolerance, device=device, ctx=early_ctx, **{r.name: r.name in o.reports for r in REPORTS},
                          **{k: v for k in ("rescue_flank", "rescue_min_score") if (v := getattr(o, k)) is not None})  # fmt: skip
                kw["aligned"] = kw["aligned"] or o.locus_rows  # (the locus rows are made of the aligned rows)
                # several: one pass for all of them; duplicate keywords and too many genes are refused here, before any typing
                typer = MultiSerotyper(dbs, **kw) if len(dbs) > 1 else Serotyper(dbs[0], **kw)
            self.typer = typer
            self.engine = self.typer.engine  # the context is created here, on the thread that will drive it
        except BaseException:
            # a bad database path, no device, no memory: the reads queued above must not be drained (gigabytes of FASTA) by
            # the interpreter's exit hook before the error is reported
            self._abandon_reads()
            raise
        if o.paf:
            self.engine.ctx.set_option("cigar", 1)  # (this run's context only)
            if o.cs or o.eqx:
                self.engine.ctx.set_option("cs", 1)
        self.marks["context_ready"] = time.perf_counter()
        # A run is one typing group per database, and a run without --db is a run with one: every chunk's outputs are
        # ((keyword, outputs), ...), one entry per database in order, and the keyword of the one database of a plain run is None
        # (its files are named as given).  A Serotyper of a MultiSerotyper types the group its engine views.
        several = isinstance(typer, MultiSerotyper)
        self.typers = tuple(typer.serotypers) if several else (typer,)
        self.keywords = tuple(t._db.metadata.keyword for t in self.typers) if several else (None,)

    def _pools(self) -> tuple:
        return (self.readers, self.shard_readers, self.copiers, self.formatters, *([self._ctx_pool] if self._ctx_pool else []))

    def _abandon_reads(self) -> None:
        """Cancel every queued read, drop what finished reads hold (shards' page-locked blocks), keep no worker waiting."""
        for pool in self._pools():
            pool.shutdown(wait=False, cancel_futures=True)
        for _, read in self._early:
            read.abandon()
        self._early = []
        self.pins.close()

    def submit_read(self, paths) -> ChunkRead:
        """One chunk to the reader threads: in one native call (TSV / PHA4GE only), or file by file with the texts kept."""
        if self.objects:
            return ChunkRead.per_file(paths, self.readers, self.copiers, True)
        return ChunkRead.shard(paths, self.shard_readers, self.shard_threads, self.pins, self.copiers)

    def close(self, fast: bool = False) -> None:
        """``fast``: the process is about to exit (the command line): reads are cancelled, nothing is waited for or freed --
        the operating system takes the page-locked memory and the device context back faster than the runtime unwinds them."""
        for pool in self._pools():
            pool.shutdown(wait=not fast, cancel_futures=True)
        if not fast and self._own_typer and self.typer._engine is not None:
            self.typer._engine.close()
        self.pins.close(fast)

    def run(self, chunks):
        """Yields ``(k, ((keyword, outputs), ...))`` for every ``(k, paths)`` of ``chunks``, in order: one entry per database
        in order (``self.keywords``), where ``outputs`` maps "tsv" / "pha4ge" / "json" / ... to the bytes this chunk adds to that
        database's stream.  Per-assembly fasta files are written here: to ``DIR/<keyword>/``, or to ``DIR`` itself for the
        keyword ``None`` of a run without ``--db``."""
        o = self.options
        self._order = []
        groups = tuple(t.engine.group for t in self.typers)  # (a MultiSerotyper's typers view the shared engine, one group each)

        def render(bt, keyword, group, aligned) -> dict:
            out = {}
            if aligned is not None:
                out["paf"] = hits_to_paf(self.engine.view(group), bt.genomes, *aligned, cs_tag=o.cs, eqx=o.eqx)
            for r in REPORTS:
                if r.name in o.reports:
                    out[r.name] = getattr(bt, r.tsv)()
            if o.locus_rows:  # (a payload for the parent to merge, not bytes for a file; no --aligned table is made of the rows)
                from kaptive_amd.distances import LocusRows

                chunk_rows = LocusRows(bt.typer._db)
                chunk_rows.add(bt)
                out[LOCUS_ROWS_KEY] = chunk_rows.state()
            if o.tsv:
                out["tsv"] = bt.tsv()
            if o.pha4ge:
                out["pha4ge"] = bt.pha4ge()
            if o.json:  # one native call per batch (kp_format_json): byte for byte result_to_json of every result
                out["json"] = bt.jsonl()
            if self.fasta_dirs:  # a file per assembly and kind, as the reference writes them; the records come per batch (kp_format_fasta)
                for flag, per_asm in bt.fasta(tuple(self.fasta_dirs)).items():
                    d, ext = self.fasta_dirs[flag]
                    d = d if keyword is None else d / keyword
                    d.mkdir(parents=True, exist_ok=True)
                    for genome, blob in zip(bt.ids, per_asm):
                        (d / f"{genome}_{FILE_SUFFIX}.{ext}").write_bytes(blob)
            return out

        # The rows of a chunk are rendered beside the driving thread (the native formatters release the interpreter lock: 35 MB
        # of JSON per 512 assemblies would otherwise stand between two submissions to the device); they leave in input order.
        rendering: deque = deque()
        done = 0

        def job(bts, aligned) -> tuple:  # every database's records from the one alignment pass of the batch
            return tuple((kw, render(bt, kw, g, aligned)) for kw, g, bt in zip(self.keywords, groups, bts))

        for bts, batch in self.engine._window(self.typers, groups, _ChunkSource(self, chunks)):
            aligned = (*batch.hits(), *batch.cigars(), *(batch.cs() if o.cs or o.eqx else ())) if o.paf else None  # (the batch's results go with it)
            batch.close()  # (waits for whatever of the batch is still in flight: the pinned words are free after it)
            self.pins.release(batch)
            rendering.append(self.formatters.submit(job, bts, aligned))
            while rendering and (rendering[0].done() or len(rendering) > 2):
                yield self._order[done], rendering.popleft().result()
                done += 1
        while rendering:
            yield self._order[done], rendering.popleft().result()
            done += 1


class _ChunkSource:
    """``(batch, ids, genomes)`` per chunk, as an iterator with ``ready()`` (the engine's typing window asks before it would
    wait).  Reads ahead of the device: PREFETCH + 1 chunks are with the reader threads at any time (started by
    ``TypingPipeline.__init__`` -- as many as its read-ahead budget allows -- before the device context even exists); their
    batches are created (uploads enqueued) as soon as the reads are through."""

    def __init__(self, pipe: TypingPipeline, chunks) -> None:
        self.pipe = pipe
        self.it = iter(chunks)
        self._prev = None
        self.reading: deque = deque(pipe._early)  # (k, ChunkRead)
        pipe._early = []
        for _ in self.reading:
            next(self.it)  # (those chunks are already being read)
        while len(self.reading) < pipe.PREFETCH + 1 and self._start_read():
            pass

    def _start_read(self) -> bool:
        try:
            k, paths = next(self.it)
        except StopIteration:
            return False
        self.pipe.pins.chunk_started()
        self.reading.append((k, self.pipe.submit_read(paths)))
        return True

    def ready(self) -> bool:
        """Whether ``next()`` would return without waiting for a read (with nothing left, StopIteration comes at once)."""
        return not self.reading or self.reading[0][1].done()

    def __iter__(self):
        return self

    def __next__(self):
        if not self.reading:
            raise StopIteration
        k, read = self.reading.popleft()
        chunk = read.result()
        self._start_read()
        pipe = self.pipe
        pipe.marks.setdefault("first_chunk_parsed", time.perf_counter())
        batch = chunk.batch(pipe.engine.ctx, pipe.pins)
        pipe.marks.setdefault("first_batch_created", time.perf_counter())
        pipe._order.append(k)
        # the batch before this one has had its upload enqueued for at least a chunk's parse: its page-locked words go back to
        # the pool now, not when its rows are written (a run then page-locks 3 GB instead of 5: a second less to lock at the
        # start and to unlock at exit)
        prev, self._prev = self._prev, batch
        if prev is not None:
            pipe.pins.release(prev, wait=True)
        return batch, chunk.ids, chunk.genomes


def hits_to_paf(engine, genomes, hits, hit_off, ops, cigar_off, cs=None, cs_off=None, cs_tag: bool = False, eqx: bool = False) -> bytes:
    """PAF lines (``--paf``) of a batch's hit table for the database ``engine`` views: its genes' hits of every genome, in
    the table's order, genomes in the batch's order.  Column-wise: the rows of the database are picked by a mask and the
    lines come from one native call (``_native.format_paf``; with ``--cs`` / ``--eqx`` ``_native.format_paf_tags``, which
    takes the batch's cs bytes ``cs`` / ``cs_off`` as well)."""
    from kaptive_amd.core.alignment import Cigars, _ragged_take

    lo, hi = engine.gene_ranges[engine.group]
    keep = (hits["gene"] >= lo) & (hits["gene"] < hi)
    if not keep.all():
        kept_before = np.concatenate([[0], np.cumsum(keep)])
        hit_off = kept_before[hit_off]
        cig = Cigars.from_offsets(ops, cigar_off)[keep]
        ops, cigar_off = cig.data, np.concatenate([[0], np.cumsum(cig.lengths, dtype=np.int64)])
        if cs_off is not None:  # the cs bytes are sliced as the ops are
            cs_off = np.asarray(cs_off, np.int64)
            cs_len = np.diff(cs_off)
            cs = _ragged_take(np.asarray(cs, np.uint8), cs_off[:-1], cs_len, np.flatnonzero(keep))[0]
            cs_off = np.concatenate([[0], np.cumsum(cs_len[keep], dtype=np.int64)])
        hits = hits[keep].copy()
        hits["gene"] -= lo
    first = np.concatenate([[0], np.cumsum([len(g.contigs.ids) for g in genomes])])
    names = [n for g in genomes for n in g.contigs.ids]
    lengths = np.concatenate([np.asarray(g.contigs.lengths, np.int32) for g in genomes]) if genomes else np.zeros(0, np.int32)
    if cs_tag or eqx:
        return _native.format_paf_tags(engine.db.genes.ids, engine.db.genes.lengths, names, lengths, first, hits, hit_off, ops, cigar_off,
                                       cs, cs_off, (_native.PAF_CS if cs_tag else 0) | (_native.PAF_EQX if eqx else 0))
    return _native.format_paf(engine.db.genes.ids, engine.db.genes.lengths, names, lengths, first, hits, hit_off, ops, cigar_off)
