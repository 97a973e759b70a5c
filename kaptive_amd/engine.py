"""Engine: a database resident on one GPU, plus the batched entry points built on the C ABI.

This is the host-side replacement for what the reference does per genome inside ``Serotyper.__call__`` before its
reduction starts: build an index, construct an ``Aligner`` and call ``map_batch`` (src/kaptive/serotyping/core.py:
145-155).  Here the database is uploaded once, assemblies go to the device as packed batches, and hit tables come
back as columns.
"""

from __future__ import annotations

from typing import Sequence

import numpy as np

from kaptive_amd import _native
from kaptive_amd.core.alignment import Alignments, Cigars
from kaptive_amd.core.genome import GenomeAssembly
from kaptive_amd.core.pairwise import PairwiseAlignments
from kaptive_amd.core.seq import Sequences
from kaptive_amd.db import Database
from kaptive_amd.pack import pack_sequences_flat


class Engine:
    """One database -- or several that are typed together (K and O loci) -- resident on one GPU.

    With a list of databases the genes of all of them go into one seed index, so a batch is scanned, chained and
    aligned once for all of them (the reference runs one ``map_batch`` per database); every database keeps its own
    typing tables as a *group* of the context and ``view(i)`` gives the engine as database ``i`` sees it.  The
    single-genome entry points (``align``, ``hits_to_alignments``) are those of a one-database engine."""

    def __init__(self, db: "Database | Sequence[Database]", device: int = 0, ctx: "_native.Context | None" = None,
                 cigar: bool = False, cs: bool = False, variants: bool = False, breakpoints: bool = False, alleles: bool = False,
                 aligned: bool = False, rescue: bool = False, rescue_flank: "int | None" = None) -> None:
        """``ctx``: a context of ``device`` the caller created ahead of time (the command line starts the runtime on a thread
        of its own while the database file is still being read); otherwise one is created here.  ``cigar``: alignment passes
        also leave the CIGAR of every hit (``Batch.cigars``; ``align`` then fills ``Alignments.cigars``) -- a second walk of
        every path on the device, off by default because typing never reads them.  ``cs``: they also leave the cs difference
        string of every hit (``Batch.cs``; include/kp_spec.h, CS) and, since those are read off the ops, the CIGARs: ``align``
        fills ``Alignments.cs`` and ``Alignments.cigars``.  ``variants``: every typing path also fetches the variant records of
        the kept hits (``Batch.variants``; include/kp_spec.h, VARIANTS): ``BatchTyping.variants()`` / ``.variants_tsv()``.  They are
        read off the ops, so such passes compute the CIGARs as well.  ``breakpoints``: every typing path also fetches the breakpoint
        records of the kept lists (``Batch.breakpoints``; include/kp_spec.h, BREAKPOINTS): ``BatchTyping.breakpoints()`` /
        ``.breakpoints_tsv()``.  They are read off the kept lists and the contigs; the alignment passes do nothing more for them.
        ``alleles``: every typing path also fetches the allele digests of the kept records and the locus pieces (``Batch.alleles``;
        include/kp_spec.h, ALLELES): ``BatchTyping.alleles()`` / ``.locus_alleles()`` / ``.alleles_tsv()``.  One kernel behind the
        reduction; the alignment passes do nothing more for them either.  ``aligned``: every typing path also fetches the aligned rows
        of the kept hits (``Batch.aligned``; include/kp_spec.h, ALIGNED ROWS): ``BatchTyping.aligned()`` / ``.aligned_codes()`` /
        ``.aligned_tsv()``.  They are read off the ops, so such passes compute the CIGARs as well.  ``rescue``: every typing path
        also fetches the rescue records of the genes the reduction lists as missing (``Batch.rescue``; include/kp_spec.h, RESCUE):
        ``BatchTyping.rescue()`` / ``.rescue_tsv()`` -- every such gene's protein aligned against the six-frame translation of the contig
        around the locus pieces, ``rescue_flank`` bases either side (default ``_native.RESCUE_FLANK``).  Kernels behind the reduction;
        the alignment passes do nothing more for them."""
        dbs = list(db) if isinstance(db, (list, tuple)) else [db]
        self.dbs = dbs
        self.db = dbs[0]
        self.group = 0
        self.device = device
        self.ctx = ctx if ctx is not None else _native.Context(device)
        self.cs = bool(cs)
        self.variants = bool(variants)
        self.breakpoints = bool(breakpoints)
        self.alleles = bool(alleles)
        self.aligned = bool(aligned)
        self.rescue = bool(rescue)
        if rescue_flank is not None and not self.rescue:
            raise ValueError("rescue_flank needs rescue=True")
        self.cigar = bool(cigar) or self.cs or self.variants or self.aligned
        if self.cigar:
            self.ctx.set_option("cigar", 1)
        if self.cs:
            self.ctx.set_option("cs", 1)
        if self.variants:
            self.ctx.set_option("variants", 1)
        if self.aligned:
            self.ctx.set_option("aligned", 1)
        if self.rescue:
            self.ctx.set_option("rescue", 1)
            if rescue_flank is not None:
                self.ctx.set_option("rescue_flank", int(rescue_flank))
        for d in dbs:  # KP_MAX_GENE_LEN (include/kp_spec.h): query positions are 16-bit fields of the anchor and hit keys
            too_long = np.flatnonzero(np.asarray(d.genes.lengths) > _native.MAX_GENE_LEN)
            if len(too_long):
                g = int(too_long[0])
                raise ValueError(f"database {d.metadata.keyword!r}: gene {d.genes.ids[g]!r} is {int(d.genes.lengths[g])} bases long; "
                                 f"the aligner handles genes up to {_native.MAX_GENE_LEN} bases (KP_MAX_GENE_LEN) -- "
                                 f"{len(too_long)} gene(s) exceed it")  # fmt: skip
        packed = [pack_sequences_flat(d.genes) for d in dbs]
        counts = [len(d.genes) for d in dbs]
        self.gene_ranges = [(sum(counts[:i]), sum(counts[: i + 1])) for i in range(len(dbs))]
        codes = np.concatenate([c for c, _ in packed]) if len(dbs) > 1 else packed[0][0]
        if len(dbs) > 1:
            base = np.cumsum([0] + [len(c) for c, _ in packed[:-1]])
            off = np.concatenate([o[:-1] + b for (_, o), b in zip(packed, base)] + [[len(codes)]]).astype(packed[0][1].dtype)
        else:
            off = packed[0][1]
        self.ctx.load_genes(codes, off)
        for g, (d, (lo, hi)) in enumerate(zip(dbs, self.gene_ranges)):
            self.ctx.load_typing(d, group=g, gene_lo=lo, gene_hi=hi)
        self._gene_names = tuple(str(i) for i in range(len(self.db.genes)))

    def view(self, group: int) -> "Engine":
        """This engine as database ``group`` sees it: same context and batches, that database's typing group."""
        if group == self.group and self.db is self.dbs[group]:
            return self
        v = object.__new__(Engine)
        v.__dict__.update(self.__dict__)
        v.db, v.group = self.dbs[group], group
        v._gene_names = tuple(str(i) for i in range(len(v.db.genes)))
        return v

    def close(self) -> None:
        self.ctx.close()

    # -- stages -------------------------------------------------------------------------------------------------
    def align_packed(self, packed: list):
        """Hit table for a list of PackedAssembly: (hits, hit_off, stats)."""
        batch = self.ctx.batch(packed)
        try:
            hits, off = batch.align()
            return hits, off, batch.stats()
        finally:
            batch.close()

    def hits_to_alignments(self, genome: GenomeAssembly, hits: np.ndarray, cigars: "Cigars | None" = None,
                           cs: "np.ndarray | None" = None) -> Alignments:
        """``cigars``: the CIGARs of ``hits``, row for row (``Cigars.from_offsets`` of a slice of ``Batch.cigars``); ``cs``:
        their cs strings, an object array of ``bytes``."""
        if len(hits) == 0:
            return Alignments.empty()
        db = self.db
        return Alignments.from_hit_table(
            self._gene_names, genome.contigs.ids,
            q_ids=hits["gene"], q_lengths=db.genes.lengths[hits["gene"]], q_starts=hits["q_start"],
            q_ends=hits["q_end"], t_ids=hits["contig"], t_lengths=genome.contigs.lengths[hits["contig"]],
            t_starts=hits["t_start"], t_ends=hits["t_end"], strands=hits["strand"], block_lens=hits["block_len"],
            matches=hits["matches"], scores=hits["score"], mapqs=hits["mapq"], cigars=cigars, cs=cs,
        )  # fmt: skip

    def align(self, genomes: Sequence[GenomeAssembly]) -> list[Alignments]:
        """One ``Alignments`` per genome; with ``cigar=True`` their ``cigars`` column is filled (every genome's is a view
        of the batch's ops: no loop over the hits)."""
        batch = self.ctx.batch([g.packed() for g in genomes])
        try:
            hits, off = batch.align()
            ops, coff = batch.cigars() if self.cigar else (None, None)
            cs_data, cs_off = batch.cs() if self.cs else (None, None)
        finally:
            batch.close()
        cs_rows = None
        if self.cs:  # one bytes object per hit, as the reference's column holds them
            blob, cs_rows = cs_data.tobytes(), np.empty(len(hits), dtype=object)
            cs_rows[:] = [blob[cs_off[i] : cs_off[i + 1]] for i in range(len(hits))]
        return [self.hits_to_alignments(g, hits[off[i] : off[i + 1]],
                                        Cigars.from_offsets(ops, coff[off[i] : off[i + 1] + 1]) if self.cigar else None,
                                        cs_rows[off[i] : off[i + 1]] if self.cs else None)
                for i, g in enumerate(genomes)]  # fmt: skip

    def protein_aligner(self, queries: Sequences, targets: Sequences) -> PairwiseAlignments:
        if len(queries.offsets) != len(targets.offsets):
            raise ValueError("Query and target batches must have the same number of sequences.")
        if len(queries.offsets) == 0:
            return PairwiseAlignments.empty()
        return PairwiseAlignments.from_table(
            self.ctx.protein_align(queries.seqs, queries.offsets, queries.lengths, targets.seqs, targets.offsets,
                                   targets.lengths)
        )  # fmt: skip

    def typing_params(self, typer) -> "_native.TypingParams":
        db = self.db
        return _native.TypingParams(
            typer.min_gene_coverage, float(np.float32(db.metadata.id_threshold)), db.max_locus_length,
            typer.partial_edge_tolerance,
        )

    def _collect(self, typer, batch, ids, scores, best, genomes=None, group: "int | None" = None):
        """The records of a batch's finished reduction as a ``BatchTyping`` -- with those of every report (``_native.REPORTS``) the
        engine was made for."""
        from kaptive_amd.serotyping import batch as B

        group = self.group if group is None else group
        sums, kept, pieces = batch.typing(group)
        reports = {r.name: getattr(batch, r.fetch)(group) if getattr(self, r.name) else None for r in _native.REPORTS}
        bt = B.BatchTyping(typer, ids, sums, kept, pieces, scores, best, genomes, **reports)
        if getattr(typer, "locus_rows", None) is not None:  # Serotyper(db, distances=True): the run's locus rows grow batch by batch
            typer.locus_rows.add(bt)
        return bt

    # -- typing: one stage step, one window ----------------------------------------------------------------------------------
    # A single database is one typing group: every entry point below goes over ``[(group, typer, params)]``.
    def _groups(self, typers: Sequence, groups: Sequence[int]) -> list:
        return [(g, t, self.view(g).typing_params(t)) for g, t in zip(groups, typers)]

    def _scores(self, batch, groups: list) -> list:
        """``(scores, best loci)`` of every group, in group order (numpy argmax: part of the bit-exact contract)."""
        from kaptive_amd.serotyping import batch as B

        staged = []
        for g, typer, _ in groups:
            scores, counts = batch.score(typer.min_gene_coverage, g)
            best, _, _ = B.choose_best_loci(scores, counts, typer._expected_genes_per_locus)
            staged.append((scores, best))
        return staged

    def _stage(self, batch, groups: list, staged: "list | None" = None) -> list:
        """The stage step of an aligned batch: the scores of every group are read back and its best loci chosen, then every
        group's reduction is enqueued -- in that order, so that no database's scores queue up behind another one's reduction
        kernels.  ``staged``: the scores, where the caller has read them already (``score_batches``)."""
        if staged is None:
            staged = self._scores(batch, groups)
        for (g, _, params), (_, best) in zip(groups, staged):
            batch.reduce_async(best, params, g)
        return staged

    def _window(self, typers: Sequence, groups: Sequence[int], source, align: bool = True, own: bool = True):
        """The typing window: ``source`` yields ``(batch, ids, genomes_or_None)``; what comes out, in the same order, is
        ``(tuple of one BatchTyping per group, batch)``.

        A context keeps the results of its ``_native.WORK_SLOTS`` most recent alignment passes (the work sets rotate at
        ``kp_batch_align``), so at most that many batches are between "alignment enqueued" and "records collected" at any
        time: the next batch is only pulled from ``source`` (created, uploaded, its pass enqueued) when a work set is free for
        it, the oldest aligned batch goes through the stage step, and then the batch before it is collected (its reduction ran
        while this one was being scored) -- or at once, when nothing is waiting.  The stream never waits for the host and no
        pass is displaced before it was read.

        A source may say whether its next item can be had without waiting (``ready()``: the CLI's reader pipeline): the window
        is then only topped up with what is there, and the driver waits for the source only when it has nothing else to do --
        the first chunk's rows leave as soon as its reduction is through, not after two more chunks were read.

        ``align=False``: the caller has enqueued every pass.  ``own``: what is still in the window on the way out (the source
        ran dry, an error, a consumer that stopped early) is closed before the context goes, waiting batches first; what was
        handed on is the caller's to close."""
        from collections import deque

        groups = self._groups(typers, groups)
        depth = _native.WORK_SLOTS
        it = iter(source)
        can_pull = getattr(source, "ready", None)
        live: deque = deque()  # aligned, not yet scored
        pending = None  # reductions enqueued, records not yet collected
        exhausted = False

        def collect(item):
            batch, ids, genomes, staged = item
            return tuple(self._collect(t, batch, ids, scores, best, genomes, g) for (g, t, _), (scores, best) in zip(groups, staged)), batch

        try:
            while live or pending is not None or not exhausted:
                while not exhausted and len(live) + (pending is not None) < depth:
                    if can_pull is not None and (live or pending is not None) and not can_pull():
                        break
                    item = next(it, None)
                    if item is None:
                        exhausted = True
                        break
                    if align:
                        item[0].align_async()
                    live.append(item)
                reduced = None
                if live:
                    batch, ids, genomes = live.popleft()
                    reduced = (batch, ids, genomes, self._stage(batch, groups))
                done, pending = pending, None  # (handed on: no longer the window's)
                if done is not None:
                    yield collect(done)
                pending = reduced
        finally:
            if own:
                for item in (*live, *([pending] if pending is not None else ())):
                    try:
                        item[0].close()
                    except Exception:  # noqa: BLE001
                        pass

    def type_batch(self, typer, batch, ids: Sequence[str], genomes: Sequence[GenomeAssembly] | None = None,
                   aligned: bool = False):
        """Whole typing of a resident batch: alignment and reduction on the device, the numpy float steps, and the
        per-assembly decisions as columns.  Returns a ``BatchTyping``; ``.results()`` / ``.rows()`` materialise objects
        and TSV lines.  ``genomes`` (optional) lets the result objects carry the extracted sequences; ``aligned`` says
        that ``batch.align_async()`` has already been enqueued."""
        if not aligned:
            batch.align_async()
        ((scores, best),) = self._stage(batch, self._groups([typer], [self.group]))
        return self._collect(typer, batch, ids, scores, best, genomes)

    def type_batches(self, typer, batches: Sequence, ids: Sequence[Sequence[str]], aligned: bool = False) -> list:
        """Any number of resident batches through the same context, software-pipelined by the typing window (``_window``);
        the batches stay the caller's.  ``aligned=True`` (the caller already enqueued every pass) is only possible for up to
        WORK_SLOTS batches."""
        if aligned and len(batches) > _native.WORK_SLOTS:
            raise ValueError(f"{len(batches)} batches were aligned up front but a context keeps only {_native.WORK_SLOTS} alignment results "
                             "(WORK_SLOTS); pass aligned=False and let type_batches schedule the passes")  # fmt: skip
        source = ((b, i, None) for b, i in zip(batches, ids))
        return [bts[0] for bts, _ in self._window([typer], [self.group], source, align=not aligned, own=False)]

    def type_stream(self, typer, source):
        """The typing window for a stream whose length is not known in advance (the CLI: batches are made while files are
        still being read).  ``source`` yields ``(batch, ids, genomes_or_None)``; what comes out, in the same order, is
        ``(BatchTyping, batch)`` -- the caller closes the batch."""
        from contextlib import closing

        with closing(self._window([typer], [self.group], source)) as window:  # (a consumer that stops early ends the window too)
            for (bt,), batch in window:
                yield bt, batch

    def type_stream_groups(self, typers: Sequence, source):
        """The typing window for every typing group at once: ``typers[g]`` types database ``g`` of this engine (one per
        database, in order).  What comes out, in order, is ``(tuple of one BatchTyping per group, batch)`` -- the caller closes
        the batch.  Every batch is aligned once."""
        typers = tuple(typers)
        if len(typers) != len(self.dbs):
            raise ValueError(f"{len(typers)} typers for an engine of {len(self.dbs)} databases: one per database, in order")
        yield from self._window(typers, range(len(typers)), source)

    def reduce_batches(self, typer, batches: Sequence, aligned: bool = False) -> list:
        """Scores back, best loci chosen (numpy), reductions enqueued, for up to WORK_SLOTS batches at once.  Returns what
        ``collect_batches`` needs; callers driving several databases put the other database's host work in between
        (bench.py does, one batch at a time).  Longer lists go through ``type_batches``, which slides a window."""
        if len(batches) > _native.WORK_SLOTS:
            raise ValueError(f"{len(batches)} batches at once, but a context keeps only {_native.WORK_SLOTS} alignment "
                             "results (WORK_SLOTS): use type_batches")  # fmt: skip
        if not aligned:
            for b in batches:
                b.align_async()
        return self.enqueue_reductions(typer, batches, self.score_batches(typer, batches))

    def score_batches(self, typer, batches: Sequence) -> list:
        """Locus scores of every batch read back and the best loci chosen.  Cheap on the device; callers with several
        engines score all of them before any reduction is enqueued, as the stage step does for the groups of one."""
        return [self._scores(b, [(self.group, typer, None)])[0] for b in batches]  # (scores need no typing parameters)

    def enqueue_reductions(self, typer, batches: Sequence, staged: list) -> list:
        groups = self._groups([typer], [self.group])
        for b, s in zip(batches, staged):
            self._stage(b, groups, [s])
        return staged

    def collect_batches(self, typer, batches: Sequence, ids: Sequence[Sequence[str]], staged: list) -> list:
        """Second half: fetch the reduction records and finish them column-wise (``BatchTyping``)."""
        return [self._collect(typer, b, i, scores, best) for b, i, (scores, best) in zip(batches, ids, staged)]

    def type_many(self, typer, genomes: Sequence[GenomeAssembly]) -> list:
        """One device submission for all genomes: alignment and reduction both run on the GPU."""
        batch = self.ctx.batch([g.packed() for g in genomes])
        try:
            return self.type_batch(typer, batch, [g.id for g in genomes], genomes).results()
        finally:
            batch.close()
