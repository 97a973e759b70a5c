"""The four reports derived from a reduction's kept list -- variant records, aligned rows, breakpoint records, allele digests -- share
one layout of the kept and piece rows and one lifetime ("Reports derived from the kept list"; kaptive_amd/csrc/kp_typing.hip).
Each report has a test file of its own for what it computes; this one is about what they share: whichever is asked for first, in
whatever order, each comes out as it does alone and as the restatement of its util module computes it; the next reduction replaces
all of them; every typing group has its own; a reduction that overflowed and ran again is laid out by its last run; and what every
entry point answers where there is nothing to report.  The batch is the smallest that reaches every part of the layout: an assembly
without a kept hit, one with a single kept hit and one locus piece, and one whose locus has a gene cut by a contig end (a breakpoint
record, two pieces) and another gene with a substitution and a one-base deletion."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.pack import pack_sequences_flat
from tests import aligned_util as A
from tests import alleles_util as L
from tests import breakpoints_util as P
from tests import cigar_util as U
from tests import variants_util as V

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
REPORTS = ("variants", "aligned", "breakpoints", "alleles")
ORDERS = [REPORTS[i:] + REPORTS[:i] for i in range(4)] + [REPORTS[::-1]]
SINGLE_LOCUS, SINGLE_GENE = 5, 1  # the second assembly holds this gene of this locus and nothing else of the database
EDITED_GENE, SUB_AT, DEL_AT = 3, 200, 400  # the third assembly's copy of this gene of P.PLANT_LOCUS: a substitution and a one-base deletion
CUT_GENE, CUT_AT = 1, 500  # ... and this one is cut by a contig end, as P.plants cuts it
OTHER_LOCUS = 4  # the third assembly reduced for this locus instead of its own: other flags, another order of the kept list
SMALL_KEPT_CAP = 8  # the smallest kept_cap the rerun tests start a reduction with (tests/test_gpu_parity.py)


def _genomes(db, with_o=None):
    """The three assemblies; ``with_o``: a second database whose first locus the third assembly then carries on a contig of its own."""
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.synth import random_dna

    rng = np.random.default_rng(20261019)
    flank = lambda n=2000: random_dna(rng, n, 0.5)  # noqa: E731

    def asm(name, *contigs):
        return GenomeAssembly(name, Sequences.from_records([SeqRecord(f"{name}_{i}", np.ascontiguousarray(c).tobytes()) for i, c in enumerate(contigs)]))

    def locus(li):
        o, n = int(db.loci.offsets[li]), int(db.loci.lengths[li])
        return np.asarray(db.loci.seqs[o : o + n], np.uint8).copy()

    def gene(li, k):
        gi = int(db.locus_gene_offsets[li]) + k
        assert db.gene_intervals.strands[gi] > 0
        return int(db.gene_intervals.starts[gi]), int(db.gene_intervals.ends[gi])

    s, e = gene(SINGLE_LOCUS, SINGLE_GENE)
    single = asm("single", np.concatenate([flank(), locus(SINGLE_LOCUS)[s:e], flank()]))
    own = locus(P.PLANT_LOCUS)
    s, e = gene(P.PLANT_LOCUS, EDITED_GENE)
    assert e - s > DEL_AT + 100
    own[s + SUB_AT] = next(c for c in b"ACGT" if c != own[s + SUB_AT])
    own = np.delete(own, s + DEL_AT)  # (the edited gene lies behind the cut one: the cut's coordinates stay)
    cs, ce = gene(P.PLANT_LOCUS, CUT_GENE)
    assert ce < s and ce - cs > CUT_AT + 100
    contigs = [np.concatenate([flank(), own[: cs + CUT_AT]]), np.concatenate([own[cs + CUT_AT :], flank()])]
    if with_o is not None:
        o, n = int(with_o.loci.offsets[0]), int(with_o.loci.lengths[0])
        contigs.append(np.concatenate([flank(500), np.asarray(with_o.loci.seqs[o : o + n], np.uint8), flank(500)]))
    return [asm("no_hit", random_dna(rng, 6000, 0.5)), single, asm("split", *contigs)]


class Run:
    """The batch aligned once on a context of its own with the ``variants`` and ``aligned`` options (or without: ``options``), scored
    once per group; ``reduce`` enqueues a reduction, ``fetch`` asks for one report."""

    def __init__(self, dbs, genomes, options=True, **ctx_options):
        from kaptive_amd.engine import Engine
        from kaptive_amd.serotyping import batch as B
        from kaptive_amd.serotyping.core import Serotyper

        self.dbs, self.genomes = dbs, genomes
        self.packed = [g.packed() for g in genomes]
        self.eng = Engine(dbs if len(dbs) > 1 else dbs[0], variants=options, aligned=options)
        for name, v in ctx_options.items():
            self.eng.ctx.set_option(name, v)
        self.typers = [Serotyper(d) for d in dbs]
        self.batch = self.eng.ctx.batch(self.packed)
        self.batch.align_async()
        self.best, self.prm = [], []
        for g, t in enumerate(self.typers):
            scores, counts = self.batch.score(t.min_gene_coverage, g)
            self.best.append(B.choose_best_loci(scores, counts, t._expected_genes_per_locus)[0])
            self.prm.append(self.eng.view(g).typing_params(t))
        self.hits, self.hoff = self.batch.hits()
        if options:
            self.ops, self.coff = self.batch.cigars()
        self.codes = [pack_sequences_flat(d.genes) for d in dbs]

    def reduce(self, best=None, group=0):
        self.batch.reduce_async(self.best[group] if best is None else best, self.prm[group], group)

    def fetch(self, name, group=0):
        return tuple(np.ascontiguousarray(x).tobytes() for x in getattr(self.batch, name)(group))

    def fetch_raw(self, name, group=0):
        return getattr(self.batch, name)(group)

    def alone(self, best=None, group=0, others=()):
        """{report: its bytes}, each fetched alone after a fresh reduction (of ``group``, and of ``others`` before it)."""
        out = {}
        for name in REPORTS:
            for g in (*others, group):
                self.reduce(best if g == group else None, g)
            out[name] = self.fetch(name, group)
        return out

    def close(self):
        self.batch.close()
        self.eng.close()


def _bytes(*arrays):
    return tuple(np.ascontiguousarray(x).tobytes() for x in arrays)


def _typing(run, group=0):
    """the group's summaries and the kept and piece rows they count"""
    sums, kept, pieces = run.batch.typing(group)
    return (sums.tobytes(), *(kept[a, : int(n)].tobytes() for a, n in enumerate(sums["n_kept"])), *(pieces[a, : int(n)].tobytes() for a, n in enumerate(sums["n_pieces"])))


def restated(run, group=0):
    """{report: its bytes} as the restatements of the four util modules give them, from the typing records of the group's current
    reduction, the batch's hit table and its ops."""
    sums, kept, pieces = run.batch.typing(group)
    lo = run.eng.gene_ranges[group][0]
    codes, goff = run.codes[group]
    records, var_off, rows, blocks, n_blocks, bps, bp_off = [], [0], np.zeros(kept.shape, A.ALIGNED_ROW_DTYPE), [], 0, [], [0]
    digests, piece_digests = np.zeros(kept.shape, L.ALLELE_DTYPE), np.zeros(pieces.shape, np.uint64)
    for a, pa in enumerate(run.packed):
        asm, nk, m = U.assembly_codes(pa), int(sums["n_kept"][a]), int(sums["n_pieces"][a])
        h = run.hits[run.hoff[a] : run.hoff[a + 1]].copy()
        h["gene"] -= lo  # (the batch's hit table numbers the genes of all databases; a group's records number its own)
        n_var = 0
        for i in range(nk):
            k = kept[a, i]
            r = V.kept_yardstick(k, h, run.ops, run.coff, int(run.hoff[a]), codes, goff, pa, asm, index=i)
            records.append(r)
            n_var += len(r)
            g = int(k["gene"])
            same = np.flatnonzero((h["gene"] == g) & (h["contig"] == k["contig"]) & (h["strand"] == k["strand"]) & (h["q_start"] == k["q_start"])
                                  & (h["q_end"] == k["q_end"]) & (h["t_start"] == k["t_start"]) & (h["t_end"] == k["t_end"]))  # fmt: skip
            z, c0 = int(run.hoff[a]) + int(same[0]), int(pa.ctg_start[k["contig"]])
            n_gene = int(goff[g + 1] - goff[g])
            row, covered, inserted, n_ins = A.row_from_ops(run.ops[run.coff[z] : run.coff[z + 1]], asm, n_gene, int(k["strand"]), int(k["q_start"]),
                                                           int(k["q_end"]), int(k["t_start"]), c0, c0 + int(pa.ctg_len[k["contig"]]))  # fmt: skip
            b = A.pack_blocks(row)
            rows[a, i] = (n_blocks, n_gene, covered, inserted, n_ins)
            blocks.append(b)
            n_blocks += len(b)
        var_off.append(var_off[-1] + n_var)
        bp = P.restate(kept[a, :nk], pa.ctg_start, pa.ctg_len, asm)
        bps.append(bp)
        bp_off.append(bp_off[-1] + len(bp))
        need = int((kept[a, :nk]["prot_off"] + kept[a, :nk]["prot_len"]).max()) if nk else 0
        prot = run.batch.proteins(a, need, group).tobytes() if need else b""
        digests[a, :nk], piece_digests[a, :m] = L.restate(kept[a, :nk], pieces[a, :m], prot, pa.ctg_start, asm)
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt)  # noqa: E731
    return dict(variants=_bytes(cat(records, _native.VARIANT_DTYPE), np.array(var_off, np.int64)), aligned=_bytes(rows, cat(blocks, np.uint64)),
                breakpoints=_bytes(cat(bps, _native.BREAKPOINT_DTYPE), np.array(bp_off, np.int64)), alleles=_bytes(digests, piece_digests))  # fmt: skip


@pytest.fixture(scope="module")
def db():
    return P.plant_db()


@pytest.fixture(scope="module")
def run(db):
    r = Run([db], _genomes(db))
    yield r
    r.close()


@pytest.fixture(scope="module")
def alone(run):
    """The fresh-alone results of the batch's own best loci, and what the batch holds: computed once, left unchanged."""
    out = run.alone()
    sums, kept, pieces = run.batch.typing()
    assert sums["n_kept"].tolist()[:2] == [0, 1] and sums["n_pieces"].tolist()[:2] == [0, 1], "no kept hit; one kept hit and one piece"
    assert sums["n_kept"][2] > SMALL_KEPT_CAP and sums["n_pieces"][2] >= 2
    records, var_off = run.fetch_raw("variants")
    third = records[var_off[2] : var_off[3]]
    assert (third["kind"] == 0).any() and (third["kind"] != 0).any(), "a substitution and an indel in a kept hit of the third assembly"
    bp, bp_off = run.fetch_raw("breakpoints")
    assert bp_off.tolist() == [0, 0, 0, 1] and bp[0]["kind"] == P.CONTIGS, "the cut gene's record"
    return out


# ---- 1. order independence ----------------------------------------------------------------------------------------------------------------
def test_every_report_alone_equals_its_restatement(run, alone):
    run.reduce()
    assert alone == restated(run)


@pytest.mark.parametrize("order", ORDERS, ids=["-".join(n[:3] for n in o) for o in ORDERS])
def test_any_order_gives_what_each_report_gives_alone(run, alone, order):
    run.reduce()
    got = {name: run.fetch(name) for name in order}
    for name in order:
        assert got[name] == alone[name], f"{name}, asked for in the order {order}"
    assert {name: run.fetch(name) for name in REPORTS} == alone, "asked for again"


# ---- 2. the next reduction replaces all four ------------------------------------------------------------------------------------------------
def test_a_second_reduction_replaces_every_report(run, alone):
    best2 = run.best[0].copy()
    assert best2[2] == P.PLANT_LOCUS != OTHER_LOCUS
    best2[2] = OTHER_LOCUS
    want = run.alone(best2)
    run.reduce()
    assert {name: run.fetch(name) for name in REPORTS} == alone
    run.reduce(best2)
    got = {name: run.fetch(name) for name in REPORTS}
    assert got == want and got == restated(run)
    changed = [name for name in REPORTS if got[name] != alone[name]]
    assert changed, "the other locus changes no report: the batch cannot show a stale one"
    run.reduce()  # ... and back
    assert {name: run.fetch(name) for name in reversed(REPORTS)} == alone


# ---- 3. every typing group has its own -------------------------------------------------------------------------------------------------------
def test_two_groups_keep_their_own_reports(db):
    from kaptive_amd.synth import make_db

    db_o = make_db("kpsc_o", seed=8)
    r = Run([db, db_o], _genomes(db, with_o=db_o))
    try:
        alone = [r.alone(group=0, others=(1,)), r.alone(group=1, others=(0,))]
        for g in (0, 1):
            r.reduce(group=g)
        assert int(r.batch.typing(1)[0]["n_kept"][2]) > 0 and int(r.batch.typing(0)[0]["n_kept"][2]) > 0
        for g in (1, 0, 1):
            assert {name: r.fetch(name, g) for name in REPORTS} == alone[g], f"group {g}"
        assert all(alone[0][name] != alone[1][name] for name in REPORTS)
        for g in (0, 1):
            assert alone[g] == restated(r, g), f"group {g}"
    finally:
        r.close()


# ---- 4. a reduction that overflowed and ran again ------------------------------------------------------------------------------------------
def test_the_layout_is_that_of_the_reductions_last_run(db, run, alone):
    r = Run([db], run.genomes, kept_cap=SMALL_KEPT_CAP)
    try:
        r.reduce()
        got = {name: r.fetch(name) for name in REPORTS}
        assert r.batch.stats()["retries"] > run.batch.stats()["retries"], "the reduction did not overflow"
        run.reduce()
        assert _typing(r) == _typing(run)
        assert got == alone
    finally:
        r.close()


# ---- 5. what the entry points answer where there is nothing to report ---------------------------------------------------------------------
def _answers(ctx, batch):
    """{report: [(code, message) of each of its entry points]}"""
    lib, h, b = _native.lib(), ctx._h, batch._h
    off, n = np.zeros(batch.n_asm + 1, np.int64), C.c_int64(0)
    rows, al, pd = np.zeros((batch.n_asm, 64), _native.ALIGNED_ROW_DTYPE), np.zeros((batch.n_asm, 64), _native.ALLELE_DTYPE), np.zeros((batch.n_asm, 8), np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    calls = dict(
        variants=[lambda: lib.kp_batch_variant_offsets(h, b, p(off)), lambda: lib.kp_batch_variants(h, b, None, C.c_int64(0))],
        aligned=[lambda: lib.kp_batch_aligned_size(h, b, C.byref(n)), lambda: lib.kp_batch_aligned_rows(h, b, p(rows), C.c_int32(64)),
                 lambda: lib.kp_batch_aligned_blocks(h, b, None, C.c_int64(0))],
        breakpoints=[lambda: lib.kp_batch_breakpoint_offsets(h, b, p(off)), lambda: lib.kp_batch_breakpoints(h, b, None, C.c_int64(0))],
        alleles=[lambda: lib.kp_batch_alleles(h, b, p(al), C.c_int32(64), p(pd), C.c_int32(8))],
    )  # fmt: skip
    return {name: [(call(), lib.kp_last_error(h)) for call in entry] for name, entry in calls.items()}


def _all(answers, code, text):
    assert answers and all(rc == code and text in msg for rc, msg in answers), (code, text, answers)


NOT_REDUCED = b"kp_batch_reduce has not run for this group since its hit table was made"


def test_error_outcomes_of_the_entry_points(db, run):
    ctx = run.eng.ctx
    b = ctx.batch(run.packed)
    try:
        got = _answers(ctx, b)  # never aligned
        _all(got["variants"], ESTATE, b"no resident alignment results")
        _all(got["aligned"], EINVAL, b"no aligned rows (aligned without the aligned option")
        b.align_async()
        got = _answers(ctx, b)  # the pass enqueued, not waited for
        _all(got["variants"], ESTATE, b"kp_batch_wait has not completed")
        _all(got["aligned"], EINVAL, b"no aligned rows (aligned without the aligned option")
        _all(got["breakpoints"], EINVAL, b"no breakpoint records: " + NOT_REDUCED)
        _all(got["alleles"], EINVAL, b"no allele digests: " + NOT_REDUCED)
        b.score(run.typers[0].min_gene_coverage)
        got = _answers(ctx, b)  # scored, not reduced
        _all(got["variants"], ESTATE, b"kp_batch_reduce has not been called")
        _all(got["aligned"], EINVAL, b"no aligned rows: " + NOT_REDUCED)
        b.reduce_async(run.best[0], run.prm[0])
        assert all(answers[0][0] == 0 for answers in _answers(ctx, b).values()), "reduced: every report is there"
        b.set_hits(*b.hits())
        got = _answers(ctx, b)  # the table replaced: the ops are gone, which is said before anything about the reduction
        _all(got["variants"], EINVAL, b"no variant records (aligned without the variants option, or its hit table was replaced)")
    finally:
        b.close()
    off = Run([db], run.genomes, options=False)  # aligned without the options and not reduced: the option is named, not the reduction
    try:
        got = _answers(off.eng.ctx, off.batch)
        _all(got["variants"], EINVAL, b"no variant records (aligned without the variants option")
        _all(got["aligned"], EINVAL, b"no aligned rows (aligned without the aligned option")
    finally:
        off.close()
