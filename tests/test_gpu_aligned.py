"""Aligned rows of the kept hits on the device (include/kp_spec.h, ALIGNED ROWS; kaptive_amd/csrc/kp_aligned.hip).  Every row of every
kept record of every assembly is compared, exactly -- blocks and row records --, with (a) the Python restatement of
tests/aligned_util.py run on the device's own ops and (b) a second route that reads no op: the same pass's variant records applied to
the gene's forward codes.  The batches: (1) the 9-locus miniature database with 90 kb assemblies (one of them without a hit),
(2) the join-limits batch of tests/join_limits_util.py (merged I ops of 33 and more columns: whole blocks of GAP in mid-row), (3) the
hand-built batch of tests/cs_util.py (both strands at every word offset, an N run, a gene that holds an n, hits at contig ends),
(4) a hand-built database with a 9000-base gene whose copies carry 296 alternating one-base insertions and deletions (hits of more
than 512 ops: several rounds of the kernel's segment table) and genes of 960, 961, 975, 1024 and 1025 bases.  Then determinism and
lifetime, the option combinations, the option off, a replaced hit table, two databases in one pass, the library and the command
line."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.pack import pack_sequences_flat
from tests import aligned_util as A
from tests import cigar_util as U
from tests import cs_util as S
from tests import join_limits_util as J

pytestmark = pytest.mark.gpu

EINVAL = -1


def restate_batch(bt, hits, hoff, ops, coff, gene_codes, gene_off, packed, gene_lo=0, variants=None):
    """(rows, blocks) as the device lays them out, from the restatement on the ops (``variants`` None) or from the variant records
    ``(records, var_off)`` of the same pass applied to the genes' forward codes."""
    rows = np.zeros(bt.kept.shape, A.ALIGNED_ROW_DTYPE)
    blocks, off = [], 0
    for a, pa in enumerate(packed):
        asm = U.assembly_codes(pa)
        h = hits[hoff[a] : hoff[a + 1]]
        recs = None if variants is None else variants[0][variants[1][a] : variants[1][a + 1]]
        for i in range(int(bt.sums["n_kept"][a])):
            k = bt.kept[a, i]
            g = int(k["gene"]) + gene_lo
            gene = gene_codes[gene_off[g] : gene_off[g + 1]]
            if variants is None:
                same = np.flatnonzero((h["gene"] == g) & (h["contig"] == k["contig"]) & (h["strand"] == k["strand"]) & (h["q_start"] == k["q_start"])
                                      & (h["q_end"] == k["q_end"]) & (h["t_start"] == k["t_start"]) & (h["t_end"] == k["t_end"]))  # fmt: skip
                assert len(same) == 1, f"kept record {k}: {len(same)} hits with its span"
                z = int(hoff[a]) + int(same[0])
                c0 = int(pa.ctg_start[k["contig"]])
                codes, covered, inserted, n_ins = A.row_from_ops(ops[coff[z] : coff[z + 1]], asm, len(gene), int(k["strand"]), int(k["q_start"]), int(k["q_end"]),
                                                                 int(k["t_start"]), c0, c0 + int(pa.ctg_len[k["contig"]]))  # fmt: skip
            else:
                codes, covered, inserted, n_ins = A.row_from_variants(gene, int(k["q_start"]), int(k["q_end"]), recs[recs["kept"] == i])
            b = A.pack_blocks(codes)
            rows[a, i] = (off, len(gene), covered, inserted, n_ins)
            blocks.append(b)
            off += len(b)
    return rows, (np.concatenate(blocks) if blocks else np.zeros(0, np.uint64))


class Typed:
    """One batch aligned and typed on an engine of its own: the typing records, the hit table with its ops, the variant records and
    the aligned rows the options left."""

    def __init__(self, db, genomes, variants=True, aligned=True):
        from kaptive_amd.engine import Engine
        from kaptive_amd.serotyping.core import Serotyper

        self.db, self.genomes = db, genomes
        self.codes, self.off = pack_sequences_flat(db.genes)
        self.packed = [g.packed() for g in genomes]
        self.ids = [g.id for g in genomes]
        self.eng = Engine(db, variants=variants, aligned=aligned)
        self.typer = Serotyper(db)
        self.typer._engine = self.eng
        self.batch = self.eng.ctx.batch(self.packed)
        self.bt = self.eng.type_batch(self.typer, self.batch, self.ids, genomes)
        self.hits, self.hoff = self.batch.hits()
        if variants or aligned:
            self.ops, self.coff = self.batch.cigars()
        if variants:
            self.records, self.var_off = self.bt.variants()
        if aligned:
            self.rows, self.blocks = self.bt.aligned()

    def want(self, bt=None, from_variants=False):
        bt = self.bt if bt is None else bt
        return restate_batch(bt, self.hits, self.hoff, self.ops, self.coff, self.codes, self.off, self.packed,
                             variants=(self.records, self.var_off) if from_variants else None)  # fmt: skip

    def close(self):
        self.batch.close()
        self.eng.close()


def _same(got, want, label, bt):
    rows, blocks = got
    w_rows, w_blocks = want
    assert rows.dtype == _native.ALIGNED_ROW_DTYPE == A.ALIGNED_ROW_DTYPE and blocks.dtype == np.uint64 and rows.shape == bt.kept.shape
    for a in range(rows.shape[0]):
        for i in range(rows.shape[1]):
            if rows[a, i].tobytes() != w_rows[a, i].tobytes():
                raise AssertionError(f"{label}: row record of kept {i} of assembly {a}: device {rows[a, i]} vs {w_rows[a, i]} (kept {bt.kept[a, i]})")
    assert len(blocks) == len(w_blocks), f"{label}: {len(blocks)} blocks on the device, {len(w_blocks)} wanted"
    if blocks.tobytes() != w_blocks.tobytes():
        z = int(np.flatnonzero(blocks != w_blocks)[0])
        a, i = next((a, i) for a in range(rows.shape[0]) for i in range(int(bt.sums["n_kept"][a]))
                    if rows[a, i]["off"] <= z < rows[a, i]["off"] + (rows[a, i]["gene_len"] + 15) // 16)  # fmt: skip
        raise AssertionError(f"{label}: block {z - int(rows[a, i]['off'])} of kept {i} of assembly {a} ({bt.kept[a, i]}): device {int(blocks[z]):016x} "
                             f"vs {int(w_blocks[z]):016x}")  # fmt: skip


def _check(run, label):
    _same((run.rows, run.blocks), run.want(), f"{label}, the restatement on the device's ops", run.bt)
    _same((run.rows, run.blocks), run.want(from_variants=True), f"{label}, the variant records applied to the gene", run.bt)
    for a, n in enumerate(run.bt.sums["n_kept"]):
        assert not np.ascontiguousarray(run.rows[a, int(n) :]).view(np.uint8).any(), "rows beyond the counts are zero"
    return run.rows


def _kept(bt) -> bytes:
    return b"".join(bt.kept[a, : int(n)].tobytes() for a, n in enumerate(bt.sums["n_kept"]))


def _rows_of(run):
    """(kept record, row record, codes) of every kept record of the batch."""
    for a in range(len(run.ids)):
        for i in range(int(run.bt.sums["n_kept"][a])):
            yield run.bt.kept[a, i], run.rows[a, i], run.bt.aligned_codes(a, i)


# ---- the batches -----------------------------------------------------------------------------------------------------------------------
def _mini():
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.synth import make_assembly, make_db, random_dna

    db = make_db("kpsc_k", seed=7, n_loci=9)
    common = dict(length=90_000, median_contigs=5, min_contig=200)
    asms = [make_assembly(db, seed=11, **common), make_assembly(db, seed=13, sub_rate=0.02, indel_rate=1e-3, n_run=50, **common),
            make_assembly(db, seed=17, sub_rate=0.03, indel_rate=2e-3, force_split=True, **common)]  # fmt: skip
    rng = np.random.default_rng(99)
    empty = GenomeAssembly("no_hit", Sequences.from_records([SeqRecord("r0", random_dna(rng, 30_000, 0.5).tobytes())]))
    return db, [asms[0], empty, *asms[1:]]


META = dict(name="hand built", keyword="hand_built", genbank="hand_built.gbk", organism="Klebsiella pneumoniae species complex", taxon=573, antigen="K",
            pathway="Wzx/Wzy", version="synth-2024", id_threshold=82.5, doi=[], owner="kaptive_amd", repo="synthetic", branch="main", contact={},
            phenotype_logic={})  # fmt: skip


def _db_of(genes, names, seed):
    """Genes (ASCII arrays) as a database: one locus per gene, as tests/join_limits_util.py builds its own."""
    from kaptive_amd.db import Database
    from kaptive_amd.synth import random_dna

    rng = np.random.default_rng(seed)
    loci = []
    for i, (name, g) in enumerate(zip(names, genes)):
        seq = np.concatenate([random_dna(rng, 100, 0.5), g, random_dna(rng, 100, 0.5)]).tobytes()
        loci.append(dict(name=f"HB{i + 1}", type=f"HT{i + 1}", extra=False, seq=seq,
                         genes=[dict(start=100, end=100 + len(g), strand=1, gene=f"hb_{name}", product=f"hand-built gene {name}")]))  # fmt: skip
    return Database.from_parts(dict(META), loci)


def _rc(x):
    lut = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGTacgt", b"TGCAtgca"):
        lut[a] = b
    return np.ascontiguousarray(lut[np.asarray(x, np.uint8)][::-1])


LONG_LENS = (9000, 960, 961, 975, 1024, 1025)
EVENTS = 296


def _long():
    """The 9000-base gene with, every 30 bases from offset 60, a one-base insertion and a one-base deletion in turn (296 events), on
    a contig of either strand; the five short genes for the last-block and one-sweep edges, the 1025-base one cut by a contig end on
    each strand."""
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.synth import random_dna

    rng = np.random.default_rng(9000)
    genes = [random_dna(rng, n, 0.5) for n in LONG_LENS]
    db = _db_of(genes, [f"len{n}" for n in LONG_LENS], seed=9001)
    big, parts, at = genes[0], [], 0
    for e in range(EVENTS):
        cut = 60 + 30 * e
        parts.append(big[at:cut])
        if e % 2 == 0:
            parts.append(random_dna(rng, 1, 0.5))  # a base the gene lacks
            at = cut
        else:
            at = cut + 1  # a gene base the contig lacks
    parts.append(big[at:])
    copy = np.concatenate(parts)
    assert len(copy) == len(big)
    sp = lambda n=300: random_dna(rng, n, 0.5)  # noqa: E731
    c1 = np.concatenate([sp(), copy, sp(), genes[1], sp(), _rc(genes[2]), sp(), genes[3], sp(), _rc(genes[4]), sp(), genes[5][:700]])
    c2 = np.concatenate([_rc(genes[5])[:640], sp(), _rc(copy), sp(), _rc(genes[1]), sp(), genes[2], sp(161)])
    asm = GenomeAssembly("long", Sequences.from_records([SeqRecord("fwd", c1.tobytes()), SeqRecord("rev", c2.tobytes())]))
    return db, [asm]


@pytest.fixture(scope="module")
def mini():
    run = Typed(*_mini())
    yield run
    run.close()


@pytest.fixture(scope="module")
def joins():
    run = Typed(J.database(), [s.asm for s in J.join_limit_cases()])
    yield run
    run.close()


@pytest.fixture(scope="module")
def hand():
    seqs, genes = S.hand_genes()
    run = Typed(_db_of(genes, ("big", "sub", "run", "with_n"), seed=4244), [S.hand_assembly(genes)])
    yield run
    run.close()


@pytest.fixture(scope="module")
def long():
    run = Typed(*_long())
    yield run
    run.close()


# ---- 1-4. rows and row records equal both yardsticks ------------------------------------------------------------------------------------
def test_mini_batch(mini):
    _check(mini, "mini")
    a = mini.ids.index("no_hit")
    assert mini.bt.sums["n_kept"][a] == 0 and int(mini.bt.sums["n_kept"].sum()) > 20
    seen = list(_rows_of(mini))
    assert {int(k["strand"]) for k, _, _ in seen} == {-1, 1}, "rows of both strands"
    assert any(k["q_start"] > 0 for k, _, _ in seen), "hits that begin inside the gene"
    assert any((c[int(k["q_start"]) : int(k["q_end"])] == A.GAP).any() for k, _, c in seen), "GAP columns inside [q_start, q_end)"
    assert any(r["inserted"] > 0 for _, r, _ in seen)
    for k, r, c in seen:
        assert len(c) == r["gene_len"] and int((c != A.GAP).sum()) == r["covered"] > 0
        assert (c[: int(k["q_start"])] == A.GAP).all() and (c[int(k["q_end"]) :] == A.GAP).all()
    assert sum(int((c == 4).sum()) for _, _, c in seen) > 0, "the N run shows"
    off = [int(r["off"]) for _, r, _ in seen]
    assert off == np.cumsum([0] + [(int(r["gene_len"]) + 15) // 16 for _, r, _ in seen])[:-1].tolist(), "rows lie back to back in kept-list order"


def test_join_limits_batch(joins):
    _check(joins, "join limits")
    whole = 0
    for k, r, c in _rows_of(joins):
        inside = A.pack_blocks(c)[(int(k["q_start"]) + 15) // 16 : int(k["q_end"]) // 16]
        whole += int((inside == np.uint64(0xFFFF << 48)).sum())
    assert whole >= 10, "merged I ops of 33 and more columns: whole blocks of GAP in mid-row"


def test_hand_built_batch(hand):
    _check(hand, "hand built")
    kept, n = hand.bt.kept[0], int(hand.bt.sums["n_kept"][0])
    assert n >= 4 and {int(s) for s in kept["strand"][:n]} == {-1, 1}
    assert {S.BIG, S.SUB, S.RUN, S.WITH_N} <= {int(g) for g in kept["gene"][:n]}
    for k, r, c in _rows_of(hand):
        if int(k["gene"]) == S.RUN:
            assert np.flatnonzero(c == 4).tolist() == [S.N_RUN_AT, S.N_RUN_AT + 1, S.N_RUN_AT + 2]
        if int(k["gene"]) == S.WITH_N:  # the row says what the contig holds, not what the gene holds
            assert c[S.GENE_N_AT] <= 3
    assert len({int(k["t_start"]) % 16 for k, _, _ in _rows_of(hand)}) == 16, "every word offset"


def test_hits_of_more_than_512_ops_and_the_last_block_edges(long):
    n_ops = []
    for a in range(len(long.ids)):
        h = long.hits[long.hoff[a] : long.hoff[a + 1]]
        for i in range(int(long.bt.sums["n_kept"][a])):
            k = long.bt.kept[a, i]
            same = np.flatnonzero((h["gene"] == k["gene"]) & (h["contig"] == k["contig"]) & (h["t_start"] == k["t_start"]) & (h["t_end"] == k["t_end"])
                                  & (h["q_start"] == k["q_start"]) & (h["q_end"] == k["q_end"]) & (h["strand"] == k["strand"]))  # fmt: skip
            z = int(long.hoff[a]) + int(same[0])
            n_ops.append((int(long.coff[z + 1] - long.coff[z]), int(k["gene"]), int(k["strand"])))
    assert {s for n, g, s in n_ops if g == 0 and n > 512} == {-1, 1}, f"a kept hit of more than 512 ops on either strand: {n_ops}"
    _check(long, "long")
    seen = list(_rows_of(long))
    assert {int(r["gene_len"]) for _, r, _ in seen} == set(LONG_LENS)
    for k, r, c in seen:
        if int(k["gene"]) == 0 and int(k["q_end"]) - int(k["q_start"]) == 9000:
            assert r["n_ins"] == EVENTS // 2 == r["inserted"] and r["covered"] == 9000 - EVENTS // 2
            gaps = np.flatnonzero(c == A.GAP)  # (a gap inside a run of one base may sit anywhere in the run)
            assert len(gaps) == EVENTS // 2 and (np.abs(gaps - np.array([60 + 30 * e for e in range(1, EVENTS, 2)])) <= 8).all()
    cut = [(int(k["strand"]), int(k["q_start"]), int(k["q_end"])) for k, _, _ in seen if int(k["gene"]) == 5]
    assert {s for s, _, _ in cut} == {-1, 1} and all(e - s < 1025 for _, s, e in cut), f"the 1025-base gene, cut by a contig end on each strand: {cut}"


# ---- 5. determinism and lifetime -----------------------------------------------------------------------------------------------------------
def test_determinism_and_lifetime(mini):
    from kaptive_amd.serotyping import batch as B

    ctx = mini.eng.ctx
    first = (mini.rows, mini.blocks)
    again = mini.batch.aligned()  # ask twice
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    b = ctx.batch(mini.packed)
    bt = mini.eng.type_batch(mini.typer, b, mini.ids, mini.genomes)  # align again
    assert _kept(bt) == _kept(mini.bt) and bt.aligned()[0].tobytes() == first[0].tobytes() and bt.aligned()[1].tobytes() == first[1].tobytes()
    # reduce again: an identity threshold above 100 changes the flags of the kept list; the rows are made again for it
    scores, counts = b.score(mini.typer.min_gene_coverage)
    best, _, _ = B.choose_best_loci(scores, counts, mini.typer._expected_genes_per_locus)
    prm = mini.eng.typing_params(mini.typer)
    prm.id_threshold = 101.0
    b.reduce_async(best, prm)
    sums, kept, _ = b.typing()
    rows, blocks = b.aligned()
    bt2 = type("KeptOnly", (), dict(sums=sums, kept=kept))
    _same((rows, blocks), restate_batch(bt2, mini.hits, mini.hoff, mini.ops, mini.coff, mini.codes, mini.off, mini.packed), "after a second reduction", bt2)
    lib = _native.lib()
    small = np.zeros(1, np.uint64)  # a buffer that is too small, a stride that is too small: refused
    assert lib.kp_batch_aligned_blocks(ctx._h, b._h, small.ctypes.data_as(C.c_void_p), C.c_int64(1)) == EINVAL
    r1 = np.zeros((b.n_asm, 1), _native.ALIGNED_ROW_DTYPE)
    assert lib.kp_batch_aligned_rows(ctx._h, b._h, r1.ctypes.data_as(C.c_void_p), C.c_int32(1)) == EINVAL and b"strides too small" in lib.kp_last_error(ctx._h)
    n = C.c_int64(-1)
    assert lib.kp_batch_aligned_size(ctx._h, b._h, C.byref(n)) == 0 and n.value == len(blocks)
    b.close()
    last = mini.batch.aligned()  # the first batch's rows, after all that went through the same context
    assert last[0].tobytes() == first[0].tobytes() and last[1].tobytes() == first[1].tobytes()


# ---- 6. option combinations -----------------------------------------------------------------------------------------------------------------
def test_aligned_alone_variants_alone_and_both_agree(mini):
    alone = Typed(mini.db, mini.genomes, variants=False, aligned=True)
    var = Typed(mini.db, mini.genomes, variants=True, aligned=False)
    try:
        assert alone.eng.cigar and alone.hits.tobytes() == mini.hits.tobytes() and _kept(alone.bt) == _kept(mini.bt)
        assert alone.rows.tobytes() == mini.rows.tobytes() and alone.blocks.tobytes() == mini.blocks.tobytes()
        assert var.records.tobytes() == mini.records.tobytes() and var.var_off.tobytes() == mini.var_off.tobytes()
        assert alone.ops.tobytes() == mini.ops.tobytes() == var.ops.tobytes()
        # asked for in the other order on one batch: rows first, records second
        b = mini.eng.ctx.batch(mini.packed)
        bt = mini.eng.type_batch(mini.typer, b, mini.ids, mini.genomes)
        rows, blocks = b.aligned()
        records, var_off = b.variants()
        assert rows.tobytes() == mini.rows.tobytes() and blocks.tobytes() == mini.blocks.tobytes()
        assert records.tobytes() == mini.records.tobytes() and var_off.tobytes() == mini.var_off.tobytes() and _kept(bt) == _kept(mini.bt)
        b.close()
        with pytest.raises(ValueError):
            alone.batch.variants()
        with pytest.raises(ValueError):
            var.batch.aligned()
    finally:
        alone.close()
        var.close()


# ---- 7. the option off ------------------------------------------------------------------------------------------------------------------
def _refused(ctx, batch, why=b"aligned option"):
    lib = _native.lib()
    n = C.c_int64(0)
    rows, blocks = np.zeros((batch.n_asm, 64), _native.ALIGNED_ROW_DTYPE), np.zeros(8, np.uint64)
    for rc in (lib.kp_batch_aligned_size(ctx._h, batch._h, C.byref(n)), lib.kp_batch_aligned_rows(ctx._h, batch._h, rows.ctypes.data_as(C.c_void_p), C.c_int32(64)),
               lib.kp_batch_aligned_blocks(ctx._h, batch._h, blocks.ctypes.data_as(C.c_void_p), C.c_int64(8))):  # fmt: skip
        assert rc == EINVAL, rc
        assert why in lib.kp_last_error(ctx._h), lib.kp_last_error(ctx._h)
    with pytest.raises(ValueError):
        batch.aligned()


def test_option_off_allocates_nothing_and_changes_nothing(mini):
    off = Typed(mini.db, mini.genomes, variants=False, aligned=False)
    try:
        before = _native.device_allocations()
        second = off.eng.ctx.batch(off.packed)
        bt = off.eng.type_batch(off.typer, second, off.ids, off.genomes)
        assert _native.device_allocations() == before  # a settled context, a repeated batch: nothing grows
        _refused(off.eng.ctx, second)
        assert _native.device_allocations() == before  # ... nor when the rows are asked for in vain
        for call in (bt.aligned, bt.aligned_tsv, lambda: bt.aligned_codes(0, 0)):
            with pytest.raises(ValueError, match="aligned=True"):
                call()
        assert _native.lib().kp_batch_cigars(off.eng.ctx._h, second._h, None, 0) == -4  # (aligned = 0 asks for no CIGARs either)
        # the typing does not depend on the option: hits, records and the report rows, byte for byte
        assert off.hits.tobytes() == mini.hits.tobytes()
        assert bt.sums.tobytes() == mini.bt.sums.tobytes() and _kept(bt) == _kept(mini.bt) == _kept(off.bt)
        assert bt.tsv() == mini.bt.tsv() == off.bt.tsv() and len(bt.tsv().splitlines()) == len(mini.ids)
        second.close()
    finally:
        off.close()


# ---- 8. a replaced hit table ----------------------------------------------------------------------------------------------------------------
def test_replaced_hit_table_refuses_and_the_context_goes_on(mini):
    from kaptive_amd.serotyping import batch as B

    ctx = mini.eng.ctx
    b = ctx.batch(mini.packed)
    bt = mini.eng.type_batch(mini.typer, b, mini.ids, mini.genomes)
    assert bt.aligned()[1].tobytes() == mini.blocks.tobytes()
    hits, hoff = b.hits()
    b.set_hits(hits, hoff)
    _refused(ctx, b)  # not reduced, and nothing describes its paths any more
    scores, counts = b.score(mini.typer.min_gene_coverage)
    best, _, _ = B.choose_best_loci(scores, counts, mini.typer._expected_genes_per_locus)
    b.reduce_async(best, mini.eng.typing_params(mini.typer))
    sums, kept, _ = b.typing()
    assert sums.tobytes() == mini.bt.sums.tobytes()  # the same table reduces to the same records
    _refused(ctx, b)  # ... but the ops are gone
    b.close()
    fresh = ctx.batch(mini.packed)
    bt = mini.eng.type_batch(mini.typer, fresh, mini.ids, mini.genomes)
    assert bt.aligned()[0].tobytes() == mini.rows.tobytes() and bt.aligned()[1].tobytes() == mini.blocks.tobytes() and bt.tsv() == mini.bt.tsv()
    fresh.close()


# ---- 9. two databases in one pass --------------------------------------------------------------------------------------------------------
def test_two_databases_in_one_pass_and_the_group_switch(mini):
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.serotyping.core import MultiSerotyper
    from kaptive_amd.synth import make_db, random_dna

    db_o = make_db("kpsc_o", seed=8)
    rng = np.random.default_rng(78)
    o, n = int(db_o.loci.offsets[0]), int(db_o.loci.lengths[0])
    o_contig = np.concatenate([random_dna(rng, 500, 0.5), np.asarray(db_o.loci.seqs[o : o + n], np.uint8), random_dna(rng, 500, 0.5)])
    genomes = []
    for g in mini.genomes[:2]:  # each with the O locus on a contig of its own
        recs = [SeqRecord(str(i), bytes(g.contigs.seqs[s : s + m])) for i, s, m in zip(g.contigs.ids, g.contigs.offsets, g.contigs.lengths)]
        genomes.append(GenomeAssembly(g.id, Sequences.from_records(recs + [SeqRecord("o_locus", o_contig.tobytes())])))
    ms = MultiSerotyper([mini.db, db_o], aligned=True, variants=True)
    try:
        packed = [g.packed() for g in genomes]
        batch = ms.engine.ctx.batch(packed)
        (groups, _), = list(ms.engine.type_stream_groups(ms.serotypers, [(batch, [g.id for g in genomes], genomes)]))
        assert len(groups) == 2
        hits, hoff = batch.hits()
        ops, coff = batch.cigars()
        codes = [pack_sequences_flat(d.genes) for d in ms.dbs]
        got = []
        for k, bt in enumerate(groups):
            lo = ms.engine.gene_ranges[k][0]
            h = hits.copy()
            h["gene"] -= lo  # (the batch's hit table numbers the genes of all databases; a group's records number its own)
            want = restate_batch(bt, h, hoff, ops, coff, codes[k][0], codes[k][1], packed)
            _same(bt.aligned(), want, f"database {k}", bt)
            _same(bt.aligned(), restate_batch(bt, h, hoff, ops, coff, codes[k][0], codes[k][1], packed, variants=bt.variants()), f"database {k}, variants", bt)
            assert bt.aligned_tsv() == A.format_tsv(bt.ids, [g.contigs.ids for g in genomes], ms.dbs[k].genes.ids, bt.sums["n_kept"], bt.kept, *bt.aligned())
            got.append(bt.aligned())
        assert (groups[1].sums["n_kept"] > 0).all() and groups[0].sums["n_kept"][0] > 0
        # the group switch: each group's rows again, in the other order
        for k in (1, 0, 1):
            rows, blocks = batch.aligned(group=k)
            assert rows.tobytes() == got[k][0].tobytes() and blocks.tobytes() == got[k][1].tobytes()
        batch.close()
    finally:
        ms.close()


# ---- 10. library and command line ----------------------------------------------------------------------------------------------------------
def _write_inputs(db, genomes, tmp_path, name="k.npz"):
    paths = []
    for g in genomes:
        p = tmp_path / f"{g.id}.fasta"
        p.write_bytes(g.contigs.to_fasta())
        paths.append(str(p))
    return str(db.save(tmp_path / name)), paths


def _fasta_seqs(blob: bytes) -> list:
    return [b"".join(rec.split(b"\n")[1:]).lower() for rec in blob.split(b">")[1:]]


def _check_table(table: bytes, gene_dir=None):
    lines = [ln.split(b"\t") for ln in table.splitlines()]
    assert lines[0] == A.HEADER.rstrip(b"\n").split(b"\t") and len(lines) > 20
    n_checked = 0
    for ln in lines[1:]:
        assert len(ln) == 13 and len(ln[12]) == int(ln[6]) and int(ln[9]) == len(ln[12].replace(b"-", b"")) and set(ln[12]) <= set(b"acgtn-")
        assert ln[12][: int(ln[7]) - 1].strip(b"-") == b"" and ln[12][int(ln[8]) :].strip(b"-") == b""
        if gene_dir is not None and int(ln[10]) == 0:  # nothing dropped: the row without its gaps is the gene as -g extracts it
            seqs = _fasta_seqs(next(gene_dir.glob(f"{ln[0].decode()}_*.ffn")).read_bytes())
            assert ln[12].replace(b"-", b"") in seqs, f"{ln[:9]}: its bases are not among the genes -g wrote"
            n_checked += 1
    return n_checked


def test_engine_serotyper_and_command_line(mini, tmp_path):
    from kaptive_amd.cli import main
    from kaptive_amd.serotyping.core import Serotyper
    from kaptive_amd.synth import make_db

    want = A.format_tsv(mini.ids, [g.contigs.ids for g in mini.genomes], mini.db.genes.ids, mini.bt.sums["n_kept"], mini.bt.kept, *mini.want())
    assert want.count(b"\n") > 20 and mini.bt.aligned_tsv() == want  # Engine(db, aligned=True): the native formatter on the device's rows
    typer = Serotyper(mini.db, aligned=True)
    try:
        results = typer.type_many(mini.genomes)
        from kaptive_amd.serotyping.io import KaptiveRow

        assert [bytes(KaptiveRow.from_result(r)) for r in results] == mini.bt.rows()  # the results do not depend on the option
        assert typer.engine.aligned and typer.engine.cigar and not typer.engine.variants
        b = typer.engine.ctx.batch(mini.packed)
        bt = typer.engine.type_batch(typer, b, mini.ids, mini.genomes)
        assert bt.aligned_tsv() == want and bt.rows() == mini.bt.rows()
        for a, i in ((0, 0), (2, 3)):
            assert bt.aligned_codes(a, i).tolist() == A.unpack_blocks(mini.blocks[int(mini.rows[a, i]["off"]) :], int(mini.rows[a, i]["gene_len"])).tolist()
        with pytest.raises(IndexError):
            bt.aligned_codes(1, 0)  # the assembly without a hit
        b.close()
    finally:
        typer.engine.close()
    db_path, paths = _write_inputs(mini.db, mini.genomes, tmp_path)
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "plain.tsv")]) == 0
    # two batches (of 3 genomes and 1): the genomes appear in input order
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--aligned", str(tmp_path / "rows.tsv"), "--batch-size", "3", "-g",
                 str(tmp_path / "genes")]) == 0  # fmt: skip
    table = (tmp_path / "rows.tsv").read_bytes()
    assert table == _native.ALIGNED_HEADER + want and _native.ALIGNED_HEADER == A.HEADER
    assert (tmp_path / "out.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()
    assert _check_table(table, tmp_path / "genes") > 10
    seen = [ln.split(b"\t")[0].decode() for ln in want.splitlines()]
    assert [n for i, n in enumerate(seen) if i == 0 or seen[i - 1] != n] == [n for n in mini.ids if n != "no_hit"]
    # with --variants, --breakpoints, --alleles and --paf in the same run: each file is what it is without --aligned
    others = ["--variants", str(tmp_path / "v.tsv"), "--breakpoints", str(tmp_path / "bp.tsv"), "--alleles", str(tmp_path / "al.tsv"), "--paf", str(tmp_path / "h.paf")]
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o1.tsv"), *others]) == 0
    alone = {f: (tmp_path / f).read_bytes() for f in ("v.tsv", "bp.tsv", "al.tsv", "h.paf", "o1.tsv")}
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o1.tsv"), *others, "--aligned", str(tmp_path / "rows2.tsv")]) == 0
    assert (tmp_path / "rows2.tsv").read_bytes() == table
    assert {f: (tmp_path / f).read_bytes() for f in alone} == alone and alone["o1.tsv"] == (tmp_path / "plain.tsv").read_bytes()
    # a second database: a table per database
    db_o = make_db("kpsc_o", seed=8)
    o_path = str(db_o.save(tmp_path / "o.npz"))
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "both.tsv"), "--aligned", str(tmp_path / "both.rows.tsv")]) == 0
    assert (tmp_path / "both.rows.kpsc_k.tsv").read_bytes() == table
    assert (tmp_path / "both.rows.kpsc_o.tsv").read_bytes().startswith(_native.ALIGNED_HEADER)
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "x.tsv"), "--aligned", "-"]) == 1  # stdout is refused
    assert not (tmp_path / "x.tsv").exists()


def test_command_line_on_two_devices(mini, tmp_path):
    import subprocess
    import sys

    if _native.device_count() < 2:
        pytest.skip("one device")
    db_path, paths = _write_inputs(mini.db, mini.genomes, tmp_path)
    from tests.conftest import ROOT

    r = subprocess.run([sys.executable, "-m", "kaptive_amd", "assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--aligned",
                        str(tmp_path / "rows.tsv"), "--devices", "0,1", "--batch-size", "2"], capture_output=True, timeout=600, cwd=str(ROOT))  # fmt: skip
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    assert (tmp_path / "rows.tsv").read_bytes() == _native.ALIGNED_HEADER + mini.bt.aligned_tsv()
