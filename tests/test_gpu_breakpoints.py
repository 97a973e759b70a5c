"""Breakpoint records of the kept lists on the device (include/kp_spec.h, BREAKPOINTS; kaptive_amd/csrc/kp_breakpoints.hip).  Every
record of every assembly is compared, exactly, with the Python restatement of tests/breakpoints_util.py run on the device's own kept
lists and contigs: (1) the eight planted events of the miniature database and an assembly without a hit, aligned and typed by the
device; (2) hand-made hit tables -- kept lists of 0 to 2048 records that sit on every limit of the pair rule -- put in place with
kp_batch_set_hits and reduced; (3) a hand-built element with terminal inverted repeats at every offset of a packed word; then
lifetime and determinism, two databases in one pass, the library and the command line."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from tests import breakpoints_util as P
from tests import cigar_util as U

pytestmark = pytest.mark.gpu

EINVAL = -1
SIZES = (0, 1, 63, 64, 65, 300, 2048)


def _yardstick(kept, sums, packed):
    """(records, bp_off) of the restatement on a batch's kept lists, assembly by assembly."""
    out, off = [], [0]
    for a, pa in enumerate(packed):
        r = P.restate(kept[a, : int(sums["n_kept"][a])], pa.ctg_start, pa.ctg_len, U.assembly_codes(pa))
        out.append(r)
        off.append(off[-1] + len(r))
    return np.concatenate(out) if out else np.zeros(0, _native.BREAKPOINT_DTYPE), np.array(off, np.int64)


def _bases(genome) -> int:
    return int(genome.contigs.lengths.sum())


def _same_records(got, want, label):
    assert got.dtype == want.dtype and len(got) == len(want), f"{label}: {len(got)} records on the device, the restatement has {len(want)}"
    if got.tobytes() != want.tobytes():
        i = next(i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes())
        raise AssertionError(f"{label}: record {i}: device {got[i]} vs the restatement's {want[i]}")


def _check(batch, packed, label, group=0):
    """The device's records of the batch's current reduction against the restatement on its own kept lists."""
    sums, kept, _ = batch.typing(group)
    records, bp_off = batch.breakpoints(group)
    want, want_off = _yardstick(kept, sums, packed)
    assert bp_off.dtype == np.int64 and bp_off.tolist() == want_off.tolist(), f"{label}: offsets {bp_off.tolist()} vs {want_off.tolist()}"
    _same_records(records, want, label)
    assert not records["pad"].any()
    for a in range(len(packed)):
        assert (np.diff(records["kept_b"][bp_off[a] : bp_off[a + 1]]) > 0).all()
    return sums, kept, records, bp_off


@pytest.fixture(scope="module")
def db():
    return P.plant_db()


class Planted:
    """The eight planted assemblies and one without a hit, aligned and typed on an engine of their own."""

    def __init__(self, db, breakpoints=True):
        from kaptive_amd.core.genome import GenomeAssembly
        from kaptive_amd.core.seq import SeqRecord, Sequences
        from kaptive_amd.engine import Engine
        from kaptive_amd.serotyping.core import Serotyper
        from kaptive_amd.synth import random_dna

        self.db, self.cases = db, P.plants(db)
        empty = GenomeAssembly("no_hit", Sequences.from_records([SeqRecord("r0", random_dna(np.random.default_rng(99), 30_000, 0.5).tobytes())]))
        self.genomes = [c[1] for c in self.cases[:4]] + [empty] + [c[1] for c in self.cases[4:]]
        self.ids = [g.id for g in self.genomes]
        self.packed = [g.packed() for g in self.genomes]
        self.eng = Engine(db, breakpoints=breakpoints)
        self.typer = Serotyper(db)
        self.typer._engine = self.eng
        self.batch = self.eng.ctx.batch(self.packed)
        self.bt = self.eng.type_batch(self.typer, self.batch, self.ids, self.genomes)

    def tsv(self, records, bp_off) -> bytes:
        return P.format_tsv(self.ids, [g.contigs.ids for g in self.genomes], self.db.genes.ids, self.bt.kept, records, bp_off,
                            self.typer.partial_edge_tolerance)  # fmt: skip

    def close(self):
        self.batch.close()
        self.eng.close()


@pytest.fixture(scope="module")
def planted(db):
    run = Planted(db)
    yield run
    run.close()


# ---- 1. planted events ---------------------------------------------------------------------------------------------------------------------
def test_planted_events(planted):
    assert max(_bases(g) for g in planted.genomes) <= 90_000
    records, bp_off = planted.bt.breakpoints()
    sums, kept, got, got_off = _check(planted.batch, planted.packed, "planted")
    assert got.tobytes() == records.tobytes() and got_off.tobytes() == bp_off.tobytes() and kept.tobytes() == planted.bt.kept.tobytes()
    a = planted.ids.index("no_hit")
    assert sums["n_kept"][a] == 0 and bp_off[a] == bp_off[a + 1]
    for name, genome, gene_index, expect in planted.cases:
        a = planted.ids.index(name)
        P.check_plant(name, gene_index, expect, kept[a], records[bp_off[a] : bp_off[a + 1]], planted.typer.partial_edge_tolerance)
    want = planted.tsv(records, bp_off)
    assert planted.bt.breakpoints_tsv() == want and want.count(b"\n") == 8
    assert {ln.split(b"\t")[2] for ln in want.splitlines()} == {b"insertion", b"deletion", b"contig_break", b"inversion"}


# ---- 2. the selection rule on hand-made hit tables ----------------------------------------------------------------------------------------------
class HandMade:
    """Assemblies whose hit tables are the fragment tables of tests/breakpoints_util.py, put in place with kp_batch_set_hits."""

    def __init__(self, db, genomes, tables):
        from kaptive_amd.engine import Engine
        from kaptive_amd.serotyping.core import Serotyper

        self.db, self.genomes, self.tables = db, genomes, tables
        self.packed = [g.packed() for g in self.genomes]
        self.eng = Engine(db)
        self.typer = Serotyper(db)
        self.typer._engine = self.eng
        self.batch = self.eng.ctx.batch(self.packed)
        self.batch.align_async()
        self.batch.wait()
        off = np.concatenate([[0], np.cumsum([len(t) for t in self.tables])]).astype(np.int64)
        self.batch.set_hits(np.concatenate(self.tables) if self.tables else np.zeros(0, _native.HIT_DTYPE), off)

    def reduce(self, id_threshold: float):
        from kaptive_amd.serotyping import batch as B

        scores, counts = self.batch.score(self.typer.min_gene_coverage)
        best, _, _ = B.choose_best_loci(scores, counts, self.typer._expected_genes_per_locus)
        prm = self.eng.typing_params(self.typer)
        prm.id_threshold = id_threshold
        self.batch.reduce_async(best, prm)

    def close(self):
        self.batch.close()
        self.eng.close()


def _layouts(db):
    out = []
    for n in SIZES:
        rng = np.random.default_rng(626200 + n)
        small = n > 300  # 2048 fragments on 90 kb: 30 bases each, few pairs whose targets overlap
        frag = 30 if small else (200 if n == 300 else 250)
        out.append(P.Layout(rng, db.genes.lengths, frag=frag, contig_len=3000, long_pairs=4 if small else 6, far_gaps=not small).fill(n))
    return out


@pytest.fixture(scope="module")
def hand_made(db):
    layouts = _layouts(db)
    run = HandMade(db, [lay.genome(f"table{n}") for lay, n in zip(layouts, SIZES)], [lay.hits() for lay in layouts])
    yield run
    run.close()


def test_selection_rule_on_hand_made_hit_tables(hand_made):
    run = hand_made
    assert max(_bases(g) for g in run.genomes) <= 90_000, [_bases(g) for g in run.genomes]
    run.reduce(0.0)  # no identity threshold: no record is spurious
    sums, kept, records, bp_off = _check(run.batch, run.packed, "hand-made tables")
    assert sums["n_kept"].tolist() == list(SIZES), "the overlap cull keeps every fragment of these tables"
    assert not (kept["flags"] & P.F_SPURIOUS).any()
    assert {int(k) for k in records["kind"]} == {P.COLLINEAR, P.INVERTED, P.DISORDERED, P.CONTIGS}
    assert (np.diff(bp_off) > 0).sum() >= 5 and bp_off[1] == 0 and bp_off[2] == 0  # 0 and 1 records: no pair
    classes: dict = {}
    for lay in _layouts(run.db):
        for k, v in lay.classes.items():
            classes[k] = classes.get(k, 0) + v
    for name in ("t_gap -64", "t_gap -65", "q overlap 64", "q overlap 65", "equal keys", "full copies", "three ranks", "rank 1 wins", "rank 2 wins"):
        assert classes.get(name, 0) > 0, f"no table holds the class {name!r}: {classes}"
    first = records.tobytes()
    # ... and with a threshold that makes a fifth of the records outside the locus spurious: the records are gone and made again
    outside = np.concatenate([kept["pident"][a, :n][(kept["flags"][a, :n] & 2) == 0] for a, n in enumerate(sums["n_kept"])])
    assert len(outside) > 500
    run.reduce(float(np.quantile(outside, 0.2)))
    sums2, kept2, records2, bp_off2 = _check(run.batch, run.packed, "hand-made tables with spurious records")
    dead = sum(int((kept2["flags"][a, :n] & P.F_SPURIOUS).astype(bool).sum()) for a, n in enumerate(sums2["n_kept"]))
    assert 100 < dead < 0.5 * sums2["n_kept"].sum() and records2.tobytes() != first and len(records2) < len(records)


# ---- 3. the inverted repeat --------------------------------------------------------------------------------------------------------------------
def test_inverted_repeat_at_every_word_offset(db):
    genome, hits, cases = P.inverted_repeat_assembly(db)
    assert _bases(genome) <= 90_000
    run = HandMade(db, [genome], [hits])
    try:
        run.reduce(0.0)
        sums, kept, records, bp_off = _check(run.batch, run.packed, "inverted repeat")
        assert len(records) == len(cases) == sums["n_kept"][0] // 2
        pa = run.packed[0]
        by_gene = {int(kept[0, int(r["kept_b"])]["gene"]): r for r in records}
        offsets = {1: set(), -1: set()}
        clean = {}
        for g, (label, strand, n) in cases.items():
            r = by_gene[g]
            assert r["kind"] == P.COLLINEAR and r["t_gap"] == n and r["q_gap"] == 0 and kept[0, int(r["kept_b"])]["strand"] == strand, (label, r)
            assert r["ir_cols"] == (min(32, n // 2) if n >= 2 else 0) and r["ir_matches"] <= r["ir_cols"], (label, r)
            if label == "tir":
                assert r["ir_matches"] >= P.TIR, (label, r)
                at = int(pa.ctg_start[kept[0, int(r["kept_b"])]["contig"]]) + int(r["t_lo"])
                offsets[strand].add(at % 16)
                clean.setdefault(strand, int(r["ir_matches"]))
                assert int(r["ir_matches"]) == clean[strand], "the same element at every offset"
        assert offsets[1] == offsets[-1] == set(range(16)), offsets
        for g, (label, strand, n) in cases.items():
            if label == "tir with N":
                assert int(by_gene[g]["ir_matches"]) == clean[strand] - 1, "an N in one repeat column takes that column away"
    finally:
        run.close()


# ---- 4. lifetime and determinism -----------------------------------------------------------------------------------------------------------
def _refused(ctx, batch):
    lib = _native.lib()
    off = np.zeros(batch.n_asm + 1, np.int64)
    for rc in (lib.kp_batch_breakpoint_offsets(ctx._h, batch._h, off.ctypes.data_as(C.c_void_p)), lib.kp_batch_breakpoints(ctx._h, batch._h, None, C.c_int64(0))):
        assert rc == EINVAL, rc
        assert b"kp_batch_reduce has not run" in lib.kp_last_error(ctx._h)


def test_lifetime_and_determinism(planted):
    ctx = planted.eng.ctx
    first = planted.bt.breakpoints()
    again = planted.batch.breakpoints()  # a second call: the same bytes
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    b = ctx.batch(planted.packed)
    _refused(ctx, b)  # never aligned
    b.align_async()
    b.wait()
    _refused(ctx, b)  # aligned, not reduced
    with pytest.raises(ValueError):
        b.breakpoints()
    bt = planted.eng.type_batch(planted.typer, b, planted.ids, planted.genomes, aligned=True)  # ... and the context types it as usual
    assert bt.breakpoints()[0].tobytes() == first[0].tobytes() and bt.breakpoints()[1].tobytes() == first[1].tobytes()
    assert bt.tsv() == planted.bt.tsv()
    small = np.zeros(1, _native.BREAKPOINT_DTYPE)  # a buffer that is too small is refused
    assert _native.lib().kp_batch_breakpoints(ctx._h, b._h, small.ctypes.data_as(C.c_void_p), C.c_int64(1)) == EINVAL
    # the next reduction of the group replaces the kept list: its records are gone and made again (an identity threshold above 100
    # makes every record outside the locus spurious)
    from kaptive_amd.serotyping import batch as B

    scores, counts = b.score(planted.typer.min_gene_coverage)
    best, _, _ = B.choose_best_loci(scores, counts, planted.typer._expected_genes_per_locus)
    prm = planted.eng.typing_params(planted.typer)
    prm.id_threshold = 101.0
    b.reduce_async(best, prm)
    _check(b, planted.packed, "after a second reduction")
    # a replaced hit table: refused until it is reduced, then served -- the records need no ops
    hits, hoff = b.hits()
    b.set_hits(hits, hoff)
    _refused(ctx, b)
    scores, counts = b.score(planted.typer.min_gene_coverage)
    b.reduce_async(best, planted.eng.typing_params(planted.typer))
    sums, kept, records, bp_off = _check(b, planted.packed, "after kp_batch_set_hits and a reduction")
    assert records.tobytes() == first[0].tobytes() and bp_off.tobytes() == first[1].tobytes()
    b.close()
    # the first batch's records, after all that went through the same context
    again = planted.batch.breakpoints()
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()


def test_option_off_changes_nothing_and_the_device_call_needs_no_option(planted):
    off = Planted(planted.db, breakpoints=False)
    try:
        second = off.eng.ctx.batch(off.packed)
        off.eng.type_batch(off.typer, second, off.ids, off.genomes)
        before = _native.device_allocations()
        bt = off.eng.type_batch(off.typer, second, off.ids, off.genomes)
        assert _native.device_allocations() == before  # a settled work set, a repeated pass: no buffer grows
        with pytest.raises(ValueError, match="breakpoints=True"):
            bt.breakpoints()
        with pytest.raises(ValueError, match="breakpoints=True"):
            bt.breakpoints_tsv()
        assert bt.tsv() == planted.bt.tsv() and bt.kept.tobytes() == planted.bt.kept.tobytes()
        records, bp_off = second.breakpoints()  # the device call itself needs no option
        assert records.tobytes() == planted.bt.breakpoints()[0].tobytes() and bp_off.tobytes() == planted.bt.breakpoints()[1].tobytes()
        off.eng.type_batch(off.typer, second, off.ids, off.genomes)
        assert second.breakpoints()[0].tobytes() == records.tobytes() and _native.device_allocations() == before  # ... nor do the records' buffers, asked for again
        second.close()
    finally:
        off.close()


def test_two_databases_in_one_pass(planted):
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.serotyping.core import MultiSerotyper
    from kaptive_amd.synth import make_db, random_dna

    db_o = make_db("kpsc_o", seed=8)
    rng = np.random.default_rng(77)
    g0 = int(db_o.locus_gene_offsets[0])
    gi = next(g for g in range(g0, g0 + int(db_o.locus_gene_lengths[0])) if db_o.gene_intervals.strands[g] > 0 and db_o.genes.lengths[g] >= 900)
    o_contig = np.concatenate([random_dna(rng, 3000, 0.5), P.locus_with_insertion(db_o, 0, gi, 450, 1000, 4, rng), random_dna(rng, 3000, 0.5)])
    genomes = []
    short = {c[0]: c[1] for c in P.plants(planted.db, flank_len=12_000)}  # (room for the O locus within 90 kb)
    for g in (short["ins1500"], planted.genomes[4], short["contig_cut_dup9_rc"]):  # an insertion, no hit, a contig cut: each with the O locus
        recs = [SeqRecord(str(n), bytes(g.contigs.seqs[o : o + m])) for n, o, m in zip(g.contigs.ids, g.contigs.offsets, g.contigs.lengths)]
        genomes.append(GenomeAssembly(g.id, Sequences.from_records(recs + [SeqRecord("o_locus", o_contig.tobytes())])))
    assert max(_bases(g) for g in genomes) <= 90_000
    ms = MultiSerotyper([planted.db, db_o], breakpoints=True)
    try:
        packed = [g.packed() for g in genomes]
        batch = ms.engine.ctx.batch(packed)
        (groups, _), = list(ms.engine.type_stream_groups(ms.serotypers, [(batch, [g.id for g in genomes], genomes)]))
        assert len(groups) == 2
        for k, (bt, n_want) in enumerate(zip(groups, ([1, 0, 1], [1, 1, 1]))):
            records, bp_off = bt.breakpoints()
            want, want_off = _yardstick(bt.kept, bt.sums, packed)
            assert bp_off.tolist() == want_off.tolist() and np.diff(bp_off).tolist() == n_want, (k, bp_off)
            _same_records(records, want, f"database {k}")
            assert bt.breakpoints_tsv() == P.format_tsv(bt.ids, [g.contigs.ids for g in genomes], ms.dbs[k].genes.ids, bt.kept, records, bp_off, 5)
        r = groups[1].breakpoints()[0]
        assert (r["kind"] == P.COLLINEAR).all() and (r["t_gap"] - r["q_gap"] == 1004).all()
        assert int(groups[1].kept[0, int(r[0]["kept_b"])]["gene"]) == gi  # gene indices of a group are its own database's
        batch.close()
    finally:
        ms.close()


# ---- 5. library and command line -------------------------------------------------------------------------------------------------------------
def _write_inputs(db, genomes, tmp_path, name="k.npz"):
    paths = []
    for g in genomes:
        p = tmp_path / f"{g.id}.fasta"
        p.write_bytes(g.contigs.to_fasta())
        paths.append(str(p))
    return str(db.save(tmp_path / name)), paths


def test_serotyper_and_command_line(planted, tmp_path):
    from kaptive_amd.cli import main
    from kaptive_amd.serotyping.core import Serotyper
    from kaptive_amd.synth import make_db

    records, bp_off = planted.bt.breakpoints()
    want = planted.tsv(records, bp_off)
    typer = Serotyper(planted.db, breakpoints=True)
    try:
        assert typer.engine.breakpoints and not typer.engine.cigar  # the alignment passes do nothing more for them
        b = typer.engine.ctx.batch(planted.packed)
        bt = typer.engine.type_batch(typer, b, planted.ids, planted.genomes)
        assert bt.breakpoints_tsv() == want and bt.rows() == planted.bt.rows()
        b.close()
    finally:
        typer.engine.close()
    db_path, paths = _write_inputs(planted.db, planted.genomes, tmp_path)
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "plain.tsv")]) == 0
    # two batches (of 5 and 4 genomes): the genomes appear in input order
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--breakpoints", str(tmp_path / "bp.tsv"), "--batch-size", "5"]) == 0
    assert (tmp_path / "bp.tsv").read_bytes() == P.HEADER + want
    assert [ln.split(b"\t")[0].decode() for ln in want.splitlines()] == [c[0] for c in planted.cases]
    assert (tmp_path / "out.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()
    # with --variants and --paf in the same run: each file is what it is alone
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "all.tsv"), "--breakpoints", str(tmp_path / "bp2.tsv"), "--variants",
                 str(tmp_path / "v.tsv"), "--paf", str(tmp_path / "h.paf")]) == 0  # fmt: skip
    assert (tmp_path / "bp2.tsv").read_bytes() == P.HEADER + want and (tmp_path / "all.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()
    assert (tmp_path / "v.tsv").read_bytes().startswith(_native.VARIANTS_HEADER) and (tmp_path / "h.paf").stat().st_size > 0
    # a second database: a table per database
    db_o = make_db("kpsc_o", seed=8)
    o_path = str(db_o.save(tmp_path / "o.npz"))
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "both.tsv"), "--breakpoints", str(tmp_path / "both.bp.tsv")]) == 0
    assert (tmp_path / "both.bp.kpsc_k.tsv").read_bytes() == P.HEADER + want
    assert (tmp_path / "both.bp.kpsc_o.tsv").read_bytes() == P.HEADER  # no O locus in these assemblies: the header alone
