"""Variant records of the kept hits on the device (include/kp_spec.h, VARIANTS; kaptive_amd/csrc/kp_variants.hip).  Every record of
every kept hit of every assembly is compared, exactly, with the Python restatement of tests/variants_util.py run on the device's
own ops -- and, by a second route, with the records read off the same pass's cs strings -- on (1) the 9-locus miniature database
with 90 kb assemblies (one of them without a hit), (2) the join-limits batch of tests/join_limits_util.py (joined hits with merged
cross-gap ops), (3) the hand-built batch of tests/cs_util.py (both strands at every target offset, an N run, a gene that holds an
n, hits at contig ends).  Then the buffer's grow-and-rewrite, determinism and lifetime, the option off, a replaced hit table, the
library and the command line."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.pack import pack_sequences_flat
from tests import cigar_util as U
from tests import cs_util as S
from tests import join_limits_util as J
from tests import variants_util as V

pytestmark = pytest.mark.gpu

EINVAL = -1


class Typed:
    """One batch aligned and typed on an engine of its own: the typing records, the hit table with its ops and cs strings, and
    the variant records the options left."""

    def __init__(self, db, genomes, cs=True, variants=True, **options):
        from kaptive_amd.engine import Engine
        from kaptive_amd.serotyping.core import Serotyper

        self.db, self.genomes = db, genomes
        self.codes, self.off = pack_sequences_flat(db.genes)
        self.packed = [g.packed() for g in genomes]
        self.ids = [g.id for g in genomes]
        self.eng = Engine(db, cs=cs, variants=variants)
        for k, v in options.items():
            self.eng.ctx.set_option(k, v)
        self.typer = Serotyper(db)
        self.typer._engine = self.eng
        self.batch = self.eng.ctx.batch(self.packed)
        self.bt = self.eng.type_batch(self.typer, self.batch, self.ids, genomes)
        self.stats = self.batch.stats()
        self.hits, self.hoff = self.batch.hits()
        if cs or variants:
            self.ops, self.coff = self.batch.cigars()
        if cs:
            data, self.csoff = self.batch.cs()
            self.cs = data.tobytes()
        if variants:
            self.records, self.var_off = self.bt.variants()

    def yardstick(self, from_cs=False):
        """(records, var_off) of the restatement on the device's own ops (or cs strings), for every kept record in the lists' order."""
        out, off = [], [0]
        for a, pa in enumerate(self.packed):
            asm = U.assembly_codes(pa)
            n = 0
            for i in range(int(self.bt.sums["n_kept"][a])):
                r = V.kept_yardstick(self.bt.kept[a, i], self.hits[self.hoff[a] : self.hoff[a + 1]], self.ops, self.coff, int(self.hoff[a]), self.codes,
                                     self.off, pa, asm, cs=self.cs if from_cs else None, csoff=self.csoff if from_cs else None, index=i)  # fmt: skip
                out.append(r)
                n += len(r)
            off.append(off[-1] + n)
        return (np.concatenate(out) if out else np.zeros(0, _native.VARIANT_DTYPE)), np.array(off, np.int64)

    def tsv(self, records=None, var_off=None) -> bytes:
        """The Python formatter on the given (default: the device's) records."""
        records, var_off = (self.records, self.var_off) if records is None else (records, var_off)
        return V.format_tsv(self.ids, [g.contigs.ids for g in self.genomes], self.db.genes.ids, self.bt.kept, records, var_off)

    def close(self):
        self.batch.close()
        self.eng.close()


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


def _hand_db():
    """The hand-built genes of tests/cs_util.py as a database: one locus per gene, as tests/join_limits_util.py builds its own."""
    from kaptive_amd.db import Database
    from kaptive_amd.synth import random_dna

    seqs, genes = S.hand_genes()
    rng = np.random.default_rng(4244)
    loci = []
    for i, (name, g) in enumerate(zip(("big", "sub", "run", "with_n"), genes)):
        seq = np.concatenate([random_dna(rng, 100, 0.5), g, random_dna(rng, 100, 0.5)]).tobytes()
        loci.append(dict(name=f"HB{i + 1}", type=f"HT{i + 1}", extra=False, seq=seq,
                         genes=[dict(start=100, end=100 + len(g), strand=1, gene=f"hb_{name}", product=f"hand-built gene {name}")]))  # fmt: skip
    meta = dict(name="hand built", keyword="hand_built", genbank="hand_built.gbk", organism="Klebsiella pneumoniae species complex", taxon=573,
                antigen="K", pathway="Wzx/Wzy", version="synth-2024", id_threshold=82.5, doi=[], owner="kaptive_amd",
                repo="synthetic", branch="main", contact={}, phenotype_logic={})  # fmt: skip
    return Database.from_parts(meta, loci), genes


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
    db, genes = _hand_db()
    run = Typed(db, [S.hand_assembly(genes)])
    yield run
    run.close()


def _kept(bt) -> bytes:
    """The kept lists of a batch, every assembly's up to its n_kept (what lies behind them in a row is not defined)."""
    return b"".join(bt.kept[a, : int(n)].tobytes() for a, n in enumerate(bt.sums["n_kept"]))


def _same_records(got, want, label):
    assert len(got) == len(want), f"{label}: {len(got)} records on the device, the restatement has {len(want)}"
    if got.tobytes() != want.tobytes():
        i = next(i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes())
        raise AssertionError(f"{label}: record {i}: device {got[i]} vs the restatement's {want[i]}")


def _check_batch(run, label):
    want, want_off = run.yardstick()
    assert run.var_off.dtype == np.int64 and len(run.var_off) == len(run.genomes) + 1
    assert run.var_off.tolist() == want_off.tolist(), f"{label}: offsets"
    _same_records(run.records, want, label)
    by_cs, cs_off = run.yardstick(from_cs=True)
    assert cs_off.tolist() == want_off.tolist()
    _same_records(run.records, by_cs, f"{label}, from the cs strings of the same pass")
    assert not run.records["pad"].any()
    for a in range(len(run.genomes)):  # kept-list order, ascending in q_pos within a hit
        r = run.records[run.var_off[a] : run.var_off[a + 1]]
        assert (np.diff(r["kept"]) >= 0).all() and (r["kept"] < run.bt.sums["n_kept"][a]).all()
        assert ((np.diff(r["q_pos"]) >= 0) | (np.diff(r["kept"]) > 0)).all()
    return want


# ---- 1. records and offsets equal the restatement ----------------------------------------------------------------------------------------
def test_mini_batch(mini):
    _check_batch(mini, "mini")
    a = mini.ids.index("no_hit")
    assert mini.bt.sums["n_kept"][a] == 0 and mini.var_off[a] == mini.var_off[a + 1]  # an assembly without a hit: an empty range
    assert (np.diff(mini.var_off) > 0).sum() >= 2
    kept_strand = np.concatenate([mini.bt.kept["strand"][a, mini.records["kept"][mini.var_off[a] : mini.var_off[a + 1]]] for a in range(len(mini.ids))])
    assert {int(s) for s in kept_strand} == {-1, 1}, "records of both strands"
    assert {int(k) for k in mini.records["kind"]} == {V.SNV, V.INS, V.DEL}


def test_join_limits_batch(joins):
    _check_batch(joins, "join limits")
    r = joins.records
    assert (r["len"][r["kind"] != V.SNV] >= 33).sum() >= 10, "merged cross-gap ops of joined hits"


def test_hand_built_batch(hand):
    want = _check_batch(hand, "hand built")
    kept, n = hand.bt.kept[0], int(hand.bt.sums["n_kept"][0])
    assert n >= 4 and {int(s) for s in kept["strand"][:n]} == {-1, 1}
    for i in range(n):
        r = want[want["kept"] == i]
        g = int(kept["gene"][i])
        if g == S.SUB and kept["q_start"][i] == 0 and kept["q_end"][i] == 700:
            assert tuple(r["q_pos"].tolist()) == S.SUB_COLUMNS, f"kept {i}: substituted columns {r['q_pos'].tolist()}"
        if g == S.BIG:
            assert len(r) == 0
        if g == S.RUN:
            assert r["q_pos"].tolist() == [S.N_RUN_AT, S.N_RUN_AT + 1, S.N_RUN_AT + 2] and (r["alt"] == 4).all()
        if g == S.WITH_N:
            assert r["q_pos"].tolist() == [S.GENE_N_AT] and r["ref"].tolist() == [4] and r["ref_aa"].tolist() == [ord("X")]
    assert {S.BIG, S.SUB, S.RUN, S.WITH_N} <= {int(g) for g in kept["gene"][:n]}


# ---- 2. grow and re-emit -----------------------------------------------------------------------------------------------------------------
def test_a_small_first_guess_grows_the_buffer_without_another_pass(joins):
    total_kept = int(joins.bt.sums["n_kept"].sum())
    assert len(joins.records) > total_kept  # more than one record per kept hit: a buffer of one per kept hit is too small
    tight = Typed(joins.db, joins.genomes, variants_per_kept=1)
    plain = Typed(joins.db, joins.genomes, cs=False, variants=False)
    try:
        assert tight.hits.tobytes() == joins.hits.tobytes() and _kept(tight.bt) == _kept(joins.bt)
        assert tight.var_off.tobytes() == joins.var_off.tobytes() and tight.records.tobytes() == joins.records.tobytes()
        assert tight.stats["retries"] == joins.stats["retries"] == plain.stats["retries"], "growing the record buffer must not rerun a pass"
        assert plain.hits.tobytes() == joins.hits.tobytes() and _kept(plain.bt) == _kept(joins.bt)
    finally:
        tight.close()
        plain.close()


# ---- 3. determinism and lifetime --------------------------------------------------------------------------------------------------------
def test_determinism_and_lifetime(mini):
    again = mini.eng.ctx.batch(mini.packed)
    bt = mini.eng.type_batch(mini.typer, again, mini.ids, mini.genomes)
    records, var_off = bt.variants()
    assert _kept(bt) == _kept(mini.bt)
    assert var_off.tobytes() == mini.var_off.tobytes() and records.tobytes() == mini.records.tobytes()
    # the first batch's records, read after a second batch went through the same context: they live as long as its typing results
    records0, var_off0 = mini.batch.variants()
    assert var_off0.tobytes() == mini.var_off.tobytes() and records0.tobytes() == mini.records.tobytes()
    assert mini.batch.typing()[0].tobytes() == mini.bt.sums.tobytes()
    small = np.zeros(1, _native.VARIANT_DTYPE)  # a buffer that is too small is refused
    assert _native.lib().kp_batch_variants(mini.eng.ctx._h, mini.batch._h, small.ctypes.data_as(C.c_void_p), C.c_int64(1)) == EINVAL
    again.close()


# ---- 4. the option off ------------------------------------------------------------------------------------------------------------------
def _refused(ctx, batch):
    lib = _native.lib()
    off = np.zeros(batch.n_asm + 1, np.int64)
    for rc in (lib.kp_batch_variant_offsets(ctx._h, batch._h, off.ctypes.data_as(C.c_void_p)), lib.kp_batch_variants(ctx._h, batch._h, None, C.c_int64(0))):
        assert rc == EINVAL, rc
        assert b"variants option" in lib.kp_last_error(ctx._h)


def test_option_off_allocates_nothing_and_changes_nothing(mini):
    off = Typed(mini.db, mini.genomes, cs=False, variants=False)
    try:
        before = _native.device_allocations()
        second = off.eng.ctx.batch(off.packed)
        bt = off.eng.type_batch(off.typer, second, off.ids, off.genomes)
        assert _native.device_allocations() == before  # a settled context, a repeated batch: nothing grows
        _refused(off.eng.ctx, second)
        with pytest.raises(ValueError):
            second.variants()
        with pytest.raises(ValueError):
            bt.variants()
        assert _native.lib().kp_batch_cigars(off.eng.ctx._h, second._h, None, 0) == -4  # (variants = 0 asks for no CIGARs either)
        # the typing does not depend on the option: hits, records and the report rows, byte for byte
        assert off.hits.tobytes() == mini.hits.tobytes()
        assert bt.sums.tobytes() == mini.bt.sums.tobytes() and _kept(bt) == _kept(mini.bt)
        assert bt.tsv() == mini.bt.tsv() == off.bt.tsv() and len(bt.tsv().splitlines()) == len(mini.ids)
        second.close()
    finally:
        off.close()


# ---- 5. a replaced hit table ----------------------------------------------------------------------------------------------------------------
def test_replaced_hit_table_refuses_and_the_context_goes_on(mini):
    ctx = mini.eng.ctx
    b = ctx.batch(mini.packed)
    bt = mini.eng.type_batch(mini.typer, b, mini.ids, mini.genomes)
    assert bt.variants()[0].tobytes() == mini.records.tobytes()
    hits, hoff = b.hits()
    b.set_hits(hits, hoff)
    from kaptive_amd.serotyping import batch as B

    scores, counts = b.score(mini.typer.min_gene_coverage)
    best, _, _ = B.choose_best_loci(scores, counts, mini.typer._expected_genes_per_locus)
    b.reduce_async(best, mini.eng.typing_params(mini.typer))
    sums, kept, _ = b.typing()
    assert sums.tobytes() == mini.bt.sums.tobytes() and b"".join(kept[a, : int(n)].tobytes() for a, n in enumerate(sums["n_kept"])) == _kept(mini.bt)  # the same table reduces to the same records
    _refused(ctx, b)  # ... but nothing describes its paths any more
    b.close()
    fresh = ctx.batch(mini.packed)
    bt = mini.eng.type_batch(mini.typer, fresh, mini.ids, mini.genomes)
    assert bt.variants()[0].tobytes() == mini.records.tobytes() and bt.variants()[1].tobytes() == mini.var_off.tobytes()
    assert bt.tsv() == mini.bt.tsv()
    fresh.close()


# ---- 6. library and command line ----------------------------------------------------------------------------------------------------------
def _write_inputs(db, genomes, tmp_path, name="k.npz"):
    paths = []
    for g in genomes:
        p = tmp_path / f"{g.id}.fasta"
        p.write_bytes(g.contigs.to_fasta())
        paths.append(str(p))
    return str(db.save(tmp_path / name)), paths


def test_engine_serotyper_and_command_line(mini, tmp_path):
    from kaptive_amd.cli import main
    from kaptive_amd.serotyping.core import Serotyper
    from kaptive_amd.synth import make_db

    want_records, want_off = mini.yardstick()
    want = mini.tsv(want_records, want_off)
    assert want.count(b"\n") == len(want_records) > 0
    assert mini.bt.variants_tsv() == want  # Engine(db, variants=True): the native formatter on the device's records
    typer = Serotyper(mini.db, variants=True)
    try:
        results = typer.type_many(mini.genomes)
        from kaptive_amd.serotyping.io import KaptiveRow

        assert [bytes(KaptiveRow.from_result(r)) for r in results] == mini.bt.rows()  # the results do not depend on the option
        assert typer.engine.variants and typer.engine.cigar
        b = typer.engine.ctx.batch(mini.packed)
        bt = typer.engine.type_batch(typer, b, mini.ids, mini.genomes)
        assert bt.variants_tsv() == want and bt.rows() == mini.bt.rows()
        b.close()
    finally:
        typer.engine.close()
    db_path, paths = _write_inputs(mini.db, mini.genomes, tmp_path)
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "plain.tsv")]) == 0
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--variants", str(tmp_path / "v.tsv"), "--batch-size", "3"]) == 0
    assert (tmp_path / "v.tsv").read_bytes() == V.HEADER + want
    assert (tmp_path / "out.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()
    # a second database: a table per database, each equal to that database's engine alone (its genes lie behind the first one's)
    db_o = make_db("kpsc_o", seed=8)
    o_path = str(db_o.save(tmp_path / "o.npz"))
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "both.tsv"), "--variants", str(tmp_path / "both.var.tsv")]) == 0
    assert (tmp_path / "both.var.kpsc_k.tsv").read_bytes() == V.HEADER + want
    alone = Typed(db_o, mini.genomes, cs=False)
    try:
        o_records, o_off = alone.yardstick()
        _same_records(alone.records, o_records, "the second database alone")
        assert (tmp_path / "both.var.kpsc_o.tsv").read_bytes() == V.HEADER + alone.tsv(o_records, o_off)
    finally:
        alone.close()


def test_command_line_on_two_devices(mini, tmp_path):
    import subprocess
    import sys

    if _native.device_count() < 2:
        pytest.skip("one device")
    db_path, paths = _write_inputs(mini.db, mini.genomes, tmp_path)
    from tests.conftest import ROOT

    r = subprocess.run([sys.executable, "-m", "kaptive_amd", "assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--variants",
                        str(tmp_path / "v.tsv"), "--devices", "0,1", "--batch-size", "2"], capture_output=True, timeout=600, cwd=str(ROOT))  # fmt: skip
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    assert (tmp_path / "v.tsv").read_bytes() == V.HEADER + mini.tsv()
