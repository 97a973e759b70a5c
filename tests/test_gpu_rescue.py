"""Rescue records of the missing genes on the device (include/kp_spec.h, RESCUE; kaptive_amd/csrc/kp_rescue.hip).  Every record of every
assembly is compared, exactly, with the yardstick of tests/rescue_util.py -- the reference-pinned extraction, translation and protein
alignment -- run on the device's own summaries and pieces: (1) one locus cut into contigs of two genes with one gene recoded so that no
nucleotide seed finds it -- found, with a stop, cut by a contig end, reverse-complemented, deleted, relocated, twice, behind 0 .. 15
more bases, with an N run, with a protein that needs strips, with the default flank unclipped -- and an assembly without a hit;
(2) hand-made hit tables over a database whose proteins sit on both sides of every limit of the fill kernel, with windows down to one
base and rescue_flank 0; then lifetime, the option off, two databases in one pass, the library and the command line.  (The
preconditions of (1) are checked without a device in tests/test_rescue_cpu.py.)"""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from tests import rescue_util as R

pytestmark = pytest.mark.gpu

EINVAL = -1


def _same(got, want, label, ids=None):
    (g, g_off), (w, w_off) = got, want
    assert g.dtype == _native.RESCUE_DTYPE == R.RESCUE_DTYPE, label
    assert g_off.tolist() == w_off.tolist(), f"{label}: offsets {g_off.tolist()} vs {w_off.tolist()}"
    if g.tobytes() != w.tobytes():
        i = next(i for i in range(len(g)) if g[i] != w[i])
        a = int(np.searchsorted(w_off, i, side="right")) - 1
        raise AssertionError(f"{label}: assembly {a} ({ids[a] if ids else '?'}) record {i}: device {g[i]} vs the yardstick's {w[i]}")


def _check(batch, packed, db, flank, tol, label, ids=None, group=0):
    sums, kept, pieces = batch.typing(group)
    got = batch.rescue(group)
    _same(got, R.restate_batch(sums, pieces, packed, db, flank, tol), label, ids)
    return sums, pieces, got


@pytest.fixture(scope="module")
def db():
    return R.plant_db()


class Planted:
    def __init__(self, db, rescue=True, names=None):
        from kaptive_amd.engine import Engine
        from kaptive_amd.serotyping.core import Serotyper

        self.db = db
        cases = R.plants(db)
        self.cases = {n: cases[n] for n in (names or cases)}
        self.genomes = [g for g, _, _ in self.cases.values()]
        self.ids = [g.id for g in self.genomes]
        self.packed = [g.packed() for g in self.genomes]
        self.eng = Engine(db, rescue=rescue)
        self.typer = Serotyper(db, rescue=rescue)
        self.typer._engine = self.eng
        self.batch = self.eng.ctx.batch(self.packed)
        self.bt = self.eng.type_batch(self.typer, self.batch, self.ids, self.genomes)

    def tsv(self, bt=None, min_score=R.MIN_SCORE) -> bytes:
        bt = self.bt if bt is None else bt
        records, off = bt.rescue()
        return R.tsv(records, off, bt.ids, [g.contigs.ids for g in self.genomes], self.db.genes.ids, self.db.loci.ids, bt.best_locus,
                     self.db.translations.lengths, min_score)  # fmt: skip

    def close(self):
        self.batch.close()
        self.eng.close()


@pytest.fixture(scope="module")
def planted(db):
    run = Planted(db)
    yield run
    run.close()


# ---- 1. the planted locus ------------------------------------------------------------------------------------------------------------------
def test_planted_genes_against_the_yardstick(planted):
    bt, db = planted.bt, planted.db
    tol = planted.typer.partial_edge_tolerance
    sums, pieces, (records, off) = _check(planted.batch, planted.packed, db, R.FLANK, tol, "planted", planted.ids)
    assert bt.rescue()[0].tobytes() == records.tobytes() and bt.rescue()[1].tolist() == off.tolist()
    prot_len = np.asarray(db.translations.lengths)
    g0 = int(db.locus_gene_offsets[R.PLANT_LOCUS])
    word_offsets = set()
    for a, (name, (genome, gene, expect)) in enumerate(planted.cases.items()):
        recs = records[off[a] : off[a + 1]]
        if name == "no_hit":
            # every expected gene of whichever locus scored best is a zero record: there is no window
            assert int(sums["n_pieces"][a]) == 0 and len(recs) == len(R.subjects(sums[a])) > 0, name
            assert (recs["piece"] == -1).all() and not any(recs[n].any() for n in recs.dtype.names if n not in ("gene", "piece")), name
            continue
        assert int(sums["best_locus"][a]) == R.PLANT_LOCUS and [g0 + j for j in R.subjects(sums[a])] == [gene], name
        r = recs[0]
        assert (int(r["score"]) >= R.MIN_SCORE) == expect["found"], (name, r)
        if "call" in expect:
            assert R.call(r, int(prot_len[gene]), R.MIN_SCORE) == expect["call"], (name, r)
        if "piece_contig" in expect:
            assert int(r["contig"]) == expect["piece_contig"] and int(sums["n_pieces"][a]) >= 3, name
        if expect.get("unclipped"):
            pc = pieces[a, int(r["piece"])]
            assert int(pc["start"]) >= R.FLANK and int(pc["end"]) + R.FLANK <= int(planted.packed[a].ctg_len[int(pc["contig"])]), name
        if name.startswith("shift"):
            pc = pieces[a, int(r["piece"])]
            ws, _ = R.window(int(pc["start"]), int(pc["end"]), int(planted.packed[a].ctg_len[int(pc["contig"])]), R.FLANK)
            word_offsets.add((int(planted.packed[a].ctg_start[int(pc["contig"])]) + ws + int(r["t_start"])) % 16)
    assert len(word_offsets) == 16, "the recoded gene starts at every offset of a packed word"
    a = planted.ids.index("reversed")
    assert int(records["strand"][off[a]]) == -1 and int(records["strand"][off[planted.ids.index("diverged")]]) == 1
    a = planted.ids.index("long")
    assert int(prot_len[int(records["gene"][off[a]])]) > R.STRIP_LIMITS[-1], "a protein cut into strips"
    want = planted.tsv()
    assert bt.rescue_tsv() == want and want.count(b"\n") == len(records)
    assert bt.rescue_tsv(min_score=10_000) == planted.tsv(min_score=10_000) and b"\tdiverged\t" not in bt.rescue_tsv(min_score=10_000)


# ---- 2. shapes through hand-made hit tables ---------------------------------------------------------------------------------------------------
class Shapes:
    def __init__(self):
        from kaptive_amd.engine import Engine
        from kaptive_amd.serotyping.core import Serotyper

        self.db = R.shape_db()
        self.genomes, self.tables = R.shape_assemblies(self.db)
        self.packed = [g.packed() for g in self.genomes]
        self.eng = Engine(self.db, rescue=True, rescue_flank=R.SHAPE_FLANK)
        self.typer = Serotyper(self.db)
        self.typer._engine = self.eng
        self.batch = self.eng.ctx.batch(self.packed)
        self.batch.align_async()
        self.batch.wait()
        off = np.concatenate([[0], np.cumsum([len(t) for t in self.tables])]).astype(np.int64)
        self.batch.set_hits(np.concatenate(self.tables), off)

    def reduce(self):
        from kaptive_amd.serotyping import batch as B

        scores, counts = self.batch.score(self.typer.min_gene_coverage)
        self.best, _, _ = B.choose_best_loci(scores, counts, self.typer._expected_genes_per_locus)
        self.batch.reduce_async(self.best, self.eng.typing_params(self.typer))

    def close(self):
        self.batch.close()
        self.eng.close()


@pytest.fixture(scope="module")
def shapes():
    run = Shapes()
    yield run
    run.close()


def test_proteins_on_both_sides_of_every_limit(shapes):
    run, tol = shapes, shapes.typer.partial_edge_tolerance
    run.reduce()
    sums, pieces, (records, off) = _check(run.batch, run.packed, run.db, R.SHAPE_FLANK, tol, "shapes", [g.id for g in run.genomes])
    prot_len = np.asarray(run.db.translations.lengths)
    recs = records[off[0] : off[1]]
    assert int(sums["n_pieces"][0]) == 2 and sorted(int(prot_len[g]) for g in recs["gene"]) == sorted(R.SHAPE_PROTEINS)
    for limit in R.STRIP_LIMITS:
        assert {limit - 1, limit, limit + 1} <= set(R.SHAPE_PROTEINS)
    by_len = {int(prot_len[r["gene"]]): r for r in recs}
    assert int(by_len[129]["score"]) > 300 and int(by_len[385]["score"]) > 1000 and (recs["score"] > 0).all()
    big = by_len[1100]  # three strips; its longer fragment ends on the contig's (and the batch's assembly's) last base
    assert int(big["score"]) > 1000 and int(big["contig"]) == 1 and int(big["t_end"]) == int(run.packed[0].ctg_len[1]) and int(big["edge"]) & 2
    assert int(big["p_end"]) - int(big["p_start"]) > R.STRIP_LIMITS[-1], "the path crosses a strip boundary"
    # rescue_flank 0: the window is the piece itself -- one to five bases, frame texts of no residue or one
    run.eng.ctx.set_option("rescue_flank", 0)
    sums, pieces, (records, off) = _check(run.batch, run.packed, run.db, 0, tol, "flank 0", [g.id for g in run.genomes])
    spans = [int(pieces["end"][a, 0]) - int(pieces["start"][a, 0]) for a in range(1, len(run.genomes))]
    assert spans == [1, 2, 3, 4, 5]
    assert not records["score"][off[1] : off[3]].any() and set(records["a_len"][off[3] :].tolist()) <= {0, 1} and records["score"][off[3] :].any()
    run.eng.ctx.set_option("rescue_flank", R.SHAPE_FLANK)
    _check(run.batch, run.packed, run.db, R.SHAPE_FLANK, tol, "the flank set back")
    with pytest.raises(ValueError, match="rescue_flank"):
        run.eng.ctx.set_option("rescue_flank", R.FLANK_MAX + 1)


# ---- 3. lifetime and surface --------------------------------------------------------------------------------------------------------------------
def _refused(ctx, batch):
    lib = _native.lib()
    off = np.zeros(batch.n_asm + 1, np.int64)
    assert lib.kp_batch_rescue_offsets(ctx._h, batch._h, off.ctypes.data_as(C.c_void_p)) == EINVAL
    assert b"no rescue records" in lib.kp_last_error(ctx._h)
    assert lib.kp_batch_rescue(ctx._h, batch._h, None, C.c_int64(0)) == EINVAL and b"no rescue records" in lib.kp_last_error(ctx._h)
    with pytest.raises(ValueError):
        batch.rescue()


def _eq(x, y):
    return x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()


PICK = ("diverged", "stop", "cut", "reversed", "deleted", "long", "no_hit")  # (in the planted batch's order)


def test_lifetime_and_determinism(planted):
    from kaptive_amd.serotyping import batch as B

    ctx = planted.eng.ctx
    first = planted.bt.rescue()
    assert _eq(planted.batch.rescue(), first)  # a second call: the same bytes
    pick = [planted.ids.index(n) for n in PICK]
    packed, ids, genomes = [planted.packed[i] for i in pick], [planted.ids[i] for i in pick], [planted.genomes[i] for i in pick]
    b = ctx.batch(packed)
    _refused(ctx, b)  # never aligned
    b.align_async()
    b.wait()
    _refused(ctx, b)  # aligned, not reduced
    bt = planted.eng.type_batch(planted.typer, b, ids, genomes, aligned=True)
    got = bt.rescue()
    for k, i in enumerate(pick):
        assert got[0][got[1][k] : got[1][k + 1]].tobytes() == first[0][first[1][i] : first[1][i + 1]].tobytes(), ids[k]
    lib = _native.lib()
    out = np.zeros(len(got[0]), _native.RESCUE_DTYPE)
    assert lib.kp_batch_rescue(ctx._h, b._h, out.ctypes.data_as(C.c_void_p), C.c_int64(len(out) - 1)) == EINVAL and b"too small" in lib.kp_last_error(ctx._h)
    # a second reduction replaces the records: with another edge tolerance the edge bits are made again
    scores, counts = b.score(planted.typer.min_gene_coverage)
    best, _, _ = B.choose_best_loci(scores, counts, planted.typer._expected_genes_per_locus)
    prm = planted.eng.typing_params(planted.typer)
    prm.edge_tolerance = 400
    b.reduce_async(best, prm)
    _, _, again = _check(b, packed, planted.db, R.FLANK, 400, "after a second reduction", ids)
    assert not _eq(again, got) and (again[0]["edge"] != got[0]["edge"]).any()
    # a replaced hit table: refused until it is reduced, then served -- the records need no ops
    hits, hoff = b.hits()
    b.set_hits(hits, hoff)
    _refused(ctx, b)
    scores, counts = b.score(planted.typer.min_gene_coverage)
    b.reduce_async(best, planted.eng.typing_params(planted.typer))
    _, _, third = _check(b, packed, planted.db, R.FLANK, planted.typer.partial_edge_tolerance, "after kp_batch_set_hits and a reduction", ids)
    assert _eq(third, got)
    b.close()
    assert _eq(planted.batch.rescue(), first)


def test_option_off_refuses_and_allocates_nothing(planted):
    off = Planted(planted.db, rescue=False, names=PICK)
    try:
        second = off.eng.ctx.batch(off.packed)
        off.eng.type_batch(off.typer, second, off.ids, off.genomes)
        before = _native.device_allocations()
        bt = off.eng.type_batch(off.typer, second, off.ids, off.genomes)
        assert _native.device_allocations() == before  # a settled work set, a repeated pass: no buffer grows
        for call in (bt.rescue, bt.rescue_tsv):
            with pytest.raises(ValueError, match="rescue=True"):
                call()
        _refused(off.eng.ctx, second)
        assert _native.device_allocations() == before
        pick = [planted.ids.index(n) for n in PICK]
        assert bt.tsv() == b"".join(planted.bt.tsv().splitlines(keepends=True)[i] for i in pick) and not off.eng.rescue
        # the option set on the same context: the records of the reduction that is already there
        off.eng.ctx.set_option("rescue", 1)
        got, want = second.rescue(), planted.bt.rescue()
        for k, i in enumerate(pick):
            assert got[0][got[1][k] : got[1][k + 1]].tobytes() == want[0][want[1][i] : want[1][i + 1]].tobytes()
        second.close()
    finally:
        off.close()


def test_two_databases_in_one_pass(planted):
    from kaptive_amd.serotyping.core import MultiSerotyper
    from kaptive_amd.synth import make_db

    db_k = make_db("kpsc_k", seed=7, n_loci=3)
    pick = [planted.ids.index(n) for n in ("diverged", "no_hit", "long")]
    genomes, packed = [planted.genomes[i] for i in pick], [planted.packed[i] for i in pick]
    ms = MultiSerotyper([db_k, planted.db], rescue=True)
    try:
        batch = ms.engine.ctx.batch(packed)
        (groups, _), = list(ms.engine.type_stream_groups(ms.serotypers, [(batch, [g.id for g in genomes], genomes)]))
        assert len(groups) == 2
        for k, bt in enumerate(groups):
            sums, kept, pieces = batch.typing(k)
            want = R.restate_batch(sums, pieces, packed, ms.dbs[k], R.FLANK, ms.serotypers[k].partial_edge_tolerance)
            _same(bt.rescue(), want, f"group {k}")
            assert bt.rescue_tsv() == R.tsv(*want, bt.ids, [g.contigs.ids for g in genomes], ms.dbs[k].genes.ids, ms.dbs[k].loci.ids, bt.best_locus,
                                            ms.dbs[k].translations.lengths)  # fmt: skip
        first = planted.bt.rescue()
        got = groups[1].rescue()
        for k, i in enumerate(pick):  # gene indices of a group are its own database's
            assert got[0][got[1][k] : got[1][k + 1]].tobytes() == first[0][first[1][i] : first[1][i + 1]].tobytes()
        assert not groups[0].rescue()[0]["score"].any() or (groups[0].rescue()[0]["score"] < R.MIN_SCORE).all()
        batch.close()
    finally:
        ms.close()


def test_serotyper_and_command_line(planted, tmp_path):
    from kaptive_amd.cli import main
    from kaptive_amd.serotyping.core import Serotyper
    from kaptive_amd.synth import make_db

    pick = [planted.ids.index(n) for n in PICK]
    genomes, ids, packed = [planted.genomes[i] for i in pick], [planted.ids[i] for i in pick], [planted.packed[i] for i in pick]
    typer = Serotyper(planted.db, rescue=True)
    try:
        assert typer.engine.rescue and not typer.engine.cigar  # the alignment passes do nothing more for them
        b = typer.engine.ctx.batch(packed)
        bt = typer.engine.type_batch(typer, b, ids, genomes)
        want = bt.rescue_tsv()
        lines = planted.bt.rescue_tsv().splitlines(keepends=True)
        assert want == b"".join(ln for ln in lines if ln.split(b"\t")[0].decode() in PICK) and want.count(b"\n") == len(bt.rescue()[0])
        loose = bt.rescue_tsv(min_score=0)
        b.close()
    finally:
        typer.engine.close()
    paths = []
    for g in genomes:
        p = tmp_path / f"{g.id}.fasta"
        p.write_bytes(g.contigs.to_fasta())
        paths.append(str(p))
    db_path = str(planted.db.save(tmp_path / "o.npz"))
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "plain.tsv")]) == 0
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--rescue", str(tmp_path / "rs.tsv"), "--batch-size", "4"]) == 0
    assert (tmp_path / "rs.tsv").read_bytes() == _native.RESCUE_HEADER + want
    assert (tmp_path / "out.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "out2.tsv"), "--rescue", str(tmp_path / "rs0.tsv"), "--rescue-min-score", "0"]) == 0
    assert (tmp_path / "rs0.tsv").read_bytes() == _native.RESCUE_HEADER + loose and loose != want
    # beside the other reports and --paf: each file is what it is without --rescue
    others = ["--alleles", str(tmp_path / "al.tsv"), "--breakpoints", str(tmp_path / "bp.tsv"), "--paf", str(tmp_path / "h.paf")]
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o1.tsv"), *others]) == 0
    alone = {f: (tmp_path / f).read_bytes() for f in ("al.tsv", "bp.tsv", "h.paf", "o1.tsv")}
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o1.tsv"), *others, "--rescue", str(tmp_path / "rs2.tsv"), "--rescue-flank", "4096"]) == 0
    assert (tmp_path / "rs2.tsv").read_bytes() == _native.RESCUE_HEADER + want
    assert {f: (tmp_path / f).read_bytes() for f in alone} == alone and alone["o1.tsv"] == (tmp_path / "plain.tsv").read_bytes()
    # a second database: a table per database, and a file is needed
    k_path = str(make_db("kpsc_k", seed=7, n_loci=3).save(tmp_path / "k.npz"))
    assert main(["assembly", db_path, *paths, "--db", k_path, "-o", str(tmp_path / "both.tsv"), "--rescue", str(tmp_path / "both.rs.tsv")]) == 0
    assert (tmp_path / "both.rs.kpsc_o.tsv").read_bytes() == _native.RESCUE_HEADER + want
    assert (tmp_path / "both.rs.kpsc_k.tsv").read_bytes().startswith(_native.RESCUE_HEADER)
    assert main(["assembly", db_path, *paths, "--db", k_path, "-o", str(tmp_path / "x.tsv"), "--rescue", "-"]) == 1  # stdout is refused
    assert not (tmp_path / "x.tsv").exists()
