"""Allele digests of the kept records and the locus pieces on the device (include/kp_spec.h, ALLELES; kaptive_amd/csrc/kp_alleles.hip).
Every digest of every assembly is compared, exactly, with the numpy restatement of tests/alleles_util.py run on the device's own kept
lists, pieces and proteins, and -- independently of the restatement's interval logic -- with the restatement's digest of the text the
host extracted: (1) one locus planted at every offset of a packed word, reverse-complemented, with a synonymous and a missense
substitution, with N runs, split over two contigs, and an assembly without a hit; (2) hand-made hit tables -- kept lists of 0 to 2048
records, intervals around one and two sweeps of a wave, the shortest ones, one ending on the batch's last base -- put in place with
kp_batch_set_hits and reduced; then lifetime and determinism, the option off, two databases in one pass, the library and the
command line."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from tests import alleles_util as A
from tests import breakpoints_util as P
from tests import cigar_util as U

pytestmark = pytest.mark.gpu

EINVAL = -1
SIZES = (0, 1, 63, 64, 65, 300, 2048)
CODONS = {a + b + c: aa for (a, b, c), aa in zip(((a, b, c) for a in "TCAG" for b in "TCAG" for c in "TCAG"),
                                                 "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG")}  # fmt: skip


def _bases(genome) -> int:
    return int(genome.contigs.lengths.sum())


def _yardstick(batch, packed, group=0):
    """(records, piece digests) of the restatement on a batch's own kept lists, pieces and proteins, laid out as the device's are."""
    sums, kept, pieces = batch.typing(group)
    out, pd = np.zeros(kept.shape, A.ALLELE_DTYPE), np.zeros(pieces.shape, np.uint64)
    for a, pa in enumerate(packed):
        nk, m = int(sums["n_kept"][a]), int(sums["n_pieces"][a])
        k = kept[a, :nk]
        need = int((k["prot_off"] + k["prot_len"]).max()) if nk else 0
        prot = batch.proteins(a, need, group).tobytes() if need else b""
        out[a, :nk], pd[a, :m] = A.restate(k, pieces[a, :m], prot, pa.ctg_start, U.assembly_codes(pa))
    return sums, kept, pieces, out, pd


def _check(batch, packed, label, group=0):
    """The device's digests of the batch's current reduction against the restatement; rows beyond the counts are zero."""
    records, piece_digests = batch.alleles(group)
    sums, kept, pieces, want, want_pd = _yardstick(batch, packed, group)
    assert records.dtype == _native.ALLELE_DTYPE == A.ALLELE_DTYPE and records.shape == kept.shape and piece_digests.shape == pieces.shape, label
    if records.tobytes() != want.tobytes():
        a, i = next((a, i) for a in range(records.shape[0]) for i in range(records.shape[1]) if records[a, i] != want[a, i])
        raise AssertionError(f"{label}: assembly {a} record {i} {kept[a, i]}: device {records[a, i]} vs the restatement's {want[a, i]}")
    assert piece_digests.tobytes() == want_pd.tobytes(), f"{label}: piece digests {piece_digests} vs {want_pd}"
    return sums, kept, pieces, records, piece_digests


@pytest.fixture(scope="module")
def db():
    return P.plant_db()


# ---- 1. the planted locus --------------------------------------------------------------------------------------------------------------------
def _plants(db, flank_len: int = P.FLANK):
    """[(name, genome)] and the edited genes {name: database gene index}."""
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.synth import random_dna, revcomp

    o, n = int(db.loci.offsets[P.PLANT_LOCUS]), int(db.loci.lengths[P.PLANT_LOCUS])
    locus = np.asarray(db.loci.seqs[o : o + n], np.uint8)
    g0 = int(db.locus_gene_offsets[P.PLANT_LOCUS])
    rng = np.random.default_rng(20261020)
    left, right, lead = random_dna(rng, flank_len, 0.5), random_dna(rng, flank_len, 0.5), random_dna(rng, 15, 0.5)

    def gene(k):
        gi = g0 + k
        assert db.gene_intervals.strands[gi] > 0, "the edited genes lie on the locus's forward strand"
        return gi, int(db.gene_intervals.starts[gi]), int(db.gene_intervals.ends[gi])

    def asm(name, *contigs):
        return name, GenomeAssembly(name, Sequences.from_records([SeqRecord(f"{name}_{i}", np.ascontiguousarray(c).tobytes()) for i, c in enumerate(contigs)]))

    def codon(s, want):
        """First codon from the gene's 40th on that `want` accepts: (index of its first base in the locus, its text)."""
        for c in range(40, 200):
            text = locus[s + 3 * c : s + 3 * c + 3].tobytes().decode()
            if want(text):
                return s + 3 * c, text
        raise AssertionError("no such codon")

    out, edited = [], {}
    for k in range(16):
        out.append(asm(f"shift{k}", np.concatenate([lead[:k], left, locus, right])))
    out.append(asm("reversed", revcomp(np.concatenate([left, locus, right]))))
    gi, s, _ = gene(1)  # a third base that does not change the amino acid
    at, text = codon(s, lambda t: CODONS[t] == CODONS[t[:2] + ("A" if t[2] != "A" else "C")] and CODONS[t] != "*")
    copy = locus.copy()
    copy[at + 2] = ord("A" if text[2] != "A" else "C")
    out.append(asm("synonymous", np.concatenate([left, copy, right])))
    edited["synonymous"] = gi
    gi, s, _ = gene(2)  # a second base that does, and makes no stop
    at, text = codon(s, lambda t: CODONS[t] not in ("*", CODONS[t[0] + ("C" if t[1] != "C" else "T") + t[2]]) and CODONS[t[0] + ("C" if t[1] != "C" else "T") + t[2]] != "*")
    copy = locus.copy()
    copy[at + 1] = ord("C" if text[1] != "C" else "T")
    out.append(asm("missense", np.concatenate([left, copy, right])))
    edited["missense"] = gi
    gi, s, _ = gene(3)
    copy = locus.copy()
    copy[s + 200] = ord("N")
    out.append(asm("one_n", np.concatenate([left, copy, right])))
    edited["one_n"] = gi
    gi, s, _ = gene(1)
    copy = locus.copy()
    copy[s + 310 : s + 330] = ord("N")  # twenty bases: they cross an edge of the digest's sixteen-column blocks wherever the hit starts
    out.append(asm("n_run", np.concatenate([left, copy, right])))
    edited["n_run"] = gi
    gi, s, _ = gene(2)
    out.append(asm("split", np.concatenate([left, locus[: s + 500]]), np.concatenate([locus[s + 500 :], right])))
    out.append(asm("no_hit", random_dna(np.random.default_rng(99), 30_000, 0.5)))
    return out, edited


class Planted:
    def __init__(self, db, alleles=True):
        from kaptive_amd.engine import Engine
        from kaptive_amd.serotyping.core import Serotyper

        self.db = db
        plants, self.edited = _plants(db)
        self.genomes = [g for _, g in plants]
        self.ids = [g.id for g in self.genomes]
        self.packed = [g.packed() for g in self.genomes]
        self.eng = Engine(db, alleles=alleles)
        self.typer = Serotyper(db)
        self.typer._engine = self.eng
        self.batch = self.eng.ctx.batch(self.packed)
        self.bt = self.eng.type_batch(self.typer, self.batch, self.ids, self.genomes)

    def tsv(self, bt=None) -> bytes:
        bt = self.bt if bt is None else bt
        records, piece_digests = bt.alleles()
        return A.format_tsv(bt.ids, [g.contigs.ids for g in self.genomes], self.db.genes.ids, self.db.loci.ids, bt.best_locus, bt.sums["n_kept"], bt.kept,
                            records, bt.sums["n_pieces"], bt.pieces, piece_digests)  # fmt: skip

    def close(self):
        self.batch.close()
        self.eng.close()


@pytest.fixture(scope="module")
def planted(db):
    run = Planted(db)
    yield run
    run.close()


def _alive(bt, a):
    return [i for i in range(int(bt.sums["n_kept"][a])) if not int(bt.kept["flags"][a, i]) & A.F_SPURIOUS]


def _by_gene(bt, records, a):
    """{gene: sorted [(nt, aa)]} of assembly a's reported records."""
    out: dict = {}
    for i in _alive(bt, a):
        out.setdefault(int(bt.kept["gene"][a, i]), []).append((int(records["nt"][a, i]), int(records["aa"][a, i])))
    return {g: sorted(v) for g, v in out.items()}


def test_planted_locus_against_the_restatement_and_the_hosts_text(planted):
    bt = planted.bt
    assert max(_bases(g) for g in planted.genomes) <= 90_000
    records, piece_digests = bt.alleles()
    sums, kept, pieces, got, got_pd = _check(planted.batch, planted.packed, "planted")
    assert got.tobytes() == records.tobytes() and got_pd.tobytes() == piece_digests.tobytes() and kept.tobytes() == bt.kept.tobytes()
    locus = bt.locus_alleles()
    assert locus.dtype == np.uint64 and locus.shape == (len(planted.ids),)
    # the text the host extracted: gene by gene, protein by protein, piece by piece
    nt_of, aa_of = {}, {}
    for a in range(len(planted.ids)):
        r, alive = bt.result(a), _alive(bt, a)
        genes, prots, parts = list(r.gene_seqs), list(r.translations), list(r.locus_seqs)
        assert len(genes) == len(prots) == len(alive) and len(parts) == int(sums["n_pieces"][a])
        for i, g, p in zip(alive, genes, prots):
            assert A.nt_digest(A.text_codes(g.seq)) == int(records["nt"][a, i]), (planted.ids[a], i)
            assert len(p.seq) == int(kept["prot_len"][a, i])
            assert (A.aa_digest(p.seq) if len(p.seq) else 0) == int(records["aa"][a, i]), (planted.ids[a], i)
            nt_of.setdefault(bytes(g.seq).upper(), set()).add(int(records["nt"][a, i]))
            if len(p.seq):
                aa_of.setdefault(bytes(p.seq), set()).add(int(records["aa"][a, i]))
        want = A.locus_digest([A.nt_digest(A.text_codes(x.seq)) for x in parts], range(len(parts)))
        assert int(locus[a]) == want and (want != 0) == (len(parts) > 0), planted.ids[a]
    # equal digests, equal texts -- and the other way round
    for table in (nt_of, aa_of):
        assert all(len(v) == 1 for v in table.values()) and len({next(iter(v)) for v in table.values()}) == len(table) > 10
    a = planted.ids.index("no_hit")
    assert sums["n_kept"][a] == 0 and sums["n_pieces"][a] == 0 and locus[a] == 0 and not records[a].view(np.uint64).any()
    a = planted.ids.index("split")
    assert sums["n_pieces"][a] == 2 and locus[a] != locus[0]
    for name in ("one_n", "n_run"):
        a = planted.ids.index(name)
        assert sum(int((U.assembly_codes(planted.packed[a])[int(pc["start"]) : int(pc["end"])] == 4).sum()) for pc in pieces[a, : sums["n_pieces"][a]]) in (1, 20)
        assert locus[a] != locus[0] and _by_gene(bt, records, a) != _by_gene(bt, records, 0)
    assert bt.alleles_tsv() == planted.tsv() and bt.alleles_tsv().count(b"\n") == sum(len(_alive(bt, a)) for a in range(len(planted.ids)))


def test_shifted_and_reversed_copies_agree_and_substitutions_show(planted):
    bt = planted.bt
    records, _ = bt.alleles()
    locus = bt.locus_alleles()
    base = _by_gene(bt, records, 0)
    assert len(base) >= 5 and locus[0] != 0
    offsets = set()
    for k in range(16):
        a = planted.ids.index(f"shift{k}")
        assert _by_gene(bt, records, a) == base and locus[a] == locus[0], f"shift{k}"
        pa = planted.packed[a]
        offsets.add((int(pa.ctg_start[0]) + int(bt.pieces["start"][a, 0])) % 16)
    assert offsets == set(range(16)), "the locus sits at every offset of a packed word"
    a = planted.ids.index("reversed")
    assert _by_gene(bt, records, a) == base and locus[a] == locus[0]
    strand_of = lambda a: {int(bt.kept["gene"][a, i]): int(bt.kept["strand"][a, i]) for i in _alive(bt, a)}  # noqa: E731
    assert all(strand_of(a)[g] == -s for g, s in strand_of(0).items() if len(base[g]) == 1), "every gene is read off the other strand"
    # a synonymous substitution: one gene's bases and the locus change, no protein does
    a, gi = planted.ids.index("synonymous"), planted.edited["synonymous"]
    got = _by_gene(bt, records, a)
    assert set(got) == set(base) and [g for g in base if got[g] != base[g]] == [gi] and locus[a] != locus[0]
    assert [aa for _, aa in got[gi]] == [aa for _, aa in base[gi]] and [nt for nt, _ in got[gi]] != [nt for nt, _ in base[gi]]
    # a missense substitution: that one gene's bases and protein
    a, gi = planted.ids.index("missense"), planted.edited["missense"]
    got = _by_gene(bt, records, a)
    assert set(got) == set(base) and [g for g in base if got[g] != base[g]] == [gi] and locus[a] != locus[0]
    assert len(got[gi]) == len(base[gi]) == 1 and got[gi][0][0] != base[gi][0][0] and got[gi][0][1] != base[gi][0][1]


# ---- 2. hand-made hit tables -------------------------------------------------------------------------------------------------------------------
class HandMade:
    """Assemblies whose hit tables are made by hand, put in place with kp_batch_set_hits."""

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
        self.best, _, _ = B.choose_best_loci(scores, counts, self.typer._expected_genes_per_locus)
        prm = self.eng.typing_params(self.typer)
        prm.id_threshold = id_threshold
        self.batch.reduce_async(self.best, prm)

    def close(self):
        self.batch.close()
        self.eng.close()


LONG = ((1023, 1, 5), (1024, -1, 1100), (1025, 1, 2200), (2048 + 17, -1, 3300), (1, 1, 5400), (2, -1, 5410), (3, 1, 5420), (3, -1, 5431), (17, -1, 5450))
LAST_CONTIG = 800  # fifty packed words: the contig ends on a word edge


def _long_assembly(db, name="long"):
    """(genome, hits): intervals around one and two sweeps of a wave and the shortest ones on a first contig, both strands; on the
    last contig a record that ends on its last base and one that starts on its first."""
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.synth import random_dna

    rng = np.random.default_rng(1024)
    contigs = [random_dna(rng, 6000, 0.5), random_dna(rng, LAST_CONTIG, 0.5)]
    contigs[0][1500:1503] = ord("N")  # inside the 1024-base interval
    rows = [(0, L, st, t0) for L, st, t0 in LONG] + [(1, 300, 1, 0), (1, 333, -1, LAST_CONTIG - 333)]
    hits = np.zeros(len(rows), _native.HIT_DTYPE)
    for g, (c, L, st, t0) in enumerate(rows):
        h = hits[g]
        h["gene"], h["contig"], h["strand"], h["q_start"], h["q_end"], h["t_start"], h["t_end"] = g, c, st, 0, min(L, int(db.genes.lengths[g])), t0, t0 + L
        h["score"], h["matches"], h["block_len"], h["mapq"] = 2 * L, L, L, 60
    genome = GenomeAssembly(name, Sequences.from_records([SeqRecord(f"{name}_c{i}", np.ascontiguousarray(c).tobytes()) for i, c in enumerate(contigs)]))
    return genome, hits


def _layouts(db):
    out = []
    for n in SIZES:
        rng = np.random.default_rng(727300 + n)
        small = n > 300  # 2048 fragments on 90 kb: 30 bases each
        frag = 30 if small else (200 if n == 300 else 250)
        out.append(P.Layout(rng, db.genes.lengths, frag=frag, contig_len=3000, long_pairs=4 if small else 6, far_gaps=not small).fill(n))
    return out


@pytest.fixture(scope="module")
def hand_made(db):
    layouts = _layouts(db)
    long_genome, long_hits = _long_assembly(db)
    run = HandMade(db, [lay.genome(f"table{n}") for lay, n in zip(layouts, SIZES)] + [long_genome], [lay.hits() for lay in layouts] + [long_hits])
    yield run
    run.close()


def _table(run, sums, kept, pieces, records, piece_digests) -> bytes:
    order = _native.piece_order(pieces, sums["n_pieces"])
    first = np.concatenate([[0], np.cumsum([len(g.contigs.ids) for g in run.genomes])]).astype(np.int64)
    got = _native.format_alleles(run.db.genes.ids, run.db.loci.ids, [g.id for g in run.genomes], [n for g in run.genomes for n in g.contigs.ids], first,
                                 sums["n_kept"], sums["n_pieces"], run.best, kept, records, piece_digests, order)  # fmt: skip
    want = A.format_tsv([g.id for g in run.genomes], [g.contigs.ids for g in run.genomes], run.db.genes.ids, run.db.loci.ids, run.best, sums["n_kept"],
                        kept, records, sums["n_pieces"], pieces, piece_digests)  # fmt: skip
    assert got == want
    return got


def test_hand_made_hit_tables(hand_made):
    run = hand_made
    assert max(_bases(g) for g in run.genomes) <= 90_000, [_bases(g) for g in run.genomes]
    run.reduce(0.0)  # no identity threshold: no record is spurious
    sums, kept, pieces, records, piece_digests = _check(run.batch, run.packed, "hand-made tables")
    assert sums["n_kept"].tolist() == list(SIZES) + [len(LONG) + 2], "the overlap cull keeps every record of these tables"
    assert not (kept["flags"] & A.F_SPURIOUS).any()
    a = len(SIZES)
    k = kept[a, : sums["n_kept"][a]]
    assert sorted((k["t_end"] - k["t_start"]).tolist()) == sorted([L for L, _, _ in LONG] + [300, 333]) and {1, -1} == {int(s) for s in k["strand"]}
    pa = run.packed[-1]
    last = k[(k["contig"] == 1) & (k["t_end"] == LAST_CONTIG)]
    assert len(last) == 1 and int(pa.ctg_len[-1]) == LAST_CONTIG and len(pa.ctg_len) == 2, "a record ends on the last base of the batch's last contig"
    assert run.batch.n_asm == a + 1 and len(np.unique(records["nt"][a, : len(k)])) == len(k)
    full = _table(run, sums, kept, pieces, records, piece_digests)
    assert full.count(b"\n") == int(sums["n_kept"].sum())
    # ... and with a threshold that makes a fifth of the records outside the locus spurious: they keep their digests and leave the table
    outside = np.concatenate([kept["pident"][a, :n][(kept["flags"][a, :n] & 2) == 0] for a, n in enumerate(sums["n_kept"])])
    assert len(outside) > 500
    run.reduce(float(np.quantile(outside, 0.2)))
    sums2, kept2, pieces2, records2, piece_digests2 = _check(run.batch, run.packed, "hand-made tables with spurious records")
    dead = [(a, i) for a, n in enumerate(sums2["n_kept"]) for i in range(n) if kept2["flags"][a, i] & A.F_SPURIOUS]
    assert 100 < len(dead) < 0.5 * sums2["n_kept"].sum() and all(records2["nt"][a, i] != 0 for a, i in dead)
    assert _table(run, sums2, kept2, pieces2, records2, piece_digests2).count(b"\n") == int(sums2["n_kept"].sum()) - len(dead)


# ---- 3. lifetime and determinism -------------------------------------------------------------------------------------------------------------
def _refused(ctx, batch):
    lib = _native.lib()
    out, pd = np.zeros((batch.n_asm, 4), _native.ALLELE_DTYPE), np.zeros((batch.n_asm, 4), np.uint64)
    rc = lib.kp_batch_alleles(ctx._h, batch._h, out.ctypes.data_as(C.c_void_p), C.c_int32(4), pd.ctypes.data_as(C.c_void_p), C.c_int32(4))
    assert rc == EINVAL, rc
    assert b"kp_batch_reduce has not run" in lib.kp_last_error(ctx._h)
    with pytest.raises(ValueError):
        batch.alleles()


def _same(x, y):
    return x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()


def test_lifetime_and_determinism(planted):
    from kaptive_amd.serotyping import batch as B

    ctx = planted.eng.ctx
    first = planted.bt.alleles()
    assert _same(planted.batch.alleles(), first)  # a second call: the same bytes
    b = ctx.batch(planted.packed)
    _refused(ctx, b)  # never aligned
    b.align_async()
    b.wait()
    _refused(ctx, b)  # aligned, not reduced
    bt = planted.eng.type_batch(planted.typer, b, planted.ids, planted.genomes, aligned=True)  # ... and the context types it as usual
    assert _same(bt.alleles(), first) and bt.tsv() == planted.bt.tsv()
    lib = _native.lib()
    kc, pc = first[0].shape[1], first[1].shape[1]
    out, pd = np.zeros((b.n_asm, kc), _native.ALLELE_DTYPE), np.zeros((b.n_asm, pc), np.uint64)
    for ks, ps in ((kc - 1, pc), (kc, int(planted.bt.sums["n_pieces"].max()) - 1)):  # strides that are too small are refused
        assert lib.kp_batch_alleles(ctx._h, b._h, out.ctypes.data_as(C.c_void_p), C.c_int32(ks), pd.ctypes.data_as(C.c_void_p), C.c_int32(ps)) == EINVAL
        assert b"strides too small" in lib.kp_last_error(ctx._h)
    # the next reduction of the group replaces the kept list: its digests are gone and made again (an identity threshold above 100
    # makes every record outside the locus spurious)
    scores, counts = b.score(planted.typer.min_gene_coverage)
    best, _, _ = B.choose_best_loci(scores, counts, planted.typer._expected_genes_per_locus)
    prm = planted.eng.typing_params(planted.typer)
    prm.id_threshold = 101.0
    b.reduce_async(best, prm)
    _check(b, planted.packed, "after a second reduction")
    # a replaced hit table: refused until it is reduced, then served -- the digests need no ops
    hits, hoff = b.hits()
    b.set_hits(hits, hoff)
    _refused(ctx, b)
    scores, counts = b.score(planted.typer.min_gene_coverage)
    b.reduce_async(best, planted.eng.typing_params(planted.typer))
    _, _, _, records, piece_digests = _check(b, planted.packed, "after kp_batch_set_hits and a reduction")
    assert _same((records, piece_digests), first)
    b.close()
    assert _same(planted.batch.alleles(), first)  # the first batch's digests, after all that went through the same context


def test_option_off_changes_nothing_and_the_device_call_needs_no_option(planted):
    off = Planted(planted.db, alleles=False)
    try:
        second = off.eng.ctx.batch(off.packed)
        off.eng.type_batch(off.typer, second, off.ids, off.genomes)
        before = _native.device_allocations()
        bt = off.eng.type_batch(off.typer, second, off.ids, off.genomes)
        assert _native.device_allocations() == before  # a settled work set, a repeated pass: no buffer grows
        for call in (bt.alleles, bt.locus_alleles, bt.alleles_tsv):
            with pytest.raises(ValueError, match="alleles=True"):
                call()
        assert bt.tsv() == planted.bt.tsv() and bt.kept.tobytes() == planted.bt.kept.tobytes()
        got = second.alleles()  # the device call itself needs no option
        assert _same(got, planted.bt.alleles())
        off.eng.type_batch(off.typer, second, off.ids, off.genomes)
        assert _same(second.alleles(), got) and _native.device_allocations() == before  # ... nor do the digests' buffers, asked for again
        second.close()
    finally:
        off.close()


# ---- 4. two databases in one pass ------------------------------------------------------------------------------------------------------------
def test_two_databases_in_one_pass(planted):
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.serotyping.core import MultiSerotyper
    from kaptive_amd.synth import make_db, random_dna

    db_o = make_db("kpsc_o", seed=8)
    rng = np.random.default_rng(78)
    o, n = int(db_o.loci.offsets[0]), int(db_o.loci.lengths[0])
    o_contig = np.concatenate([random_dna(rng, 3000, 0.5), np.asarray(db_o.loci.seqs[o : o + n], np.uint8), random_dna(rng, 3000, 0.5)])
    genomes = []
    short = dict(_plants(planted.db, flank_len=12_000)[0])  # (room for the O locus within 90 kb)
    for name in ("shift3", "no_hit", "split"):  # each with the O locus on a contig of its own
        g = short[name]
        recs = [SeqRecord(str(i), bytes(g.contigs.seqs[s : s + m])) for i, s, m in zip(g.contigs.ids, g.contigs.offsets, g.contigs.lengths)]
        genomes.append(GenomeAssembly(g.id, Sequences.from_records(recs + [SeqRecord("o_locus", o_contig.tobytes())])))
    assert max(_bases(g) for g in genomes) <= 90_000
    ms = MultiSerotyper([planted.db, db_o], alleles=True)
    try:
        packed = [g.packed() for g in genomes]
        batch = ms.engine.ctx.batch(packed)
        (groups, _), = list(ms.engine.type_stream_groups(ms.serotypers, [(batch, [g.id for g in genomes], genomes)]))
        assert len(groups) == 2
        for k, bt in enumerate(groups):
            records, piece_digests = bt.alleles()
            sums, kept, pieces, want, want_pd = _yardstick(batch, packed, group=k)
            assert kept.tobytes() == bt.kept.tobytes() and records.tobytes() == want.tobytes() and piece_digests.tobytes() == want_pd.tobytes(), k
            assert bt.alleles_tsv() == A.format_tsv(bt.ids, [g.contigs.ids for g in genomes], ms.dbs[k].genes.ids, ms.dbs[k].loci.ids, bt.best_locus,
                                                    sums["n_kept"], kept, records, sums["n_pieces"], pieces, piece_digests)  # fmt: skip
        bk, bo = groups
        assert bk.sums["n_kept"].tolist()[1] == 0 and (bo.sums["n_kept"] > 0).all()
        lo = bo.locus_alleles()
        assert lo[0] == lo[1] == lo[2] != 0, "the same O locus in all three"
        assert bk.locus_alleles()[0] == planted.bt.locus_alleles()[0] and bk.locus_alleles()[1] == 0
        g0 = int(db_o.locus_gene_offsets[0])
        assert {int(g) for g in bo.kept["gene"][0, _alive(bo, 0)]} >= set(range(g0, g0 + int(db_o.locus_gene_lengths[0])))  # gene indices of a group are its own database's
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

    pick = [planted.ids.index(n) for n in ("shift0", "shift5", "reversed", "synonymous", "no_hit", "missense", "one_n", "n_run", "split")]
    genomes, ids, packed = [planted.genomes[i] for i in pick], [planted.ids[i] for i in pick], [planted.packed[i] for i in pick]
    typer = Serotyper(planted.db, alleles=True)
    try:
        assert typer.engine.alleles and not typer.engine.cigar  # the alignment passes do nothing more for them
        b = typer.engine.ctx.batch(packed)
        bt = typer.engine.type_batch(typer, b, ids, genomes)
        want = bt.alleles_tsv()
        records, piece_digests = bt.alleles()
        assert want == A.format_tsv(ids, [g.contigs.ids for g in genomes], planted.db.genes.ids, planted.db.loci.ids, bt.best_locus, bt.sums["n_kept"], bt.kept,
                                    records, bt.sums["n_pieces"], bt.pieces, piece_digests)  # fmt: skip
        lines = {ln.split(b"\t")[0]: ln for ln in planted.bt.alleles_tsv().splitlines()}
        assert all(ln in planted.bt.alleles_tsv() for ln in want.splitlines()) and len(lines) == len(planted.ids) - 1
        b.close()
    finally:
        typer.engine.close()
    db_path, paths = _write_inputs(planted.db, genomes, tmp_path)
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "plain.tsv")]) == 0
    # two batches (of 5 and 4 genomes): the genomes appear in input order
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--alleles", str(tmp_path / "al.tsv"), "--batch-size", "5"]) == 0
    assert (tmp_path / "al.tsv").read_bytes() == _native.ALLELES_HEADER + want and _native.ALLELES_HEADER == A.HEADER
    seen = [ln.split(b"\t")[0].decode() for ln in want.splitlines()]
    assert [n for i, n in enumerate(seen) if i == 0 or seen[i - 1] != n] == [n for n in ids if n != "no_hit"]
    assert (tmp_path / "out.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()
    # with --variants, --breakpoints and --paf in the same run: each file is what it is without --alleles
    others = ["--variants", str(tmp_path / "v.tsv"), "--breakpoints", str(tmp_path / "bp.tsv"), "--paf", str(tmp_path / "h.paf")]
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o1.tsv"), *others]) == 0
    alone = {f: (tmp_path / f).read_bytes() for f in ("v.tsv", "bp.tsv", "h.paf", "o1.tsv")}
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o1.tsv"), *others, "--alleles", str(tmp_path / "al2.tsv")]) == 0
    assert (tmp_path / "al2.tsv").read_bytes() == _native.ALLELES_HEADER + want
    assert {f: (tmp_path / f).read_bytes() for f in alone} == alone and alone["o1.tsv"] == (tmp_path / "plain.tsv").read_bytes()
    assert alone["v.tsv"].startswith(_native.VARIANTS_HEADER) and len(alone["h.paf"]) > 0
    # a second database: a table per database
    db_o = make_db("kpsc_o", seed=8)
    o_path = str(db_o.save(tmp_path / "o.npz"))
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "both.tsv"), "--alleles", str(tmp_path / "both.al.tsv")]) == 0
    assert (tmp_path / "both.al.kpsc_k.tsv").read_bytes() == _native.ALLELES_HEADER + want
    assert (tmp_path / "both.al.kpsc_o.tsv").read_bytes() == _native.ALLELES_HEADER  # no O locus in these assemblies: the header alone
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "x.tsv"), "--alleles", "-"]) == 1  # stdout is refused
    assert not (tmp_path / "x.tsv").exists()
