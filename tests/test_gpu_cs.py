"""cs difference strings of the hits on the device (include/kp_spec.h, CS; kaptive_amd/csrc/kp_cs.hip).  Every string of every hit
is compared, exactly, with the Python yardstick of tests/cs_util.py run on the device's own ops: (1) the small batch of
tests/cigar_util.py, (2) the join-limits batch of tests/join_limits_util.py (joined paths, cross gaps up to 500 columns, the
24 000-base gene), (3) a hand-built batch that plants what those two do not guarantee -- a 12 000-column clean copy, substitutions
at chosen columns with the target start at every residue modulo 16 in both orientations, an N run across a word edge, a gene
that holds an n.  Then the buffer's grow-and-rewrite, determinism and lifetime, the option off, the library and the command line."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.pack import pack_sequences_flat
from tests import cigar_util as U
from tests import cs_util as S
from tests import join_limits_util as J
from tests.test_gpu_parity import _same_records

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = -4, -1


class Run:
    """One batch aligned on a context of its own: hits, and what the options left of CIGARs and cs strings."""

    def __init__(self, genes, genomes, cigar=0, cs=1, **options):
        self.genomes = genomes
        self.codes, self.off = pack_sequences_flat(genes)
        self.packed = [g.packed() for g in genomes]
        self.ctx = _native.Context(0)
        self.ctx.load_genes(self.codes, self.off)
        for k, v in options.items():
            self.ctx.set_option(k, v)
        self.ctx.set_option("cigar", cigar)
        self.ctx.set_option("cs", cs)
        self.batch = self.ctx.batch(self.packed)
        self.hits, self.hoff = self.batch.align()
        self.stats = self.batch.stats()
        if cigar or cs:
            self.ops, self.coff = self.batch.cigars()
        if cs:
            self.cs, self.csoff = self.batch.cs()
            self.blob = self.cs.tobytes()

    def string(self, i) -> bytes:
        return self.blob[self.csoff[i] : self.csoff[i + 1]]

    def cigar(self, i):
        return self.ops[self.coff[i] : self.coff[i + 1]]

    def yardstick(self):
        """cs_from_ops on the device's own ops, for every hit, in the table's order."""
        out = []
        for a, pa in enumerate(self.packed):
            asm = U.assembly_codes(pa)
            out.extend(S.hit_cs_yardstick(self.hits[i], self.cigar(i), self.codes, self.off, pa, asm) for i in range(self.hoff[a], self.hoff[a + 1]))
        return out

    def close(self):
        self.batch.close()
        self.ctx.close()


def _with_oracle(oracle, genes, genomes):
    run = Run(genes, genomes)
    odb = oracle.OracleDB(run.codes, run.off)
    return run, [odb.align(pa) for pa in run.packed], run.yardstick()


@pytest.fixture(scope="module")
def small(oracle):
    db = U.small_db()
    run, want, yard = _with_oracle(oracle, db.genes, U.small_batch(db))
    yield db, run, want, yard
    run.close()


@pytest.fixture(scope="module")
def joins(oracle):
    sides = J.join_limit_cases()
    run, want, yard = _with_oracle(oracle, J.database().genes, [s.asm for s in sides])
    yield sides, run, want, yard
    run.close()


@pytest.fixture(scope="module")
def hand(oracle):
    seqs, genes = S.hand_genes()
    run, want, yard = _with_oracle(oracle, seqs, [S.hand_assembly(genes)])
    yield genes, run, want, yard
    run.close()


def _check_batch(run, want, yard, genes):
    """Hits are the oracle's, ops those of a cigar-only run, every string the yardstick's and consistent with its hit."""
    for a, g in enumerate(run.genomes):
        _same_records(run.hits[run.hoff[a] : run.hoff[a + 1]], want[a], f"{g.id}: hits with cs=1")
    plain = Run(genes, run.genomes, cigar=1, cs=0)
    try:
        assert plain.hits.tobytes() == run.hits.tobytes() and plain.coff.tobytes() == run.coff.tobytes() and plain.ops.tobytes() == run.ops.tobytes()
        assert _native.lib().kp_batch_cs(plain.ctx._h, plain.batch._h, None, 0) == ESTATE
    finally:
        plain.close()
    assert len(run.csoff) == len(run.hits) + 1 and run.csoff[0] == 0 and run.csoff[-1] == len(run.cs) and len(yard) == len(run.hits)
    for i, y in enumerate(yard):
        got = run.string(i)
        assert got == y, f"hit {i} {run.hits[i]}: device {got[:100]!r} vs yardstick {y[:100]!r}"
        S.check_cs(y, run.cigar(i), f"hit {i}", matches=run.hits[i]["matches"])
        toks = S.TOKEN.findall(y)
        assert toks[0][:1] == b":" and toks[-1][:1] == b":", f"hit {i}: a path begins and ends on a match"


# ---- 1. the small batch ----------------------------------------------------------------------------------------------------------------
def test_small_batch(small):
    db, run, want, yard = small
    assert len(run.hits) >= 60 and {int(s) for s in run.hits["strand"]} == {-1, 1}
    _check_batch(run, want, yard, db.genes)
    assert any(b"*n" in y for y in yard) and any(b"+" in y for y in yard) and any(b"-" in y for y in yard)


# ---- 2. the join limits ---------------------------------------------------------------------------------------------------------------
def test_join_limits_batch(joins):
    sides, run, want, yard = joins
    _check_batch(run, want, yard, J.database().genes)
    long_gaps = sum(1 for y in yard if any(t[:1] in (b"+", b"-") and len(t) - 1 >= 33 for t in S.TOKEN.findall(y)))
    assert long_gaps >= 20, f"{long_gaps} hits with a + or - token of 33 or more letters"
    assert any(int(t[1:]) >= 10000 for y in yard for t in S.TOKEN.findall(y) if t[:1] == b":")  # a five-digit run: the 24 000-base gene


# ---- 3. the hand-built batch ----------------------------------------------------------------------------------------------------------
def test_hand_built_batch(hand):
    genes, run, want, yard = hand
    _check_batch(run, want, yard, S.hand_genes()[0])
    pa, hits = run.packed[0], want[0]
    # what the batch was built for, read off the oracle's hits and the yardstick's strings
    by_gene = {g: [i for i in range(len(run.hits)) if run.hits[i]["gene"] == g] for g in range(4)}
    assert [(int(h["gene"]), int(h["q_start"]), int(h["q_end"])) for h in hits if h["gene"] == S.BIG] == [(S.BIG, 0, 12000)]
    assert [yard[i] for i in by_gene[S.BIG]] == [b":12000"]
    subs = [h for h in hits if h["gene"] == S.SUB]
    assert len(subs) == 32 and all(h["q_start"] == 0 and h["q_end"] == 700 for h in subs)  # every copy is one hit
    for strand in (1, -1):
        starts = {(int(pa.ctg_start[h["contig"]]) + int(h["t_start"])) % 16 for h in subs if h["strand"] == strand}
        assert starts == set(range(16)), f"strand {strand}: target starts modulo 16 {sorted(starts)}"
    for i in by_gene[S.SUB]:
        cols, at = [], 0
        for t in S.TOKEN.findall(yard[i]):
            if t[:1] == b"*":
                cols.append(at)
            at += int(t[1:]) if t[:1] == b":" else 1
        fwd = cols if run.hits[i]["strand"] > 0 else sorted(699 - c for c in cols)
        assert tuple(fwd) == S.SUB_COLUMNS, f"hit {i}: substituted columns {fwd}"
    (i_run,) = by_gene[S.RUN]
    assert b"*n" in yard[i_run] and S.TOKEN.findall(yard[i_run])[1:4] == [t for t in S.TOKEN.findall(yard[i_run]) if t[:2] == b"*n"]
    first_n = int(pa.ctg_start[run.hits[i_run]["contig"]]) + int(run.hits[i_run]["t_start"]) + int(S.TOKEN.findall(yard[i_run])[0][1:])
    assert first_n % 16 == 15 and pa.n_runs.tolist() == [[first_n, first_n + 3]]  # the run straddles a word edge
    (i_n,) = by_gene[S.WITH_N]
    assert yard[i_n] == b":400*cn:399"


# ---- 4. grow and re-emit -----------------------------------------------------------------------------------------------------------------
def test_a_small_first_guess_grows_the_buffer_without_another_pass(joins):
    sides, run, _, _ = joins
    assert run.csoff[-1] > len(run.hits)  # more than one byte per hit: a buffer of one per hit is too small
    tight = Run(J.database().genes, run.genomes, cs_bytes_per_hit=1)
    try:
        assert tight.hits.tobytes() == run.hits.tobytes()
        assert tight.coff.tobytes() == run.coff.tobytes() and tight.ops.tobytes() == run.ops.tobytes()
        assert tight.csoff.tobytes() == run.csoff.tobytes() and tight.blob == run.blob
        assert tight.stats["retries"] == run.stats["retries"], "growing the cs buffer must not rerun the alignment pass"
    finally:
        tight.close()


# ---- 5. determinism and lifetime --------------------------------------------------------------------------------------------------------
def test_determinism_and_lifetime(joins):
    sides, run, _, _ = joins
    lib = _native.lib()
    again = run.ctx.batch(run.packed)
    hits, hoff = again.align()
    data, off = again.cs()
    assert hits.tobytes() == run.hits.tobytes() and off.tobytes() == run.csoff.tobytes() and data.tobytes() == run.blob
    # the first batch's strings, read after a second batch was aligned and waited for on the same context
    data0, off0 = run.batch.cs()
    assert off0.tobytes() == run.csoff.tobytes() and data0.tobytes() == run.blob
    # kp_batch_set_hits discards them: they described the table that was replaced
    again.set_hits(hits, hoff)
    off_buf = np.zeros(len(hits) + 1, np.int64)
    assert lib.kp_batch_cs(run.ctx._h, again._h, None, 0) == ESTATE
    assert lib.kp_batch_cs_offsets(run.ctx._h, again._h, off_buf.ctypes.data_as(C.c_void_p)) == ESTATE
    # a buffer that is too small is refused
    small_buf = np.zeros(1, np.uint8)
    assert lib.kp_batch_cs(run.ctx._h, run.batch._h, small_buf.ctypes.data_as(C.c_void_p), C.c_int64(1)) == EINVAL
    again.close()


# ---- 6. the option off ----------------------------------------------------------------------------------------------------------------------
def test_option_off_allocates_nothing_and_changes_nothing(small):
    db, run, _, _ = small
    ctx = _native.Context(0)
    ctx.load_genes(run.codes, run.off)
    ctx.set_option("cs", 0)
    first = ctx.batch(run.packed)
    first.align()
    before = _native.device_allocations()
    second = ctx.batch(run.packed)
    hits, _ = second.align()
    assert _native.device_allocations() == before  # a settled context, a repeated batch: nothing grows
    assert hits.tobytes() == run.hits.tobytes()
    off_buf = np.zeros(len(hits) + 1, np.int64)
    assert _native.lib().kp_batch_cs(ctx._h, second._h, None, 0) == ESTATE
    assert _native.lib().kp_batch_cs_offsets(ctx._h, second._h, off_buf.ctypes.data_as(C.c_void_p)) == ESTATE
    assert _native.lib().kp_batch_cigars(ctx._h, second._h, None, 0) == ESTATE  # (cs = 0 asks for no CIGARs either)
    with pytest.raises(_native.NativeError):
        second.cs()
    for b in (first, second):
        b.close()
    ctx.set_option("cigar", 1)  # cigar = 1, cs = 0: the ops of the cs = 1 run, and still no strings
    third = ctx.batch(run.packed)
    third.align()
    ops, coff = third.cigars()
    assert ops.tobytes() == run.ops.tobytes() and coff.tobytes() == run.coff.tobytes()
    assert _native.lib().kp_batch_cs(ctx._h, third._h, None, 0) == ESTATE
    third.close()
    ctx.close()


def test_typed_rows_do_not_depend_on_the_option(small):
    from kaptive_amd.engine import Engine
    from kaptive_amd.serotyping.core import Serotyper

    db, run, _, _ = small
    rows = []
    for cs in (False, True):
        eng = Engine(db, cs=cs)
        typer = Serotyper(db)
        typer._engine = eng
        batch = eng.ctx.batch(run.packed)
        rows.append(eng.type_batch(typer, batch, [g.id for g in run.genomes]).rows())
        if cs:
            assert batch.cs()[0].tobytes() == run.blob
        batch.close()
        eng.close()
    assert rows[0] == rows[1] and len(rows[0]) == len(run.genomes)


# ---- 7. library and command line ----------------------------------------------------------------------------------------------------------
def _write_inputs(db, genomes, tmp_path):
    paths = []
    for g in genomes:
        p = tmp_path / f"{g.id}.fasta"
        p.write_bytes(g.contigs.to_fasta())
        paths.append(str(p))
    return str(db.save(tmp_path / "k.npz")), paths


def test_engine_alignments_and_command_line(small, tmp_path):
    from kaptive_amd.cli import main
    from kaptive_amd.engine import Engine
    from kaptive_amd.synth import make_db

    db, run, _, _ = small
    genomes = run.genomes[:2]
    db_path, paths = _write_inputs(db, genomes, tmp_path)
    eng = Engine(db, cs=True)
    tables = eng.align(genomes)
    eng.close()
    for a, t in enumerate(tables):  # the Alignments carry the batch's strings and CIGARs, row for row
        assert len(t.cs) == len(t.cigars) == len(t) == run.hoff[a + 1] - run.hoff[a]
        assert list(t.cs) == [run.string(i) for i in range(run.hoff[a], run.hoff[a + 1])] and all(isinstance(c, bytes) for c in t.cs)
        assert [t.cigars[i].tolist() for i in range(len(t))] == [run.cigar(i).tolist() for i in range(run.hoff[a], run.hoff[a + 1])]
    names = tuple(db.genes.ids)
    assert b"".join(t.to_paf(names, cs=False, eqx=False) for t in tables) == b"".join(t.to_paf(names) for t in tables)
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "plain.tsv")]) == 0
    for flags, kw in [(["--cs"], dict(cs=True)), (["--eqx"], dict(eqx=True)), (["--cs", "--eqx"], dict(cs=True, eqx=True))]:
        want = b"".join(t.to_paf(names, **kw) for t in tables)
        assert want.count(b"\n") == run.hoff[2] and (b"\tcs:Z::" in want) == ("cs" in kw) and (b"=" in want) == ("eqx" in kw)
        assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--paf", str(tmp_path / "hits.paf"), *flags]) == 0
        assert (tmp_path / "hits.paf").read_bytes() == want, flags
        assert (tmp_path / "out.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()
    # a second database: a file per database, each equal to that database's engine alone
    db_o = make_db("kpsc_o", seed=8)
    o_path = str(db_o.save(tmp_path / "o.npz"))
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "both.tsv"), "--paf", str(tmp_path / "both.paf"), "--cs", "--eqx"]) == 0
    assert (tmp_path / "both.kpsc_k.paf").read_bytes() == b"".join(t.to_paf(names, cs=True, eqx=True) for t in tables)
    eng_o = Engine(db_o, cs=True)
    want_o = b"".join(t.to_paf(tuple(db_o.genes.ids), cs=True, eqx=True) for t in eng_o.align(genomes))
    eng_o.close()
    assert (tmp_path / "both.kpsc_o.paf").read_bytes() == want_o


def test_command_line_on_two_devices(small, tmp_path):
    import subprocess
    import sys

    from kaptive_amd.engine import Engine

    if _native.device_count() < 2:
        pytest.skip("one device")
    db, run, _, _ = small
    db_path, paths = _write_inputs(db, run.genomes, tmp_path)
    from tests.conftest import ROOT

    r = subprocess.run([sys.executable, "-m", "kaptive_amd", "assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--paf",
                        str(tmp_path / "hits.paf"), "--cs", "--eqx", "--devices", "0,1", "--batch-size", "2"], capture_output=True, timeout=600, cwd=str(ROOT))  # fmt: skip
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    eng = Engine(db, cs=True)
    want = b"".join(t.to_paf(tuple(db.genes.ids), cs=True, eqx=True) for t in eng.align(run.genomes))
    eng.close()
    assert (tmp_path / "hits.paf").read_bytes() == want
