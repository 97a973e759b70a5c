"""The variable sites of locus rows without a device (include/kp_spec.h, SITES): the specification's known answers through the
restatement of tests/sites_util.py and through kaptive_amd/csrc/kp_sites.h under g++; the bit-sliced counter against a plain count at
every number of adds it may take; the transposition; the predicate, MAJOR and INFORMATIVE at every tie and edge; the column-to-gene
mapping at the gene lengths around a block; the header constants and their mirrors; ``kp_format_sites`` and ``kp_format_site_rows``
byte for byte against the restatement's f-strings, their refusals included; ``LocusRows.sites`` / ``sites_tsv`` /
``snp_alignment_tsv`` on hand-made tables with a stand-in for the device handle; the command line's flags."""

from __future__ import annotations

import ctypes as C
import pickle

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.distances import SITE_RECORD_DTYPE, LocusRows
from tests import distances_util as D
from tests import sites_util as SU
from tests.test_distances_cpu import PLAN_1, PLAN_2, ROW_A, ROW_B, _hand_batch, _hand_db


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _known_rows():
    return np.stack([D.unpack(D.gene_blocks(D.codes_of(ROW_A))), D.unpack(D.gene_blocks(D.codes_of(ROW_B))), np.full(32, D.GAP, np.uint8)])


def _recs(*rows):
    out = np.zeros(len(rows), SU.SITE_DTYPE)
    for i, (c, n, nn) in enumerate(rows):
        out[i] = (c, n, nn)
    return out


def _derived(n, n_n, R):
    out = np.zeros(6, np.int32)
    SU.harness().kpy_site_derived(_p(np.array([*n, n_n], np.int32)), R, 0, _p(out))
    return dict(site=bool(out[0]), core=bool(out[1]), alleles=int(out[2]), major=int(out[3]), informative=bool(out[4]), gap=int(out[5]))


# ---- the specification's known answers ---------------------------------------------------------------------------------------------------
def test_known_answers_through_the_restatement_and_the_header():
    codes = _known_rows()
    blocks = D.pack(codes).reshape(3, -1)
    want_blocks = [0xFFC0000000000924, 0xFFC0000000000E79, 0xFFFF000000000000]
    for how in (lambda c, core: (SU.profile(c), SU.sites(c, core), SU.site_blocks(c, SU.sites(c, core)["column"])),
                lambda c, core: SU.harness_sites(D.pack(c).reshape(c.shape[0], -1), SU.CORE if core else 0)):  # fmt: skip
        prof, s, rows = how(codes, False)
        assert len(prof) == 32 and prof["column"].tolist() == list(range(32))
        assert s["column"].tolist() == [2, 3, 4, 9, 10, 11]  # 5 and 8 hold one base and an N
        assert prof[5]["n"].tolist() == [0, 0, 0, 1] and prof[5]["n_n"] == 1 and prof[8]["n"].tolist() == [1, 0, 0, 0] and prof[8]["n_n"] == 1
        assert s[0]["n"].tolist() == [1, 1, 0, 0] and s[0]["n_n"] == 0
        assert [int(x) for x in rows[:, 0]] == want_blocks and rows.shape == (3, 1)
        assert not prof[20:]["n"].any() and not prof[20:]["n_n"].any()  # padding: GAP in every row
        _, s, rows = how(codes, True)
        assert len(s) == 0 and rows.shape == (3, 0)  # row C holds no base anywhere
        _, s, rows = how(codes[:2], True)  # A and B alone: the same six
        assert s["column"].tolist() == [2, 3, 4, 9, 10, 11] and [int(x) for x in rows[:, 0]] == want_blocks[:2]
    assert blocks.shape == (3, 2)
    d = _derived((1, 1, 0, 0), 0, 3)
    assert d == dict(site=True, core=False, alleles=2, major=0, informative=False, gap=1)
    assert (SU.alleles((1, 1, 0, 0)), SU.major((1, 1, 0, 0)), SU.informative((1, 1, 0, 0))) == (2, 0, False)
    assert "".join(SU.TEXT[c] for c in SU.site_codes(codes, [2, 3, 4, 9, 10, 11])[0]) == "acgacg"
    assert SU.alignment_lines("L", ["A", "B", "C"], SU.site_codes(codes, [2, 3, 4, 9, 10, 11])) == b"L\tA\t6\tacgacg\nL\tB\t6\tcgtcgt\nL\tC\t6\t------\n"


# ---- the header, host build ------------------------------------------------------------------------------------------------------------
def test_the_mirrored_constants():
    out = np.zeros(8, np.int32)
    SU.harness().kpy_sites_layout(_p(out))
    assert out.tolist() == [24, SU.THREADS, SU.PLANES, SU.LANE_ROWS, SU.SLAB, 5, SU.CORE, 16]
    assert (_native.SITES_THREADS, _native.SITES_LANE_ROWS, _native.SITES_SLAB, _native.SITES_CORE) == (SU.THREADS, SU.LANE_ROWS, SU.SLAB, SU.CORE)
    assert SU.LANE_ROWS == 2**SU.PLANES - 1 and SU.SLAB == SU.THREADS * SU.LANE_ROWS and SU.THREADS % 64 == 0
    assert _native.SITE_DTYPE == SU.SITE_DTYPE and _native.SITE_DTYPE.itemsize == 24
    assert _native.SITES_HEADER == SU.SITES_HEADER and _native.SNP_ALIGNMENT_HEADER == SU.SNP_ALIGNMENT_HEADER
    rec = np.zeros(1, SU.SITE_DTYPE)
    SU.harness().kpy_site_store(_p(rec), 7, 1, 2, 3, 4, 5)
    assert rec[0]["column"] == 7 and rec[0]["n"].tolist() == [1, 2, 3, 4] and rec[0]["n_n"] == 5


@pytest.mark.parametrize("kind", ("random", "ones", "zeros"))
def test_bit_sliced_counter_against_a_plain_count(kind):
    rng = np.random.default_rng(11)
    h = SU.harness()
    for n in range(SU.LANE_ROWS + 1):  # 0 .. 2^P - 1 adds: the last fills every plane of an all-ones column
        masks = {"random": rng.integers(0, 2**64, n, dtype=np.uint64), "ones": np.full(n, 2**64 - 1, np.uint64), "zeros": np.zeros(n, np.uint64)}[kind]
        got = np.zeros(64, np.int32)
        h.kpy_sites_counter(_p(masks), n, _p(got))
        want = ((masks[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).sum(axis=0) if n else np.zeros(64)
        assert got.tolist() == [int(x) for x in want], (kind, n)
        if kind == "ones":
            assert got.tolist() == [n] * 64


def test_transposition_of_a_wave():
    rng = np.random.default_rng(12)
    h = SU.harness()
    for x in (rng.integers(0, 2**64, 64, dtype=np.uint64), np.uint64(1) << np.arange(64, dtype=np.uint64), np.full(64, 2**64 - 1, np.uint64),
              np.where(np.arange(64) == 5, np.uint64(2**64 - 1), np.uint64(0)).astype(np.uint64)):  # fmt: skip
        got = np.ascontiguousarray(x).copy()
        h.kpy_sites_transpose(_p(got))
        bits = (x[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)  # [lane, bit]
        want = (bits.T << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
        assert got.tolist() == want.tolist()
        assert [bin(int(v)).count("1") for v in got] == [int(v) for v in bits.sum(axis=0)]  # lane j: the lanes that had bit j


def test_predicate_major_and_informative_at_every_tie_and_edge():
    R = 9
    for n, n_n, want in (
        ((1, 1, 0, 0), 0, dict(site=True, core=False, alleles=2, major=0, informative=False, gap=7)),
        ((0, 1, 0, 1), 0, dict(site=True, core=False, alleles=2, major=1, informative=False, gap=7)),  # the tie goes to the first
        ((1, 2, 0, 0), 0, dict(site=True, core=False, alleles=2, major=1, informative=False, gap=6)),
        ((2, 1, 0, 0), 0, dict(site=True, core=False, alleles=2, major=0, informative=False, gap=6)),
        ((0, 0, 2, 2), 0, dict(site=True, core=False, alleles=2, major=2, informative=True, gap=5)),
        ((2, 2, 2, 3), 0, dict(site=True, core=True, alleles=4, major=3, informative=True, gap=0)),
        ((R, 0, 0, 0), 0, dict(site=False, core=False, alleles=1, major=0, informative=False, gap=0)),
        ((0, 0, 0, R), 0, dict(site=False, core=False, alleles=1, major=3, informative=False, gap=0)),
        ((0, 0, 0, 0), R, dict(site=False, core=False, alleles=0, major=0, informative=False, gap=0)),
        ((0, 0, 0, 0), 0, dict(site=False, core=False, alleles=0, major=0, informative=False, gap=R)),
        ((R - 1, 1, 0, 0), 0, dict(site=True, core=True, alleles=2, major=0, informative=False, gap=0)),
        ((R - 2, 1, 0, 0), 1, dict(site=True, core=False, alleles=2, major=0, informative=False, gap=0)),  # core with one N
        ((R - 2, 1, 0, 0), 0, dict(site=True, core=False, alleles=2, major=0, informative=False, gap=1)),  # core with one GAP
        ((1, 0, 0, 0), R - 1, dict(site=False, core=False, alleles=1, major=0, informative=False, gap=0)),  # base + N
    ):
        assert _derived(n, n_n, R) == want, (n, n_n)
        assert (SU.alleles(n), SU.major(n), SU.informative(n)) == (want["alleles"], want["major"], want["informative"])
        codes = np.concatenate([np.full(c, k, np.uint8) for k, c in enumerate((*n, n_n, want["gap"]))])[:, None]
        assert (len(SU.sites(codes)), len(SU.sites(codes, True))) == (int(want["site"]), int(want["core"])), (n, n_n)


def test_column_to_gene_mapping():
    lengths = [1, 15, 16, 17, 32]  # blocks 1, 1, 1, 2, 2: first columns 0, 16, 32, 48, 80; 112 columns
    gb = np.array([(L + 15) // 16 for L in lengths], np.int64)
    h = SU.harness()
    for c in range(-2, 115):
        pos = C.c_int64(-9)
        g = h.kpy_site_gene(_p(gb), len(gb), C.c_int64(c), C.byref(pos))
        first = [0, 16, 32, 48, 80, 112]
        if c < 0 or c >= 112:
            assert g == -1 and SU.gene_of(lengths, c) is None
            continue
        want_g = max(i for i in range(5) if first[i] <= c)
        assert (g, pos.value) == (want_g, c - first[want_g])
        real = SU.gene_of(lengths, c)
        assert (real is None) == (pos.value >= lengths[g])  # padding
        if real is not None:
            assert real == (g, pos.value, sum(lengths[:g]) + pos.value)
    assert SU.gene_of(lengths, 0) == (0, 0, 0) and SU.gene_of(lengths, 1) is None and SU.gene_of(lengths, 111) == (4, 31, 80)  # a first and a last column
    assert SU.gene_of(lengths, 30) == (1, 14, 15) and SU.gene_of(lengths, 31) is None and SU.gene_of(lengths, 64) == (3, 16, 48)
    assert h.kpy_site_gene(None, 0, C.c_int64(0), None) == -1


@pytest.mark.parametrize("R,nb", ((2, 1), (3, 5), (65, 9), (257, 3), (SU.SLAB + 1, 1)))
def test_header_route_against_the_restatement(R, nb):
    codes = D.population(np.random.default_rng([R, nb]), R, nb)
    codes[:, 0] = 2  # every counter plane of the first lanes carries
    codes[R - 1, 0] = 1
    blocks = D.pack(codes).reshape(R, -1)
    for core in (False, True):
        prof, s, rows = SU.harness_sites(blocks, SU.CORE if core else 0)
        want = SU.sites(codes, core)
        assert prof.tobytes() == SU.profile(codes).tobytes() and s.tobytes() == want.tobytes()
        assert rows.tobytes() == SU.site_blocks(codes, want["column"]).tobytes() and rows.shape == (R, (len(want) + 15) // 16)
    # PROPERTY: the differences of every pair over the site matrix are those over the full matrix
    if R <= 65:
        s = SU.sites(codes)
        a, b = D.all_pairs(codes), D.all_pairs(D.unpack(SU.site_blocks(codes, s["column"])))
        assert a["differences"].tolist() == b["differences"].tolist() and a["a"].tolist() == b["a"].tolist()


# ---- kp_format_sites, kp_format_site_rows ------------------------------------------------------------------------------------------------
GENES, LENGTHS = ["wzi", "gene two", "", "g_4"], [16, 17, 31, 20]  # blocks 1, 2, 2, 2: first columns 0, 16, 48, 80


def _both(locus, R, recs, genes=None):
    got = _native.format_sites(locus, GENES, LENGTHS, R, recs, genes=genes)
    shown = GENES if genes is None else [GENES[i] for i in genes]
    assert got == SU.site_lines(locus, shown, LENGTHS, R, recs)
    return got


def test_format_sites_byte_for_byte():
    recs = _recs((0, (1, 1, 0, 0), 0), (15, (0, 0, 5, 2), 1), (16, (2, 2, 2, 3), 0), (32, (0, 1, 0, 1), 7), (78, (3, 0, 0, 3), 0), (99, (0, 8, 1, 0), 0))
    got = _both("KL2", 9, recs)
    assert got.splitlines()[0] == b"KL2\twzi\t1\t1\t9\t1\t1\t0\t0\t0\t7\t2\ta\tno"
    assert got.splitlines()[1] == b"KL2\twzi\t16\t16\t9\t0\t0\t5\t2\t1\t1\t2\tg\tyes"
    assert got.splitlines()[3] == b"KL2\tgene two\t17\t33\t9\t0\t1\t0\t1\t7\t0\t2\tc\tno"  # the one column of the gene's second block
    assert got.splitlines()[4] == b"KL2\t\t31\t64\t9\t3\t0\t0\t3\t0\t3\t2\ta\tyes" and got.splitlines()[5].startswith(b"KL2\tg_4\t20\t84\t9\t")
    assert _both("", 9, recs).startswith(b"\twzi\t1\t1\t9\t") and _both("KL2", 9, recs[:0]) == b""
    assert _both("KL2", 9, recs, genes=[3, 2, 1, 0]).splitlines()[0].startswith(b"KL2\tg_4\t1\t1\t")
    assert _native.format_sites("x", [], [], 0, recs[:0]) == b""


def test_format_sites_refusals():
    good = _recs((0, (1, 1, 0, 0), 0), (20, (2, 0, 1, 0), 0))
    assert _native.format_sites("x", GENES, LENGTHS, 3, good).count(b"\n") == 2
    for bad in (
        _recs((33, (1, 1, 0, 0), 0)),  # padding: gene two has 17 bases
        _recs((79, (1, 1, 0, 0), 0)),  # the last column of gene 2's blocks
        _recs((112, (1, 1, 0, 0), 0)),  # outside the matrix
        _recs((-1, (1, 1, 0, 0), 0)),
        _recs((0, (2, 2, 0, 0), 0)),  # counts that exceed R
        _recs((0, (1, 1, 0, 0), 2)),
        _recs((0, (3, 0, 0, 0), 0)),  # fewer than two non-zero bases
        _recs((0, (0, 0, 0, 0), 3)),
        _recs((0, (-1, 2, 1, 0), 0)),
        _recs((0, (1, 1, 0, 0), -1)),
        _recs((20, (2, 0, 1, 0), 0), (0, (1, 1, 0, 0), 0)),  # not ascending
        _recs((0, (1, 1, 0, 0), 0), (0, (1, 1, 0, 0), 0)),
    ):
        with pytest.raises(ValueError):
            _native.format_sites("x", GENES, LENGTHS, 3, bad)
    with pytest.raises(ValueError):
        _native.format_sites("x", GENES, LENGTHS, 3, good, genes=[0, 1, 2, 4])
    with pytest.raises(ValueError):
        _native.format_sites("x", GENES[:3], LENGTHS, 3, good)
    with pytest.raises(ValueError):
        _native.format_sites("x", GENES, [16, -1, 31, 20], 3, good)
    lib = _native.lib()
    lib.kp_format_sites.restype = C.c_int64
    off, lens, one = np.array([0, 1, 2], np.int64), np.array([16, 5], np.int32), _recs((17, (1, 2, 0, 0), 0))
    call = lambda **kw: lib.kp_format_sites(kw.get("locus", b"x"), C.c_int32(kw.get("locus_len", 1)), b"ab", kw.get("off", _p(off)), C.c_int32(kw.get("n", 2)), None,  # noqa: E731
                                            kw.get("lens", _p(lens)), C.c_int32(kw.get("R", 3)), kw.get("sites", _p(one)), C.c_int64(kw.get("n_sites", 1)), None, C.c_int64(kw.get("cap", 0)))
    assert call() == len(b"x\tb\t2\t18\t3\t1\t2\t0\t0\t0\t0\t2\tc\tno\n")  # the sizing call
    for kw in (dict(cap=8), dict(cap=-1), dict(off=None), dict(lens=None), dict(sites=None), dict(n=-1), dict(n_sites=-1), dict(locus_len=-1), dict(locus=None), dict(R=-1),
               dict(R=2)):  # fmt: skip
        assert call(**kw) == -1, kw


def test_format_site_rows_byte_for_byte_and_refusals():
    rng = np.random.default_rng(13)
    names = ["iso_1", "b", "", "a third name"]
    for S in (1, 15, 16, 17, 40):
        sc = rng.choice(6, (4, S), p=[0.2, 0.2, 0.2, 0.2, 0.1, 0.1]).astype(np.uint8)
        blocks = SU.site_blocks(sc, np.arange(S))
        got = _native.format_site_rows("KL2", names, S, blocks)
        assert got == SU.alignment_lines("KL2", names, sc) and got.count(b"\n") == 4
        assert all(len(ln.split(b"\t")[3]) == S and set(ln.split(b"\t")[3]) <= set(b"acgtn-") for ln in got.splitlines())
        rows = [3, 0, 2, 1]
        assert _native.format_site_rows("KL2", names, S, blocks, rows=rows) == SU.alignment_lines("KL2", [names[i] for i in rows], sc)
    assert _native.format_site_rows("KL2", names, 0, np.zeros((4, 0), np.uint64)) == b""  # a locus without a site writes no line
    assert _native.format_site_rows("KL2", [], 0, np.zeros((0, 0), np.uint64)) == b"" and _native.format_site_rows("KL2", [], 5, np.zeros((0, 1), np.uint64)) == b""
    good = SU.site_blocks(np.zeros((4, 17), np.uint8), np.arange(17))
    assert _native.format_site_rows("x", names, 17, good) == b"".join(f"x\t{n}\t17\t{'a' * 17}\n".encode() for n in names)
    unflagged = good.copy()
    unflagged[2, 1] &= np.uint64(~(1 << 63) & (2**64 - 1))  # padding that is not flagged
    both = good.copy()
    both[1, 0] |= np.uint64((1 << 32) | (1 << 48))  # N and GAP at once
    for bad in (unflagged, both):
        with pytest.raises(ValueError):
            _native.format_site_rows("x", names, 17, bad)
    for kw in (dict(rows=[0, 1, 2, 4]), dict(rows=[0, 1, 2])):
        with pytest.raises(ValueError):
            _native.format_site_rows("x", names, 17, good, **kw)
    with pytest.raises(ValueError):
        _native.format_site_rows("x", names, 33, good)  # rows of two blocks for 33 sites
    with pytest.raises(ValueError):
        _native.format_site_rows("x", names, -1, good)
    lib = _native.lib()
    lib.kp_format_site_rows.restype = C.c_int64
    off, blk = np.array([0, 1, 2], np.int64), np.array([0xFFFC000000000004, 0xFFFC000100000000], np.uint64)
    call = lambda **kw: lib.kp_format_site_rows(kw.get("locus", b"x"), C.c_int32(kw.get("locus_len", 1)), b"ab", kw.get("off", _p(off)), C.c_int32(kw.get("n", 2)), None,  # noqa: E731
                                                C.c_int64(kw.get("S", 2)), kw.get("blocks", _p(blk)), None, C.c_int64(kw.get("cap", 0)))
    assert call() == len(b"x\ta\t2\tac\nx\tb\t2\tna\n")
    for kw in (dict(cap=8), dict(cap=-1), dict(off=None), dict(blocks=None), dict(n=-1), dict(S=-1), dict(locus_len=-1), dict(locus=None), dict(S=1)):
        assert call(**kw) == -1, kw


# ---- LocusRows on hand-made tables ---------------------------------------------------------------------------------------------------------
class _RestatedHandle:
    """Stands in for ``_native.Distances``: the restatement instead of the device."""

    made = 0

    def __init__(self, ctx, rows_matrix):
        type(self).made += 1
        self.ctx, self._h, self.codes, self._cols = ctx, True, D.unpack(np.asarray(rows_matrix, np.uint64)), None

    def profile(self):
        return SU.profile(self.codes)

    def sites(self, core=False):
        s = SU.sites(self.codes, core)
        self._cols = s["column"]
        return s

    def site_rows(self):
        return SU.site_blocks(self.codes, self._cols)

    def pairs(self, max_diff=None, min_compared=0):
        return D.all_pairs(self.codes, max_diff, min_compared)

    def close(self):
        self._h = None


def _db():
    db = _hand_db()
    db.genes.ids = ["g0", "g1", "g2", "g3"]
    return db


def _two_batches(db):
    return _hand_batch(db, 1, ["a0", "a1", "a2", "a3"], PLAN_1, [0, 0, 1, 1]), _hand_batch(db, 2, ["b0", "b1", "b2"], PLAN_2, [0, 1, 0])


def _tuples(rec):
    return [(int(r["locus"]), int(r["gene"]), int(r["position"]), int(r["column"]), tuple(int(x) for x in r["n"]), int(r["n_n"])) for r in rec]


def test_locus_rows_sites_from_hand_made_tables(monkeypatch):
    monkeypatch.setattr(_native, "Distances", _RestatedHandle)
    db = _db()
    lr = LocusRows(db)
    for b in _two_batches(db):
        lr.add(b)  # L0: assemblies 0, 1, 4, 6; L1: 2, 3, 5
    ctx = object()
    for core in (False, True):
        rec = lr.sites(ctx, core)
        assert rec.dtype == SITE_RECORD_DTYPE and _tuples(rec) == SU.run_sites(lr, core)
        assert lr.sites_tsv(ctx, core) == SU.run_sites_tsv(lr, core) and lr.snp_alignment_tsv(ctx, core) == SU.run_alignment_tsv(lr, core)
        assert lr.sites_tsv(ctx, core).count(b"\n") == len(rec)
    rec = lr.sites(ctx)
    assert len(rec) > 4 and set(rec["locus"].tolist()) == {0, 1} and rec["locus"].tolist() == sorted(rec["locus"].tolist())  # loci in database order
    assert all(0 <= r["position"] < db.genes.lengths[r["gene"]] and (r["gene"] < 3) == (r["locus"] == 0) for r in rec)
    assert all(0 <= r["column"] < (64 if r["locus"] == 0 else 20) for r in rec)
    idx, s, blocks = lr.site_rows(ctx, 0)
    assert idx.tolist() == [0, 1, 4, 6] and blocks.shape == (4, (len(s) + 15) // 16) and blocks.tobytes() == SU.site_blocks(D.unpack(lr.locus_matrix(0)[1]), s["column"]).tobytes()
    assert lr.profile(ctx, 1).tobytes() == SU.profile(D.unpack(lr.locus_matrix(1)[1])).tobytes() and len(lr.profile(ctx, 1)) == 32
    made = _RestatedHandle.made
    assert lr.tsv(ctx, None, 0).count(b"\n") == 6 + 3 and _RestatedHandle.made == made  # one handle per locus serves every table
    lr.close()
    lr.sites(ctx)
    assert _RestatedHandle.made == made + 2


def test_a_locus_with_a_single_row_makes_no_device_call(monkeypatch):
    monkeypatch.setattr(_native, "Distances", _RestatedHandle)
    db = _db()
    lr = LocusRows(db)
    lr.add(_hand_batch(db, 1, ["a0", "a1", "a2"], PLAN_1[:3], [0, 0, 1]))
    made = _RestatedHandle.made
    rec = lr.sites(object())
    assert _RestatedHandle.made == made + 1 and set(rec["locus"].tolist()) <= {0}  # the single row needs no handle and has no site
    idx, s, blocks = lr.site_rows(object(), 1)
    assert idx.tolist() == [2] and len(s) == 0 and blocks.shape == (1, 0)
    assert lr.profile(object(), 1).tobytes() == SU.profile(D.unpack(lr.locus_matrix(1)[1])).tobytes() and _RestatedHandle.made == made + 1
    assert lr.sites_tsv(object()) == SU.run_sites_tsv(lr) and lr.snp_alignment_tsv(object()) == SU.run_alignment_tsv(lr)
    assert not any(ln.startswith(b"L1\t") for ln in lr.snp_alignment_tsv(object()).splitlines())


def test_a_site_the_matrix_cannot_have_is_refused(monkeypatch):
    class _Wrong(_RestatedHandle):
        def sites(self, core=False):
            s = super().sites(core)[:1].copy()
            s["column"] = 16 * (self.codes.shape[1] // 16) - 1  # L1's gene has 20 bases: column 31 is padding
            return s

    monkeypatch.setattr(_native, "Distances", _Wrong)
    db = _db()
    lr = LocusRows(db)
    for b in _two_batches(db):
        lr.add(b)
    with pytest.raises(ValueError):
        lr.sites_tsv(object())


def test_sites_after_a_state_and_merge_round_trip(monkeypatch):
    monkeypatch.setattr(_native, "Distances", _RestatedHandle)
    db = _db()
    b1, b2 = _two_batches(db)
    whole = LocusRows(db)
    whole.add(b1)
    whole.add(b2)
    merged = LocusRows(db)
    for b in (b1, b2):
        part = LocusRows(db)
        part.add(b)
        merged.merge(pickle.loads(pickle.dumps(part.state())))  # as it travels between processes
    ctx = object()
    assert merged.sites(ctx).tobytes() == whole.sites(ctx).tobytes() and merged.sites_tsv(ctx) == whole.sites_tsv(ctx) == SU.run_sites_tsv(whole)
    assert merged.snp_alignment_tsv(ctx, True) == whole.snp_alignment_tsv(ctx, True) == SU.run_alignment_tsv(whole, True)


# ---- the command line's flags ---------------------------------------------------------------------------------------------------------------
def test_command_line_flags():
    from kaptive_amd.cli import PAIR_TABLES, build_parser

    ap = build_parser()
    base = ["assembly", "db.npz", "a.fasta"]
    ns = ap.parse_args([*base, "--sites", "s.tsv"])
    assert ns.sites == "s.tsv" and not any(hasattr(ns, f) for f in ("snp_alignment", "core_sites", "mst", "newick", "clusters", "distances", "aligned", "min_compared"))
    ns = ap.parse_args([*base, "--snp-alignment", "a.tsv"])
    assert ns.snp_alignment == "a.tsv" and not any(hasattr(ns, f) for f in ("sites", "core_sites"))
    ns = ap.parse_args([*base, "--sites", "s.tsv", "--core-sites"])
    assert ns.core_sites is True and ns.sites == "s.tsv"
    ns = ap.parse_args([*base, "--snp-alignment", "a.tsv", "--core-sites", "--mst", "m.tsv", "--distances", "d.tsv"])
    assert (ns.snp_alignment, ns.core_sites, ns.mst, ns.distances) == ("a.tsv", True, "m.tsv", "d.tsv")
    assert {"sites", "snp_alignment"} <= set(PAIR_TABLES)
    for bad in (["--core-sites"], ["--core-sites", "--mst", "m.tsv"], ["--sites"], ["--sites", "s.tsv", "--max-distance", "3"], ["--sites", "s.tsv", "--min-compared", "3"]):
        with pytest.raises(SystemExit):
            ap.parse_args([*base, *bad])


def test_stdout_with_several_databases_is_refused(tmp_path):
    from kaptive_amd.cli import main

    g = tmp_path / "a.fasta"
    g.write_text(">c\nACGT\n")
    for flag in ("--sites", "--snp-alignment"):
        assert main(["assembly", str(tmp_path / "k.npz"), str(g), "--db", str(tmp_path / "o.npz"), "-o", str(tmp_path / "x.tsv"), flag, "-"]) == 1
        assert not (tmp_path / "x.tsv").exists()
