"""Variant records, the parts that need no GPU (include/kp_spec.h, VARIANTS): kp_variants.h's per-hit function -- the one the device
kernels give a lane per kept record -- built with g++ (tests/native_harness/variants_harness.cpp) and compared, count and
records, with the Python restatement of tests/variants_util.py on hand-built pairs, each taken on both strands; the same records
read off the yardstick cs string of the pair; the codon table; the storing sink's bounds; kp_format_variants against a Python
formatter; the buffer policy of the records (kp_caps.h)."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.core.seq import CODON_MAP
from tests import cs_util as S
from tests import variants_util as V

M, I, D = S.M, S.I, S.D


def _rng():
    return np.random.default_rng(70707)


def _pair(ops, q0=0, t0=0, trim=None, **kw):
    """(ops, gene as built, asm, q0, t0): ``trim`` cuts the gene behind the hit's last row so that its length is ``trim`` modulo 3."""
    gene, asm = S.build_pair(_rng(), ops, q0=q0, t0=t0, **kw)
    if trim is not None:
        rows = q0 + sum(n for k, n in ops if k != D)
        gene = gene[: rows + (trim - rows) % 3]
        assert len(gene) % 3 == trim and len(gene) >= rows
    return S.ops_of(*ops), gene, asm, q0, t0


GAPS = [(M, 30), (I, 1), (M, 20), (D, 1), (M, 20), (I, 2), (M, 20), (D, 2), (M, 20), (I, 3), (M, 20), (D, 3), (M, 25), (I, 21), (M, 20), (D, 21), (M, 30)]

# name -> the pair; every one is walked as a strand +1 hit of the gene as built and as a strand -1 hit of its reverse complement
PAIRS = {
    "codon positions": _pair([(M, 90)], q0=0, t0=3, sub_rows=(30, 40, 50)),  # rows 30, 40, 50: residues 0, 1, 2 modulo 3
    "first and last column": _pair([(M, 61)], q0=6, t0=9, sub_rows=(6, 66)),
    "gene word edge": _pair([(M, 70)], q0=0, t0=2, sub_rows=(15, 16, 39, 40)),  # r & 7 = 7 and 0
    "contig word edge": _pair([(M, 70)], q0=0, t0=5, sub_rows=(26, 27, 58, 59)),  # t & 15 = 15 and 0 (t = r + 5)
    "two in one codon": _pair([(M, 80)], q0=0, t0=1, sub_rows=(30, 31, 32)),  # three neighbours: two share a codon on either strand
    "gene n": _pair([(M, 80)], q0=3, t0=7, gene_n=(20, 47)),
    "contig N run inside an M op": _pair([(M, 90)], q0=2, t0=7, n_runs=((7 + 40, 3),)),
    "n against n": _pair([(M, 60)], q0=2, t0=11, gene_n=(20,), n_runs=((11 + 18, 1),)),
    "gaps of 1, 2, 3 and 21": _pair(GAPS, q0=5, t0=13, sub_rows=(5 + 29, 5 + 31 + 20, 5 + 100)),  # an SNV before an I op and behind a D op
    "q_start not a multiple of 3": _pair([(M, 50), (I, 2), (M, 40)], q0=4, t0=0, sub_rows=(10, 11, 70)),
    "cut codon, one base": _pair([(M, 64)], q0=0, t0=4, sub_rows=(0, 63), trim=1),
    "cut codon, two bases": _pair([(M, 65)], q0=0, t0=4, sub_rows=(0, 1, 63, 64), trim=2),
    "clean": _pair([(M, 120)], q0=7, t0=21),
    "short ops": _pair([(M, 3), (I, 1), (M, 2), (D, 1), (M, 5), (I, 2), (M, 1), (D, 3), (M, 7), (I, 1), (M, 4)], q0=1, t0=14, sub_rows=(2, 9, 12)),
}
CASES = [(name, strand) for name in PAIRS for strand in (1, -1)]


def _hit(name, strand):
    """(ops, gene forward codes, asm, strand, q_start, q_end, t_abs) of the pair taken on ``strand``."""
    ops, gene, asm, q0, t0 = PAIRS[name]
    rows = int(sum(int(o) >> 4 for o in ops if int(o) & 15 != D))
    if strand > 0:
        return ops, gene, asm, 1, q0, q0 + rows, t0
    return ops, V.revcomp_codes(gene), asm, -1, len(gene) - (q0 + rows), len(gene) - q0, t0  # (the gene as built is the gene as aligned)


def _same_records(got, want, label):
    assert got.dtype == want.dtype and len(got) == len(want), f"{label}: {len(got)} records, the restatement has {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.tobytes() == w.tobytes(), f"{label}: record {i} {g} vs the restatement's {w}"


@pytest.mark.parametrize("name,strand", CASES)
def test_header_against_the_restatement_and_the_cs_string(name, strand):
    ops, gene, asm, strand, qs, qe, t = _hit(name, strand)
    want = V.records_from_ops(ops, gene, asm, strand, qs, qe, t, 0, kept=5)
    count, got, guard = V.harness_variants(ops, gene, asm, strand, qs, qe, t, kept=5)
    assert count == len(want) and guard
    _same_records(got, want, f"{name}, strand {strand}")
    assert (np.diff(want["q_pos"]) >= 0).all(), "records ascend in q_pos"
    assert (want["kept"] == 5).all() and not want["pad"].any()
    # one to one with the cs string of the same pair
    aligned = gene if strand > 0 else V.revcomp_codes(gene)
    cs = S.cs_from_ops(ops, aligned, asm, qs if strand > 0 else len(gene) - qe, t)
    _same_records(V.records_from_cs(cs, gene, strand, qs, qe, t, 0, kept=5), want, f"{name}, strand {strand}, from the cs string")
    toks = S.TOKEN.findall(cs)
    assert len(want) == sum(1 for x in toks if x[:1] != b":")
    assert [int(k) for k in np.sort(want["kind"])] == sorted({b"*": V.SNV, b"-": V.INS, b"+": V.DEL}[x[:1]] for x in toks if x[:1] != b":")


def test_what_the_pairs_were_built_for():
    rec = {c: V.records_from_ops(*_hit(*c)[:7], 0) for c in CASES}
    for strand in (1, -1):
        assert sorted(int(q) % 3 for q in rec["codon positions", strand]["q_pos"]) == [0, 1, 2]
        ops, gene, asm, s, qs, qe, t = _hit("first and last column", strand)
        assert rec["first and last column", strand]["q_pos"].tolist() == [qs, qe - 1]
        two = rec["two in one codon", strand]
        assert len(two) == 3 and len(set((two["q_pos"] // 3).tolist())) < 3  # at least two records share a codon
        # ... each annotated against the unmodified codon: a record's ref_aa is the gene's own amino acid whatever its neighbour did
        g = _hit("two in one codon", strand)[1]
        for v in two:
            c0 = int(v["q_pos"]) // 3 * 3
            assert v["ref_aa"] == CODON_MAP[int(g[c0]) * 25 + int(g[c0 + 1]) * 5 + int(g[c0 + 2])]
        assert (rec["gene n", strand]["ref"] == 4).all() and len(rec["gene n", strand]) == 2
        run = rec["contig N run inside an M op", strand]
        assert len(run) == 3 and (run["alt"] == 4).all() and all(V.effect(v) == b"ambiguous" for v in run)
        nn = rec["n against n", strand]
        assert any(v["ref"] == 4 and v["alt"] == 4 for v in nn)
        gaps = rec["gaps of 1, 2, 3 and 21", strand]
        for kind in (V.INS, V.DEL):
            assert sorted(gaps["len"][gaps["kind"] == kind].tolist()) == [1, 2, 3, 21]
        assert (gaps["kind"] == V.SNV).sum() == 3
        order = gaps["kind"].tolist()
        assert any(a == V.SNV and b != V.SNV or a != V.SNV and b == V.SNV for a, b in zip(order, order[1:]))
        assert _hit("q_start not a multiple of 3", strand)[4] % 3 != 0
        for name, n_cut in (("cut codon, one base", 1), ("cut codon, two bases", 2)):
            cut, n_gene = rec[name, strand], len(_hit(name, strand)[1])
            in_cut = cut[cut["q_pos"] >= n_gene - n_gene % 3]
            assert n_gene % 3 == n_cut and len(in_cut) == n_cut and (in_cut["ref_aa"] == ord("X")).all() and (in_cut["alt_aa"] == ord("X")).all()
            assert (cut[cut["q_pos"] < n_gene - n_gene % 3]["ref_aa"] != ord("X")).all()
        assert len(rec["clean", strand]) == 0
    rev = rec["gaps of 1, 2, 3 and 21", -1]
    assert (np.diff(rev["q_pos"]) >= 0).all() and (np.diff(rev["t_pos"]) <= 0).all()  # ascending on the gene: back to front on the contig


def test_codon_table_is_the_python_translation():
    table = np.zeros(125, np.uint8)
    V.harness().kpy_codon_table(table.ctypes.data_as(C.c_void_p))
    assert table.tobytes() == np.asarray(CODON_MAP, np.uint8).tobytes() and len(CODON_MAP) == 125


@pytest.mark.parametrize("name,strand", [("gaps of 1, 2, 3 and 21", 1), ("gaps of 1, 2, 3 and 21", -1), ("short ops", -1), ("gene word edge", 1)])
def test_storing_sink_stays_inside_its_buffer(name, strand):
    ops, gene, asm, strand, qs, qe, t = _hit(name, strand)
    want = V.records_from_ops(ops, gene, asm, strand, qs, qe, t, 0)
    n = len(want)
    assert n >= 4
    for cap in (0, 1, n - 1, n):
        count, got, guard = V.harness_variants(ops, gene, asm, strand, qs, qe, t, cap=cap)
        assert count == n, f"capacity {cap}: the count is exact whatever the buffer holds"
        assert guard, f"capacity {cap}: a record written beyond the buffer"
        _same_records(got[:cap], want[:cap], f"{name}, strand {strand}, capacity {cap}")
    # a hit whose range starts at record 3 of the buffer: what lies before it is not touched
    count, got, guard = V.harness_variants(ops, gene, asm, strand, qs, qe, t, base=3, cap=3 + n - 2)
    assert count == n and guard and (got[:3].view(np.uint8) == V.GUARD).all()
    _same_records(got[3:], want[: n - 2], "a range inside the buffer")


# ---- kp_format_variants ---------------------------------------------------------------------------------------------------------------
def _formatter_table():
    """Two assemblies (the second without a record) whose records are those of the pairs above, plus hand-made ones for every Effect."""
    from kaptive_amd.serotyping.batch import KEPT_DTYPE

    kept = np.zeros((2, 3), KEPT_DTYPE)
    kept[0]["gene"], kept[0]["contig"], kept[0]["strand"] = [2, 0, 1], [1, 0, 1], [1, -1, 1]
    recs = []
    for k, (name, strand) in enumerate([("gaps of 1, 2, 3 and 21", 1), ("contig N run inside an M op", -1), ("two in one codon", 1)]):
        ops, gene, asm, s, qs, qe, t = _hit(name, strand)
        recs.append(V.records_from_ops(ops, gene, asm, s, qs, qe, t, 0, kept=k))
    hand = np.zeros(5, _native.VARIANT_DTYPE)
    for i, (ref, alt, ref_aa, alt_aa) in enumerate([(0, 1, "K", "K"), (0, 3, "K", "*"), (3, 0, "*", "K"), (1, 2, "A", "G"), (4, 2, "X", "X")]):
        hand[i] = (2, 30 + i, 500 + i, 1, V.SNV, ref, alt, ord(ref_aa), ord(alt_aa), (0, 0, 0))
    records = np.concatenate([*recs, hand])
    return kept, records, np.array([0, len(records), len(records)], np.int64)


def test_formatter_against_the_python_formatter():
    kept, records, var_off = _formatter_table()
    genes, asm_names, contigs = ["wzi", "galF", "wcaJ_1"], ["asm one", "empty"], [["c1", "contig two"], ["x"]]
    want = V.format_tsv(asm_names, contigs, genes, kept, records, var_off)
    got = _native.format_variants(genes, asm_names, [c for cs in contigs for c in cs], [0, 2, 3], kept, records, var_off)
    assert got == want and got.count(b"\n") == len(records)
    effects = {line.split(b"\t")[-1] for line in got.splitlines()}
    assert effects == {b"ambiguous", b"synonymous", b"nonsense", b"stop_lost", b"missense", b"frameshift", b"inframe"}
    assert all(len(line.split(b"\t")) == 14 for line in got.splitlines()) and _native.VARIANTS_HEADER == V.HEADER
    first = got.splitlines()[0].split(b"\t")
    assert first[:2] == [b"asm one", b"contig two"] and first[4] == b"wcaJ_1" and first[3] == b"+"
    # a record that names a kept record, or a contig, the tables do not have is refused
    bad = records.copy()
    bad["kept"][0] = 3
    with pytest.raises(ValueError):
        _native.format_variants(genes, asm_names, [c for cs in contigs for c in cs], [0, 2, 3], kept, bad, var_off)
    with pytest.raises(ValueError):
        _native.format_variants(genes, asm_names, ["only one", "x"], [0, 1, 2], kept, records, var_off)
    assert _native.format_variants(genes, [], [], [0], kept[:0], records[:0], [0]) == b""


# ---- buffer policy ------------------------------------------------------------------------------------------------------------------
def test_variants_buffer_policy():
    lib = V.harness()
    first = (C.c_int32 * 2)()
    lib.kpy_var_layout(first)
    assert first[0] == 8 and first[1] == 24 == _native.VARIANT_DTYPE.itemsize  # the first guess (kp_caps.h says that it is one)
    state = (C.c_uint32 * 2)(8, 0)
    assert lib.kpy_var_size(state, C.c_uint64(1000)) == 8000 and state[1] == 8
    assert lib.kpy_var_size(state, C.c_uint64(0)) == 8  # a batch without a kept record still gets a buffer
    # records beyond the buffer grow it and ask for the records to be stored again (0), nothing else; the second time they fit
    cap = C.c_uint64(8000)
    assert lib.kpy_var_after(state, C.byref(cap), C.c_uint64(1000), C.c_uint64(20000)) == 0
    assert cap.value == 25000 and state[1] == 25
    assert lib.kpy_var_after(state, C.byref(cap), C.c_uint64(1000), C.c_uint64(20000)) == 1 and cap.value == 25000
    # ... and a batch that overflows the grown buffer as well is for the caller to refuse (KP_EOVERFLOW): the policy says 0 again
    assert lib.kpy_var_after(state, C.byref(cap), C.c_uint64(1000), C.c_uint64(40000)) == 0 and cap.value == 50000 and state[1] == 50
    assert lib.kpy_var_size(state, C.c_uint64(500)) == 25000  # later reductions start from what was learnt
    cap = C.c_uint64(25000)
    assert lib.kpy_var_after(state, C.byref(cap), C.c_uint64(500), C.c_uint64(600)) == 1 and state[1] == 50  # it never shrinks
    assert lib.kpy_var_after(state, C.byref(cap), C.c_uint64(500), C.c_uint64(24000)) == 1 and state[1] == 60  # what came close makes room
    others = (C.c_uint32 * 2)(777, 888)
    assert lib.kpy_var_set_option(state, others, b"variants_per_kept", C.c_int64(1)) == 1
    assert (state[0], state[1], others[0], others[1]) == (1, 0, 777, 888)
    assert lib.kpy_var_size(state, C.c_uint64(1000)) == 1000
    assert lib.kpy_var_set_option(state, others, b"cs_bytes_per_hit", C.c_int64(5)) == 1 and (state[0], state[1], others[0], others[1]) == (1, 1, 777, 0)
    assert lib.kpy_var_set_option(state, others, b"variants", C.c_int64(1)) == 0  # (not a buffer size: kp_ctx_set_option's own)
