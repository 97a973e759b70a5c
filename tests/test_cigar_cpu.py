"""CIGARs, the parts that need no GPU (include/kp_spec.h, CIGAR): the yardstick the device's ops are compared with -- the
banded recurrence restated in tests/native_harness/cigar_harness.cpp -- checked on hand-built pairs with a unique optimum and
tied to the pinned oracle on the band tasks of the small batch; the buffer policy of the ops (kp_caps.h); kp_format_paf
against a Python formatter; the Cigars column; the command line's --paf option."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.core.alignment import Alignments, Cigars
from tests import cigar_util as U

M, I, D = U.M, U.I, U.D


def ops_of(*pairs) -> list:
    return [(n << 4) | k for k, n in pairs]


def _random_codes(rng, n):
    return rng.integers(0, 4, size=n).astype(np.uint8)


def _other(*codes):
    """A base that differs from all of `codes`."""
    return next(c for c in range(4) if c not in codes)


def _pair(gene, target, lo, width, left=40):
    """Yardstick on `target` planted `left` bases into a contig of random flanks: (out7, ops, contig start of the target)."""
    rng = np.random.default_rng(99)
    asm = np.concatenate([_random_codes(rng, left), target, _random_codes(rng, 40)]).astype(np.uint8)
    out7, ops = U.yardstick(gene, asm, lo + left, width, 0, len(asm))
    return out7, ops.tolist(), left


@pytest.fixture(scope="module")
def gene():
    return _random_codes(np.random.default_rng(7), 240)


def test_yardstick_perfect_copy(gene):
    out7, ops, left = _pair(gene, gene, -8, 16)
    assert ops == ops_of((M, 240))
    assert out7.tolist() == [480, 0, 240, left, left + 240, 240, 240]


def test_yardstick_substitutions_only(gene):
    t = gene.copy()
    for at in (50, 120, 200):
        t[at] = (t[at] + 1) % 4
    out7, ops, left = _pair(gene, t, -8, 16)
    assert ops == ops_of((M, 240))
    assert out7.tolist() == [480 - 3 * 6, 0, 240, left, left + 240, 237, 240]


def test_yardstick_one_base_insertion_and_deletion(gene):
    # an extra base in the target that differs from both neighbours: the gap has one place to go (a D op)
    at = 100
    t = np.concatenate([gene[:at], [_other(gene[at - 1], gene[at])], gene[at:]]).astype(np.uint8)
    out7, ops, left = _pair(gene, t, -8, 16)
    assert ops == ops_of((M, 100), (D, 1), (M, 140))
    assert out7.tolist() == [480 - 6, 0, 240, left, left + 241, 240, 241]
    # a base of the gene missing from the target, different from both of its neighbours (an I op)
    at = next(i for i in range(100, 200) if gene[i] != gene[i - 1] and gene[i] != gene[i + 1])
    t = np.delete(gene, at)
    out7, ops, left = _pair(gene, t, -8, 16)
    assert ops == ops_of((M, at), (I, 1), (M, 239 - at))
    assert out7.tolist() == [478 - 6, 0, 240, left, left + 239, 239, 240]


@pytest.mark.parametrize("size,credit", [(20, 0), (21, 1)])
def test_yardstick_long_gap_credit(size, credit):
    """KP_GAP_LONG: a gap of 20 columns costs 4 + 2 * 20 either way; one of 21 is credited 1 (24 + 21 against 4 + 42)."""
    rng = np.random.default_rng(11)
    g = _random_codes(rng, 600)
    ins = _random_codes(rng, size)
    ins[0], ins[-1] = _other(g[299], g[300]), _other(g[299], g[300], ins[0] if size > 1 else 9)
    t = np.concatenate([g[:300], ins, g[300:]]).astype(np.uint8)
    out7, ops, left = _pair(g, t, -40, 64)
    assert [o & 15 for o in ops] == [M, D, M] and ops[1] >> 4 == size
    assert sum(o >> 4 for o in ops if o & 15 == M) == 600
    assert out7[0] == 1200 - (4 + 2 * size) + credit == 1200 - int(U.gap_cost(size))
    assert out7[6] == 600 + size and out7[5] == 600


def test_yardstick_reverse_strand(gene):
    """The gene's reverse complement is what is aligned: ops run along the target, the hit's query span is flipped back."""
    rc = np.ascontiguousarray((3 - gene)[::-1])
    at = 60  # a deletion from the target, 60 bases into the reverse complement
    while not (rc[at] != rc[at - 1] and rc[at] != rc[at + 1]):
        at += 1
    t = np.delete(rc, at)[10:]  # ... whose first ten bases are missing as well
    codes, off = gene, np.array([0, 240], np.int32)
    assert np.array_equal(U.gene_as_aligned(codes, off, 1), rc)
    out7, ops, left = _pair(rc, t, -24, 32)
    assert ops == ops_of((M, at - 10), (I, 1), (M, 239 - at))
    assert out7.tolist()[:5] == [2 * 229 - 6, 10, 240, left, left + 229]
    assert U.result_to_hit_fields(out7, 1, 240, 0) == (0, 230, left, left + 229, -1)


# ---- the yardstick against the pinned oracle on the band tasks of the small batch ---------------------------------------------
@pytest.fixture(scope="module")
def small():
    db = U.small_db()
    return db, U.small_batch(db), U.db_codes(db)


def test_yardstick_equals_oracle_on_the_small_batch(small, oracle):
    """Every band task of batch (a): the yardstick's score, spans, matches and block_len are the oracle's (kpo_sw), and
    every hit of kpo_align that no join produced is one of those results turned into a hit record."""
    db, genomes, (codes, off) = small
    odb = oracle.OracleDB(codes, off)
    n_tasks = n_checked = 0
    kinds = set()
    for g in genomes:
        pa = g.packed()
        asm = U.assembly_codes(pa)
        tasks = odb.tasks(pa)
        want = odb.sw(pa, tasks)
        records = set()
        for task, w in zip(tasks, want):
            got, ops = U.task_yardstick(codes, off, pa, asm, task)
            n_tasks += 1
            if w[0] < U.MIN_DP_SCORE:
                assert got[0] == w[0], f"{g.id}: task {task}: score {got[0]} vs {w[0]}"
                continue
            # kpo_sw reports the best cell's score; the yardstick (like a hit) the path's score under the two-piece gap cost:
            # every gap op longer than KP_GAP_LONG = 20 columns is credited what exceeds 20
            credit = sum(max((int(o) >> 4) - 20, 0) for o in ops if int(o) & 15 != M)
            assert [int(got[0]) - credit, *got[1:].tolist()] == w.tolist(), f"{g.id}: task {task}: {got.tolist()} (credit {credit}) vs the oracle's {w.tolist()}"
            kinds.update((int(o) & 15, min(int(o) >> 4, 32)) for o in ops)
            gs = int(task["gs"])
            qlen = int(off[(gs >> 1) + 1] - off[gs >> 1])
            records.add((gs >> 1, int(task["contig"]), *U.result_to_hit_fields(got, gs, qlen, int(pa.ctg_start[task["contig"]])),
                         int(got[0]), int(got[5]), int(got[6])))  # fmt: skip
            n_checked += 1
        joins = odb.joins(pa)
        n_joined = int((joins["piece"][:, :, 0] == 1).sum()) if len(joins) else 0
        hits = odb.align(pa)
        unmatched = [h for h in hits if (int(h["gene"]), int(h["contig"]), int(h["q_start"]), int(h["q_end"]), int(h["t_start"]), int(h["t_end"]),
                                         int(h["strand"]), int(h["score"]), int(h["matches"]), int(h["block_len"])) not in records]  # fmt: skip
        assert len(unmatched) <= n_joined, f"{g.id}: {len(unmatched)} hits are no band task's result, {n_joined} joined hits"
    assert n_checked >= 60
    # the batch reaches what it was built for: 1-base gaps of both kinds, gaps of 20, 21 and 31 columns
    for want_kind in [(I, 1), (D, 1), (D, 20), (I, 21), (D, 21), (I, 31), (D, 31)]:
        assert want_kind in kinds, f"no band task of the small batch has an op {want_kind}"


# ---- buffer policy ----------------------------------------------------------------------------------------------------------
def test_cigar_buffer_policy():
    lib = U.harness()
    layout = (C.c_int32 * 3)()
    lib.kpy_layout(layout)
    assert layout[2] == 4  # the first guess (kp_caps.h says why)
    state = (C.c_uint32 * 3)(4, 0, 0)
    assert lib.kpy_cigar_size(state, C.c_uint64(1000)) == 4000 and state[1] == 4
    assert lib.kpy_cigar_size(state, C.c_uint64(0)) == 4  # an empty table still gets a buffer
    # a pass whose ops exceed the buffer grows it and asks for the ops to be written again (0), nothing else
    cap = C.c_uint64(4000)
    assert lib.kpy_cigar_after(state, C.byref(cap), C.c_uint64(1000), C.c_uint64(9000)) == 0
    assert cap.value == 9000 + 9000 // 4 and state[1] == 12  # ceil(11250 / 1000)
    assert lib.kpy_cigar_after(state, C.byref(cap), C.c_uint64(1000), C.c_uint64(9000)) == 1 and cap.value == 11250
    assert lib.kpy_cigar_size(state, C.c_uint64(500)) == 6000  # later passes start from what was learnt
    # the learnt size never shrinks
    cap = C.c_uint64(6000)
    assert lib.kpy_cigar_after(state, C.byref(cap), C.c_uint64(500), C.c_uint64(600)) == 1 and state[1] == 12 and cap.value == 6000
    # a pass that came close makes room for the next one
    cap = C.c_uint64(6000)
    assert lib.kpy_cigar_after(state, C.byref(cap), C.c_uint64(500), C.c_uint64(5900)) == 1 and state[1] == 15  # ceil(7375 / 500)
    # setting the option resets what was learnt, and only that
    other = C.c_uint32(777)
    assert lib.kpy_set_option(state, C.byref(other), b"cigar_ops_per_hit", C.c_int64(2)) == 1
    assert (state[0], state[1], other.value) == (2, 0, 777)
    assert lib.kpy_cigar_size(state, C.c_uint64(1000)) == 2000
    assert lib.kpy_set_option(state, C.byref(other), b"hit_cap", C.c_int64(5)) == 1 and (state[0], state[1], other.value) == (2, 2, 0)
    assert lib.kpy_set_option(state, C.byref(other), b"cigar", C.c_int64(1)) == 0  # (not a buffer size: kp_ctx_set_option's own)


# ---- kp_format_paf ------------------------------------------------------------------------------------------------------------
def _paf_python(gene_names, gene_len, ctg_names, ctg_len, first, hits, hit_off, ops, coff) -> bytes:
    out = []
    for a in range(len(hit_off) - 1):
        for i in range(hit_off[a], hit_off[a + 1]):
            h = hits[i]
            c = first[a] + int(h["contig"])
            cg = "".join(f"{int(o) >> 4}{'MID'[int(o) & 15]}" for o in ops[coff[i] : coff[i + 1]])
            out.append("\t".join(map(str, [gene_names[h["gene"]], gene_len[h["gene"]], h["q_start"], h["q_end"], "-" if h["strand"] < 0 else "+",
                                           ctg_names[c], ctg_len[c], h["t_start"], h["t_end"], h["matches"], h["block_len"], h["mapq"],
                                           f"AS:i:{h['score']}", f"NM:i:{h['block_len'] - h['matches']}", f"cg:Z:{cg}"])) + "\n")  # fmt: skip
    return "".join(out).encode()


def _paf_table():
    gene_names = ["g" * 300, "wzi", "KL1_01_galF"]  # (names are blobs with offsets: any length)
    gene_len = [65535, 1200, 900]
    ctg_names = ["contig_1", "c" * 500, "NODE_3_length_1073676288"]
    ctg_len = [5000, 70000, (1 << 30) - 65536]
    first = [0, 1, 3]
    hits = np.zeros(4, _native.HIT_DTYPE)
    rows = [  # gene, contig, q_start, q_end, t_start, t_end, score, matches, block_len, strand, mapq
        (1, 0, 0, 1200, 100, 1301, 2380, 1199, 1202, 1, 60),
        (0, 0, 10, 65535, 17, 65000, 120000, 64000, 66000, -1, 0),
        (2, 1, 5, 900, 1073000000, 1073000897, 1700, 890, 897, -1, 255),
        (1, 0, 100, 400, 0, 300, 600, 300, 300, 1, 3),
    ]
    for h, r in zip(hits, rows):
        for name, v in zip(("gene", "contig", "q_start", "q_end", "t_start", "t_end", "score", "matches", "block_len", "strand", "mapq"), r):
            h[name] = v
    hit_off = [0, 1, 4]
    cig = [ops_of((M, 600), (I, 1), (M, 300), (D, 2), (M, 299)), ops_of((M, 1234), (D, 1500), (M, 64000)), ops_of((M, 895)), ops_of((M, 300))]
    ops = np.array([o for c in cig for o in c], np.uint32)
    coff = np.concatenate([[0], np.cumsum([len(c) for c in cig])]).astype(np.int64)
    return gene_names, gene_len, ctg_names, ctg_len, first, hits, hit_off, ops, coff


def test_format_paf_matches_python_formatter():
    table = _paf_table()
    want = _paf_python(*table)
    assert _native.format_paf(*table) == want
    assert want.count(b"\n") == 4 and b"\t-\t" in want and b"\t+\t" in want and b"1I" in want and b"2D" in want and b"1500D" in want


def test_format_paf_reports_the_size_it_needs():
    gene_names, gene_len, ctg_names, ctg_len, first, hits, hit_off, ops, coff = _paf_table()
    want = _paf_python(gene_names, gene_len, ctg_names, ctg_len, first, hits, hit_off, ops, coff)
    gn, go = _native._blob(gene_names)
    cn, co = _native._blob64(ctg_names)
    keep = [np.asarray(gene_len, np.int32), np.asarray(ctg_len, np.int32), np.asarray(first, np.int64), np.asarray(hit_off, np.int64)]
    t = _native.PafTables(gene_names=gn.ctypes.data, gene_name_off=go.ctypes.data, gene_len=keep[0].ctypes.data, n_genes=3,
                          ctg_names=cn.ctypes.data, ctg_name_off=co.ctypes.data, ctg_len=keep[1].ctypes.data, asm_first_ctg=keep[2].ctypes.data)  # fmt: skip
    f = _native.lib().kp_format_paf
    f.restype = C.c_int64
    args = (C.byref(t), C.c_int32(2), hits.ctypes.data_as(C.c_void_p), keep[3].ctypes.data_as(C.c_void_p), ops.ctypes.data_as(C.c_void_p),
            coff.ctypes.data_as(C.c_void_p))  # fmt: skip
    small = np.full(100, 0x7E, np.uint8)
    assert f(*args, small.ctypes.data_as(C.c_void_p), C.c_int64(50)) == len(want)  # too small: the size, as kp_format_rows
    assert (small[50:] == 0x7E).all()  # nothing written past the cap
    assert f(*args, None, C.c_int64(0)) == len(want)
    hits["gene"][0] = 3  # a gene the tables do not have
    assert f(*args, None, C.c_int64(0)) == -1


# ---- the Cigars column ----------------------------------------------------------------------------------------------------------
def _alignments(n, first_gene=0):
    return Alignments.from_hit_table(
        ("a", "b", "c"), ("c0", "c1"), q_ids=(np.arange(n) + first_gene) % 3, q_lengths=np.full(n, 500), q_starts=np.zeros(n), q_ends=np.full(n, 100),
        t_ids=np.arange(n) % 2, t_lengths=np.full(n, 900), t_starts=np.arange(n), t_ends=np.arange(n) + 100, strands=np.where(np.arange(n) % 2, -1, 1),
        block_lens=np.full(n, 100), matches=np.full(n, 99), scores=np.full(n, 190), mapqs=np.full(n, 60),
    )  # fmt: skip


def test_cigars_slicing_mask_and_concat():
    per_hit = [ops_of((M, 100)), ops_of((M, 40), (I, 2), (M, 58)), ops_of((M, 10), (D, 3), (M, 87)), ops_of((M, 100)), ops_of((M, 1), (I, 98), (M, 1))]
    ops = np.array([o for c in per_hit for o in c], np.uint32)
    off = np.concatenate([[0], np.cumsum([len(c) for c in per_hit])]).astype(np.int64)
    hit_off = [0, 2, 2, 5]  # three assemblies, the second without hits
    parts = [Cigars.from_offsets(ops, off[hit_off[a] : hit_off[a + 1] + 1]) for a in range(3)]
    assert [len(p) for p in parts] == [2, 0, 3]
    assert all(p.data is ops or np.shares_memory(p.data, ops) for p in parts)  # per-assembly views, no copy
    assert [parts[0][i].tolist() for i in range(2)] == per_hit[:2] and [parts[2][i].tolist() for i in range(3)] == per_hit[2:]
    assert parts[2].to_strings() == ["10M3D87M", "100M", "1M98I1M"]
    import dataclasses

    tables = [dataclasses.replace(_alignments(len(p), a), cigars=p) for a, p in enumerate(parts)]
    masked = tables[2][np.array([True, False, True])]
    assert [masked.cigars[i].tolist() for i in range(2)] == [per_hit[2], per_hit[4]] and masked[1].cigar.tolist() == per_hit[4]
    assert tables[2][1:].cigars.to_strings() == ["100M", "1M98I1M"]
    joined = Alignments.concat([tables[0], tables[2], _alignments(2)])
    assert [joined.cigars[i].tolist() for i in range(7)] == [*per_hit, [], []]
    paf = tables[2].to_paf(("geneA", "geneB", "geneC")).decode().splitlines()
    assert [line.split("\t")[-1] for line in paf] == ["cg:Z:10M3D87M", "cg:Z:100M", "cg:Z:1M98I1M"]
    assert paf[0].split("\t")[:9] == ["geneC", "500", "0", "100", "+", "c0", "900", "0", "100"]
    assert _alignments(2).to_paf().decode().splitlines()[1].split("\t")[-1] == "cg:Z:"  # a table without CIGARs


# ---- command line ---------------------------------------------------------------------------------------------------------------
def test_paf_option_and_per_database_name():
    from kaptive_amd.cli import build_parser, per_database_path

    args = build_parser().parse_args(["assembly", "db.npz", "a.fasta", "b.fasta", "-o", "out.tsv", "--paf", "hits.paf"])
    assert args.paf == "hits.paf" and args.out == "out.tsv"
    assert not hasattr(build_parser().parse_args(["assembly", "db.npz", "a.fasta"]), "paf")  # off unless asked for
    args = build_parser().parse_args(["assembly", "db.npz", "a.fasta", "--db", "o.npz", "--paf", "hits.paf"])
    assert args.db == ["o.npz"] and per_database_path(args.paf, "kpsc_k") == "hits.kpsc_k.paf"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["convert", "db.npz", "x.jsonl", "--paf", "hits.paf"])
