"""The minimum spanning forest of locus rows without a device (include/kp_spec.h, TREE): the specification's known answers through the
restatement of tests/tree_util.py and through kaptive_amd/csrc/kp_tree.h under g++; the packed key, the predicate for a matrix that
fits it and the round bound at their edges; the header's serial Boruvka against Kruskal; the two properties that tie the forest to
CLUSTERS; ``kp_format_newick`` byte for byte against the restatement's writer, its refusals included; ``LocusRows.tree`` /
``tree_tsv`` / ``newick_tsv`` on hand-made tables with a stand-in for the device handle; the command line's flags."""

from __future__ import annotations

import ctypes as C
import pickle

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.distances import DIST_RECORD_DTYPE, LocusRows
from tests import clusters_util as CU
from tests import distances_util as D
from tests import tree_util as TU
from tests.test_distances_cpu import PLAN_1, PLAN_2, ROW_A, ROW_B, _hand_batch, _hand_db


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _known_rows():
    return np.stack([D.unpack(D.gene_blocks(D.codes_of(ROW_A))), D.unpack(D.gene_blocks(D.codes_of(ROW_B))), np.full(32, D.GAP, np.uint8)])


def _edges(*recs):
    return np.array([(a, b, c, d, u, 0) for a, b, c, d, u in recs], D.PAIR_DTYPE).reshape(len(recs))


def _tuples(edges):
    return [(int(e["a"]), int(e["b"]), int(e["compared"]), int(e["differences"]), int(e["unshared"])) for e in edges]


# ---- the specification's known answers ---------------------------------------------------------------------------------------------------
def test_known_answers_through_the_restatement_and_the_header():
    codes = _known_rows()
    blocks = D.pack(codes).reshape(3, -1)
    for how in (lambda mc: TU.forest(codes, mc), lambda mc: TU.harness_forest(blocks, mc)[:2]):
        edges, comp = how(1)
        assert _tuples(edges) == [(0, 1, 6, 6, 0)] and comp.tolist() == [0, 0, 2]
        edges, comp = how(0)  # the empty row is 0 differences from both: it carries the tree
        assert _tuples(edges) == [(0, 2, 0, 0, 8), (1, 2, 0, 0, 8)] and comp.tolist() == [0, 0, 0]
    assert TU.newick_lines("L", ["A", "B", "C"], *TU.forest(codes, 1)) == b"L\t1\t2\t(B:6)A;\nL\t2\t1\tC;\n"
    assert TU.newick_lines("L", ["A", "B", "C"], *TU.forest(codes, 0)) == b"L\t1\t3\t((B:0)C:0)A;\n"


# ---- the header, host build ------------------------------------------------------------------------------------------------------------
def test_the_mirrored_constants():
    out = np.zeros(4, np.int64)
    TU.harness().kpy_tree_layout(_p(out))
    assert out.tolist() == [TU.ROW_BITS, TU.DIFF_BITS, TU.MAX_COLUMNS, D.MAX_ROWS] and _native.TREE_MAX_COLUMNS == TU.MAX_COLUMNS
    assert TU.DIFF_BITS + 2 * TU.ROW_BITS == 64 and D.MAX_ROWS <= 1 << TU.ROW_BITS and _native.newick_header() == TU.NEWICK_HEADER


def test_packed_key_round_trip_and_order():
    h = TU.harness()
    top = ((1 << 28) - 1, (1 << 18) - 2, (1 << 18) - 1)
    for t in ((0, 0, 1), top, (5, 7, 9), (1 << 27, 1 << 17, (1 << 17) + 1)):
        assert TU.harness_unpack(h.kpy_tree_key(*t)) == t
    assert h.kpy_tree_key(0, 0, 1) == 1 and h.kpy_tree_key(*top) == (top[0] << 36) | (top[1] << 18) | top[2]
    none = h.kpy_tree_key_none()
    assert none == 2**64 - 1 and h.kpy_tree_key(*top) < none
    rng = np.random.default_rng(5)
    triples = []
    for _ in range(400):
        a = int(rng.integers(0, (1 << 18) - 1))
        triples.append((int(rng.integers(0, 1 << 28)), a, int(rng.integers(a + 1, 1 << 18))))
    for d, a, b in list(triples[:60]):  # neighbours that differ in one field by one
        triples += [(d + 1, a, b), (d, a + 1, b + 1), (d, a, b + 1)] if d + 1 < 1 << 28 and b + 1 < 1 << 18 else []
    triples += [(0, 0, 1), top, (1, 0, 1), (0, 0, 2), (0, 1, 2)]
    keys = [h.kpy_tree_key(*t) for t in triples]
    assert all(k < none for k in keys)
    order = sorted(range(len(triples)), key=lambda i: triples[i])
    assert [keys[i] for i in order] == sorted(keys)  # the key orders as the tuple
    for i in range(0, len(triples) - 1):
        assert (keys[i] < keys[i + 1]) == (triples[i] < triples[i + 1]) and (keys[i] == keys[i + 1]) == (triples[i] == triples[i + 1])


def test_fits_the_key_at_its_edge():
    h = TU.harness()
    assert h.kpy_tree_fits(((1 << 28) - 16) // 16) == 1 and h.kpy_tree_fits((1 << 28) // 16) == 0  # 16 * n_blocks = 2^28 - 16, 2^28
    assert h.kpy_tree_fits(0) == 1 and h.kpy_tree_fits(1) == 1 and h.kpy_tree_fits(1 << 27) == 0


def test_round_bound():
    h = TU.harness()
    assert [h.kpy_tree_max_rounds(n) for n in (0, 1, 2, 3, 64, 65, 1 << 18)] == [2, 2, 2, 3, 7, 8, 19]
    assert [h.kpy_tree_max_rounds(n) for n in (4, 5, 128, 129, 197)] == [3, 4, 8, 9, 9]


def test_the_union_names_the_root_it_moved():
    moved, label = TU.harness_unite(8, [(5, 6), (6, 5), (2, 6), (0, 7), (7, 5), (3, 3), (1, 4), (4, 0)])
    assert moved.tolist() == [6, -1, 5, 7, 2, -1, 4, 1] and label.tolist() == [0, 0, 0, 3, 0, 0, 0, 0]
    assert len(set(m for m in moved.tolist() if m >= 0)) == 6  # a root moves once: the slots are distinct


@pytest.mark.parametrize("R", (2, 3, 65, 197))
def test_header_boruvka_against_kruskal_and_the_two_properties(R):
    nb = 9
    codes = D.population(np.random.default_rng([R, nb]), R, nb)
    every = D.all_pairs(codes)
    blocks = D.pack(codes).reshape(R, -1)
    for mc in (0, 1, 16 * nb // 2):
        edges, comp = TU.forest_of(R, every, mc)
        got_e, got_c, rounds = TU.harness_forest(blocks, mc)
        assert got_e.tobytes() == edges.tobytes() and got_c.tobytes() == comp.tobytes(), (R, mc)
        assert len(edges) == R - len(set(comp.tolist())) and 1 <= rounds <= TU.harness().kpy_tree_max_rounds(R)
        key = list(zip(edges["differences"].tolist(), edges["a"].tolist(), edges["b"].tolist()))
        assert key == sorted(key) and (edges["a"] < edges["b"]).all()
        # PROPERTY: cutting the forest above T gives the CLUSTERS labels at T
        levels = (0, 1, 2, 5, 10, 40, 2**31 - 1)
        want = CU.labels_of(R, every, levels, mc)
        for k, t in enumerate(levels):
            assert TU.components_under(R, got_e, t).tobytes() == want[k].tobytes(), (R, mc, t)
        assert got_c.tobytes() == want[-1].tobytes()
        # PROPERTY: every row's nearest pair is an edge
        have = set(zip(got_e["a"].tolist(), got_e["b"].tolist()))
        rec = {(int(e["a"]), int(e["b"])): e for e in got_e}
        for r, n in enumerate(CU.nearest_of(R, every, mc)):
            if n["row"] >= 0:
                pair = (min(r, int(n["row"])), max(r, int(n["row"])))
                assert pair in have, (R, mc, r, n)
                assert (rec[pair]["compared"], rec[pair]["differences"], rec[pair]["unshared"]) == (n["compared"], n["differences"], n["unshared"])


# ---- kp_format_newick ------------------------------------------------------------------------------------------------------------------------
def _both(locus, names, edges, comp, rows=None):
    got = _native.format_newick(locus, names, edges, comp, rows=rows)
    shown = names if rows is None else [names[i] for i in rows]
    assert got == TU.newick_lines(locus, shown, edges, comp)
    return got


def test_newick_star_chain_and_forest():
    names = ["n0", "n1", "n2", "n3", "n4"]
    star = _edges((0, 1, 9, 3, 0), (0, 2, 9, 1, 0), (0, 3, 9, 1, 0), (0, 4, 9, 2, 0))
    assert _both("K1", names, star, np.zeros(5, np.int32)) == b"K1\t1\t5\t(n2:1,n3:1,n4:2,n1:3)n0;\n"
    chain = _edges((0, 1, 9, 1, 0), (1, 2, 9, 2, 0), (2, 3, 9, 1, 0), (3, 4, 9, 3, 0))
    assert _both("K1", names, chain, np.zeros(5, np.int32)) == b"K1\t1\t5\t((((n4:3)n3:1)n2:2)n1:1)n0;\n"
    centre = _edges((0, 2, 9, 4, 0), (1, 2, 9, 0, 0), (2, 3, 9, 4, 0), (2, 4, 9, 2, 0))  # rooted at the smallest row, not at the hub
    assert _both("K1", names, centre, np.zeros(5, np.int32)) == b"K1\t1\t5\t((n1:0,n4:2,n3:4)n2:4)n0;\n"
    forest = _edges((1, 3, 7, 2, 1))
    assert _both("K1", names, forest, np.array([0, 1, 2, 1, 4], np.int32)) == b"K1\t1\t1\tn0;\nK1\t2\t2\t(n3:2)n1;\nK1\t3\t1\tn2;\nK1\t4\t1\tn4;\n"
    assert _both("", names, forest, np.array([0, 1, 2, 1, 4], np.int32)).startswith(b"\t1\t1\tn0;\n")
    assert _both("K1", [], _edges(), np.zeros(0, np.int32)) == b""  # the empty locus
    assert _both("K1", ["only"], _edges(), np.zeros(1, np.int32)) == b"K1\t1\t1\tonly;\n"
    rows = [4, 2, 0, 1, 3]  # row i of the matrix is names[rows[i]]
    assert _both("K1", names, chain, np.zeros(5, np.int32), rows=rows) == b"K1\t1\t5\t((((n3:3)n1:1)n0:2)n2:1)n4;\n"


def test_newick_names_that_need_quotes():
    names = ["plain_A-1.fa", "two words", "it's", "Ärger", "a,b", "(x)", "semi;colon", "c:d", ""]
    edges = _edges(*((0, i, 5, i, 0) for i in range(1, len(names))))
    got = _both("L", names, edges, np.zeros(len(names), np.int32))
    assert got == ("L\t1\t9\t('two words':1,'it''s':2,'Ärger':3,'a,b':4,'(x)':5,'semi;colon':6,'c:d':7,:8)plain_A-1.fa;\n").encode()
    assert TU.newick_name("a'b''c") == b"'a''b''''c'" and TU.newick_name("ok.-_9") == b"ok.-_9"


def test_newick_of_a_long_chain_without_recursion():
    R = 200_000
    names = [f"r{i}" for i in range(R)]
    edges = np.zeros(R - 1, D.PAIR_DTYPE)
    edges["a"], edges["b"] = np.arange(R - 1), np.arange(1, R)
    edges["differences"] = np.arange(R - 1) % 7
    edges["compared"] = 100
    got = _native.format_newick("L", names, edges, np.zeros(R, np.int32))
    assert got.startswith(b"L\t1\t200000\t((((") and got.endswith(b")r2:1)r1:0)r0;\n") and got.count(b"(") == R - 1
    assert got == TU.newick_lines("L", names, edges, np.zeros(R, np.int32))


def test_newick_refusals():
    names = ["a", "b", "c", "d"]
    good, comp = _edges((0, 1, 5, 1, 0), (1, 2, 5, 2, 0)), np.array([0, 0, 0, 3], np.int32)
    assert _native.format_newick("x", names, good, comp) == b"x\t1\t3\t((c:2)b:1)a;\nx\t2\t1\td;\n"
    for bad_edges, bad_comp in (
        (_edges((0, 4, 5, 1, 0)), comp),  # an edge outside the names
        (_edges((-1, 1, 5, 1, 0)), comp),
        (_edges((1, 0, 5, 1, 0), (1, 2, 5, 2, 0)), comp),  # a >= b
        (_edges((1, 1, 5, 1, 0)), comp),
        (_edges((0, 1, 5, 1, 0), (1, 2, 5, 2, 0), (0, 2, 5, 3, 0)), comp),  # closes a cycle
        (_edges((0, 1, 5, 1, 0), (0, 1, 5, 1, 0)), np.array([0, 0, 2, 3], np.int32)),  # the same edge twice
        (_edges((0, 1, 5, 1, 0), (2, 3, 5, 2, 0)), comp),  # joins different components
        (good, np.array([0, 0, 0, 0], np.int32)),  # a component its edges do not connect
        (good, np.array([1, 1, 1, 3], np.int32)),  # a label that is not the smallest row of its tree
        (good, np.array([0, 0, 0, 2], np.int32)),
        (good, np.array([0, 0, 0, -1], np.int32)),
        (good, np.array([0, 0, 0, 4], np.int32)),
    ):
        with pytest.raises(ValueError):
            _native.format_newick("x", names, bad_edges, bad_comp)
    with pytest.raises(ValueError):
        _native.format_newick("x", names, good, comp, rows=[0, 1, 2, 4])
    with pytest.raises(ValueError):
        _native.format_newick("x", names[:3], good, comp)
    lib = _native.lib()
    lib.kp_format_newick.restype = C.c_int64
    off = np.array([0, 1, 2], np.int64)
    e, c = _edges((0, 1, 5, 3, 2)), np.array([0, 0], np.int32)
    call = lambda **kw: lib.kp_format_newick(kw.get("locus", b"x"), C.c_int32(kw.get("locus_len", 1)), b"ab", kw.get("off", _p(off)), C.c_int32(kw.get("n", 2)), None,  # noqa: E731
                                             kw.get("edges", _p(e)), C.c_int64(kw.get("n_edges", 1)), kw.get("comp", _p(c)), None, C.c_int64(kw.get("cap", 0)))
    assert call() == len(b"x\t1\t2\t(b:3)a;\n")  # the sizing call
    for kw in (dict(cap=8), dict(cap=-1), dict(off=None), dict(comp=None), dict(edges=None), dict(n=-1), dict(n_edges=-1), dict(locus_len=-1), dict(locus=None)):
        assert call(**kw) == -1, kw


# ---- LocusRows on hand-made tables ---------------------------------------------------------------------------------------------------------
class _RestatedHandle:
    """Stands in for ``_native.Distances``: the restatement instead of the device."""

    made = 0

    def __init__(self, ctx, rows_matrix):
        type(self).made += 1
        self.ctx, self._h, self.codes = ctx, True, D.unpack(np.asarray(rows_matrix, np.uint64))

    def tree(self, min_compared=D.MIN_COMPARED):
        return TU.forest(self.codes, min_compared)

    def pairs(self, max_diff=None, min_compared=0):
        return D.all_pairs(self.codes, max_diff, min_compared)

    def close(self):
        self._h = None


def _two_batches(db):
    return _hand_batch(db, 1, ["a0", "a1", "a2", "a3"], PLAN_1, [0, 0, 1, 1]), _hand_batch(db, 2, ["b0", "b1", "b2"], PLAN_2, [0, 1, 0])


def _records(rec):
    return [tuple(int(r[f]) for f in ("locus", "a", "b", "compared", "differences", "unshared")) for r in rec]


def test_locus_rows_tree_from_hand_made_tables(monkeypatch):
    monkeypatch.setattr(_native, "Distances", _RestatedHandle)
    db = _hand_db()
    lr = LocusRows(db)
    for b in _two_batches(db):
        lr.add(b)  # L0: assemblies 0, 1, 4, 6; L1: 2, 3, 5
    ctx = object()
    for mc in (1, 0, 3):
        rec = lr.tree(ctx, mc)
        assert rec.dtype == DIST_RECORD_DTYPE and _records(rec) == TU.run_edges(lr, mc)
        assert all({a, b} <= ({0, 1, 4, 6} if L == 0 else {2, 3, 5}) and a < b for L, a, b, *_ in _records(rec))  # assembly numbers, not rows
        assert lr.tree_tsv(ctx, mc) == TU.run_tree_tsv(lr, mc) and lr.newick_tsv(ctx, mc) == TU.run_newick_tsv(lr, mc)
    rec = lr.tree(ctx, 0)
    assert rec["locus"].tolist() == [0, 0, 0, 1, 1] and lr.tree_tsv(ctx, 0).count(b"\n") == 5  # with min_compared 0 every locus is one tree
    assert lr.newick_tsv(ctx, 0).count(b"\n") == 2 and lr.newick_tsv(ctx, 0).startswith(b"L0\t1\t4\t(") and b"\nL1\t1\t3\t(" in lr.newick_tsv(ctx, 0)
    made = _RestatedHandle.made
    assert lr.tsv(ctx, None, 0).count(b"\n") == 6 + 3 and _RestatedHandle.made == made  # one handle per locus serves every table
    lr.close()
    lr.tree(ctx)
    assert _RestatedHandle.made == made + 2


def test_two_loci_one_of_them_with_a_single_row(monkeypatch):
    monkeypatch.setattr(_native, "Distances", _RestatedHandle)
    db = _hand_db()
    lr = LocusRows(db)
    lr.add(_hand_batch(db, 1, ["a0", "a1", "a2"], PLAN_1[:3], [0, 0, 1]))
    made = _RestatedHandle.made
    rec = lr.tree(object(), 0)
    assert _RestatedHandle.made == made + 1  # the single row needs no handle
    assert _records(rec) == TU.run_edges(lr, 0) and rec["locus"].tolist() == [0] and (rec["a"][0], rec["b"][0]) == (0, 1)
    lines = lr.newick_tsv(object(), 0).splitlines()
    assert lines[1] == b"L1\t1\t1\ta2;" and lines[0].startswith(b"L0\t1\t2\t(a1:") and lines[0].endswith(b")a0;") and len(lines) == 2
    assert lr.newick_tsv(object(), 0) == TU.run_newick_tsv(lr, 0) and lr.tree_tsv(object(), 0) == TU.run_tree_tsv(lr, 0)


def test_tree_after_a_state_and_merge_round_trip(monkeypatch):
    monkeypatch.setattr(_native, "Distances", _RestatedHandle)
    db = _hand_db()
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
    assert merged.tree(ctx, 0).tobytes() == whole.tree(ctx, 0).tobytes() and merged.tree_tsv(ctx, 0) == whole.tree_tsv(ctx, 0) == TU.run_tree_tsv(whole, 0)
    assert merged.newick_tsv(ctx, 0) == whole.newick_tsv(ctx, 0) == TU.run_newick_tsv(whole, 0)
    made = _RestatedHandle.made
    merged.merge(whole.state())  # the rows change: the handles go, the next table is made of all fourteen rows
    assert sum(int(f) for f in (line.split(b"\t")[2] for line in merged.newick_tsv(ctx, 0).splitlines())) == 14 and _RestatedHandle.made == made + 2


# ---- the command line's flags ---------------------------------------------------------------------------------------------------------------
def test_command_line_flags():
    from kaptive_amd.cli import build_parser

    ap = build_parser()
    base = ["assembly", "db.npz", "a.fasta"]
    ns = ap.parse_args([*base, "--mst", "m.tsv"])
    assert ns.mst == "m.tsv" and not any(hasattr(ns, f) for f in ("newick", "clusters", "min_compared", "distances", "aligned", "cluster_levels"))
    ns = ap.parse_args([*base, "--mst", "m.tsv", "--min-compared", "100"])  # --min-compared beside --mst alone
    assert ns.min_compared == 100 and not hasattr(ns, "newick")
    ns = ap.parse_args([*base, "--newick", "n.tsv", "--min-compared", "7"])  # ... and beside --newick alone
    assert (ns.newick, ns.min_compared) == ("n.tsv", 7) and not hasattr(ns, "mst")
    ns = ap.parse_args([*base, "--mst", "m.tsv", "--newick", "n.tsv", "--clusters", "c.tsv", "--distances", "d.tsv", "--cluster-levels", "0,3"])
    assert (ns.mst, ns.newick, ns.clusters, ns.distances, ns.cluster_levels) == ("m.tsv", "n.tsv", "c.tsv", "d.tsv", (0, 3))
    for bad in (["--mst", "m.tsv", "--cluster-levels", "0,1"], ["--newick", "n.tsv", "--cluster-levels", "0,1"], ["--mst", "m.tsv", "--max-distance", "3"],
                ["--min-compared", "3"], ["--mst", "m.tsv", "--min-compared", "-1"], ["--newick", "n.tsv", "--min-compared", str(2**31)]):  # fmt: skip
        with pytest.raises(SystemExit):
            ap.parse_args([*base, *bad])
