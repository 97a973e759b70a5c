"""Clusters and nearest neighbours of locus rows, the parts that need no GPU (include/kp_spec.h, CLUSTERS): the specification's known
answers through the restatement of tests/clusters_util.py and through kp_clust.h built with g++ (tests/native_harness/
clust_harness.cpp); the header's host build -- the first level of a pair at every edge, the nearest key's order, find / unite in
three orders with parent[x] <= x after every call, the cluster numbers --; kp_format_clusters byte for byte; ``LocusRows.clusters`` on
hand-made tables with the device call replaced by the restatement; ``state()`` / ``merge()``; the mirrors of the header's constants;
the command line's flags."""

from __future__ import annotations

import ctypes as C
import pickle
import re
from pathlib import Path

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.distances import LocusRows, clust_record_dtype
from tests import clusters_util as CU
from tests import distances_util as D
from tests.test_distances_cpu import PLAN_1, PLAN_2, ROW_A, ROW_B, _hand_batch, _hand_db

ROOT = Path(__file__).resolve().parent.parent


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _known_rows():
    return np.stack([D.unpack(D.gene_blocks(D.codes_of(ROW_A))), D.unpack(D.gene_blocks(D.codes_of(ROW_B))), np.full(32, D.GAP, np.uint8)])


# ---- the specification's known answers ---------------------------------------------------------------------------------------------------
def test_known_answers_through_the_restatement_and_the_header():
    codes = _known_rows()
    blocks = D.pack(codes).reshape(3, -1)
    for how in (lambda mc: CU.clusters(codes, (0, 6), mc), lambda mc: CU.harness_clusters(blocks, (0, 6), mc)):
        labels, near = how(1)
        assert labels.tolist() == [[0, 1, 2], [0, 0, 2]]
        assert near.tolist() == [(1, 6, 6, 0), (0, 6, 6, 0), (-1, 0, 0, 0)]
        labels, near = how(0)  # the empty row is 0 differences from everything: it links A to B
        assert labels.tolist() == [[0, 0, 0], [0, 0, 0]]
        assert near.tolist() == [(2, 0, 0, 8), (2, 0, 0, 8), (0, 0, 0, 8)]
    labels, near = CU.clusters(codes, (), 1)  # no level: nearest alone
    assert labels.shape == (0, 3) and near["row"].tolist() == [1, 0, -1]


# ---- the header, host build ------------------------------------------------------------------------------------------------------------
def test_first_level_of_a_pair_at_every_edge():
    top = 2**31 - 1
    for levels in ((0, 1, 2, 5, 10), (0,), (6,), CU.EIGHT, (0, 1, 2, 3, 4, 5, 6, top)):
        K = len(levels)
        for k, t in enumerate(levels):
            assert CU.harness_first_level(levels, t) == k
            if t < top:
                assert CU.harness_first_level(levels, t + 1) == k + 1  # (levels ascend strictly: t + 1 <= the next level)
            if t > 0:
                assert CU.harness_first_level(levels, t - 1) == (k if k == 0 or levels[k - 1] < t - 1 else k - 1)
        assert CU.harness_first_level(levels, 0) == (0 if levels[0] >= 0 else 1)
        assert CU.harness_first_level(levels, top) == (K if levels[-1] < top else K - 1)  # above every level
    for diff in (0, 1, top):
        assert CU.harness_first_level((), diff) == 0  # K = 0: every pair is beyond the levels
    h = CU.harness()
    lv = lambda *t: (_p(np.array(t, np.int32)), C.c_int32(len(t)))  # noqa: E731
    assert h.kpy_clust_levels_valid(*lv(0, 1, 2, 5, 10)) and h.kpy_clust_levels_valid(None, C.c_int32(0)) and h.kpy_clust_levels_valid(*lv(*range(8)))
    for bad in ((0, 0), (1, 0), (-1, 2), tuple(range(9))):
        assert not h.kpy_clust_levels_valid(*lv(*bad)), bad
    assert not h.kpy_clust_levels_valid(None, C.c_int32(2)) and not h.kpy_clust_levels_valid(*lv(0)[:1], C.c_int32(-1))


def test_nearest_key_orders_by_differences_then_row():
    h = CU.harness()
    none = int(h.kpy_clust_key_none())
    assert none == 2**64 - 1
    keys = [(d, s) for d in (0, 1, 2, 2**31 - 1) for s in (0, 1, 77, D.MAX_ROWS - 1)]
    packed = [int(h.kpy_clust_key(d, s)) for d, s in keys]
    assert packed == sorted(packed) and len(set(packed)) == len(packed)  # the order of (differences, row)
    assert all(p == (d << 32 | s) and p < none for p, (d, s) in zip(packed, keys))  # "none" loses to everything
    assert all((h.kpy_clust_key_differences(p), h.kpy_clust_key_row(p)) == k for p, k in zip(packed, keys))
    assert h.kpy_clust_key_row(none) == -1 and h.kpy_clust_key_differences(none) == 0


def _flood(R, edges, levels):
    out = np.zeros((len(levels), R), np.int32)
    for k, t in enumerate(levels):
        lab = list(range(R))
        moved = True
        while moved:
            moved = False
            for a, b, d in edges:
                if d <= t and lab[a] != lab[b]:
                    lab[a] = lab[b] = min(lab[a], lab[b])
                    moved = True
        out[k] = lab
    return out


def test_find_and_unite_in_every_order_keep_the_invariant():
    rng = np.random.default_rng(5)
    levels = (0, 2, 3, 6)
    for R, n in ((1, 0), (2, 1), (7, 5), (40, 30), (90, 200), (300, 260)):
        e = np.stack([rng.integers(0, R, n), rng.integers(0, R, n), rng.integers(0, 9, n)], axis=1).astype(np.int32) if n else np.zeros((0, 3), np.int32)
        e = e[e[:, 0] != e[:, 1]]
        e[:, :2] = np.sort(e[:, :2], axis=1)
        want = _flood(R, e.tolist(), levels)
        for order in (e, e[::-1], e[rng.permutation(len(e))]):  # forward, reversed, random: the harness checks parent[x] <= x after every call
            got = CU.harness_labels(R, order, levels)
            assert got.tolist() == want.tolist(), (R, n)
        assert (np.diff(want, axis=0) <= 0).all()  # levels nest: a label can only fall
    chain = np.array([(x - 1, x, 1) for x in range(299, 0, -1)], np.int32)  # hooked from its far end: the deepest tree
    got = CU.harness_labels(300, chain, (0, 1))
    assert got[0].tolist() == list(range(300)) and not got[1].any()
    num = np.zeros(6, np.int32)
    h = CU.harness()
    assert h.kpy_clust_numbers(_p(np.array([0, 0, 2, 0, 4, 2], np.int32)), C.c_int32(6), _p(num)) == 1 and num.tolist() == [1, 1, 2, 1, 3, 2]
    for bad in ([0, 2, 2], [0, 1, 1, 2], [-1, 1], [1, 1]):  # above its row, not a root, negative, above its row
        assert h.kpy_clust_numbers(_p(np.array(bad, np.int32)), C.c_int32(len(bad)), _p(num)) == 0, bad


def test_header_on_random_matrices_against_the_restatement():
    rng = np.random.default_rng(6)
    for R, nb in ((2, 1), (9, 3), (40, 5)):
        codes = D.population(rng, R, nb)
        m = D.pack(codes).reshape(R, -1)
        for levels, mc in (((0, 1, 2, 5, 10), 1), (CU.EIGHT, 0), ((6,), 16 * nb // 2), ((), 1)):
            want_l, want_n = CU.clusters(codes, levels, mc)
            got_l, got_n = CU.harness_clusters(m, levels, mc)
            assert got_l.tobytes() == want_l.tobytes() and got_n.tobytes() == want_n.tobytes(), (R, nb, levels, mc)


# ---- the mirrors ---------------------------------------------------------------------------------------------------------------------------
def test_header_constants_and_their_mirrors():
    out = np.zeros(4, np.int32)
    CU.harness().kpy_clust_layout(_p(out))
    assert out.tolist()[:3] == [16, CU.MAX_LEVELS, 4 * (CU.MAX_LEVELS + 1)]
    assert (_native.CLUST_MAX_LEVELS, _native.CLUSTER_LEVELS) == (CU.MAX_LEVELS, CU.LEVELS)
    spec = (ROOT / "include" / "kp_spec.h").read_text()
    assert re.search(r"#define KP_CLUST_MAX_LEVELS 8\b", spec) and "CLUSTERS" in spec
    body = re.search(r"typedef struct kp_dist_nearest \{(.*?)\} kp_dist_nearest;", spec, re.S)[1]
    fields = [f.strip() for decl in re.findall(r"int32_t ([^;]+);", body) for f in decl.split(",")]
    assert fields == list(_native.DIST_NEAREST_DTYPE.names) and _native.DIST_NEAREST_DTYPE == CU.NEAREST_DTYPE and _native.DIST_NEAREST_DTYPE.itemsize == 16
    assert _native.clusters_header(CU.LEVELS) == CU.header(CU.LEVELS) == b"Locus\tAssembly\tHC0\tHC1\tHC2\tHC5\tHC10\tNearest\tDifferences\tCompared\tUnshared\n"
    assert _native.clusters_header(()) == CU.header(()) == b"Locus\tAssembly\tNearest\tDifferences\tCompared\tUnshared\n"
    for bad in ((1, 1), (2, 1), (-1,), tuple(range(9))):
        with pytest.raises(ValueError):
            _native.check_cluster_levels(bad)
    assert len(_native.REPORTS) == 5 and "clusters" not in [r.name for r in _native.REPORTS]  # a layer beside the per-batch reports


# ---- the formatter ---------------------------------------------------------------------------------------------------------------------------
def _near(*recs):
    return np.array(list(recs), CU.NEAREST_DTYPE)


def test_format_clusters_byte_for_byte():
    names = ["iso_1", "", "a name with spaces", "é"]
    near = _near((1, 25000, 0, 0), (0, 25000, 0, 0), (3, 2**31 - 1, 2**31 - 1, 2**31 - 1), (-1, 0, 0, 0))  # the last row has no neighbour
    one = np.array([[0, 0, 2, 3]], np.int32)
    eight = np.array([[0, 1, 2, 3]] * 3 + [[0, 0, 2, 3]] * 2 + [[0, 0, 2, 2]] * 2 + [[0, 0, 0, 0]], np.int32)
    for labels in (np.zeros((0, 4), np.int32), one, eight):  # K = 0, 1, 8
        got = _native.format_clusters("KL107", names, labels, near)
        assert got == CU.format_lines("KL107", names, labels, near) and got.count(b"\n") == 4
    assert _native.format_clusters("KL107", names, one, near).splitlines()[3] == "KL107\té\t3\t.\t.\t.\t.".encode()
    assert _native.format_clusters("KL107", names, one, near).splitlines()[0] == b"KL107\tiso_1\t1\t\t0\t25000\t0"  # (its neighbour's name is empty)
    assert _native.format_clusters("", [], np.zeros((2, 0), np.int32), near[:0]) == b""
    # rows: row i of the matrix is named names[rows[i]]
    assert _native.format_clusters("x", names, one, near, rows=[1, 0, 2, 3]).splitlines()[0] == b"x\t\t1\tiso_1\t0\t25000\t0"
    R = 5000  # more lines than the first buffer holds: the size-then-fill convention
    many_names = [f"assembly_{i:05d}_with_a_long_name_{'x' * 80}" for i in range(R)]
    labels = np.stack([np.arange(R, dtype=np.int32), (np.arange(R, dtype=np.int32) // 7) * 7, np.zeros(R, np.int32)])
    near = np.zeros(R, CU.NEAREST_DTYPE)
    near["row"], near["differences"], near["compared"] = np.arange(R)[::-1], np.arange(R), 25000
    assert _native.format_clusters("L" * 300, many_names, labels, near) == CU.format_lines("L" * 300, many_names, labels, near)
    # every refusal
    near = _near((1, 1, 1, 1), (0, 1, 1, 1), (0, 1, 1, 1), (0, 1, 1, 1))
    for bad in ([[0, 2, 2, 3]], [[0, 1, 2, 4]], [[0, -1, 2, 3]], [[0, 1, 1, 2]]):  # above its row, outside the table, negative, not a root
        with pytest.raises(ValueError):
            _native.format_clusters("x", names, np.array(bad, np.int32), near)
    for bad in (4, -2):
        worse = near.copy()
        worse["row"][2] = bad
        with pytest.raises(ValueError):
            _native.format_clusters("x", names, one, worse)
    with pytest.raises(ValueError):
        _native.format_clusters("x", names, one, near, rows=[0, 1, 2, 4])
    with pytest.raises(ValueError):
        _native.format_clusters("x", names[:3], one, near)
    lib = _native.lib()
    lib.kp_format_clusters.restype = C.c_int64
    off = np.array([0, 1, 2], np.int64)
    lab, nr = np.array([0, 0], np.int32), _near((1, 5, 3, 2), (0, 5, 3, 2))
    call = lambda **kw: lib.kp_format_clusters(kw.get("locus", b"x"), C.c_int32(kw.get("locus_len", 1)), b"ab", kw.get("off", _p(off)), C.c_int32(kw.get("n", 2)), None,  # noqa: E731
                                               C.c_int32(kw.get("K", 1)), kw.get("lab", _p(lab)), kw.get("near", _p(nr)), None, C.c_int64(kw.get("cap", 0)))
    assert call() == len(b"x\ta\t1\tb\t3\t5\t2\nx\tb\t1\ta\t3\t5\t2\n")  # the sizing call
    for kw in (dict(cap=8), dict(cap=-1), dict(K=9), dict(K=-1), dict(off=None), dict(lab=None), dict(near=None), dict(n=-1), dict(locus_len=-1), dict(locus=None)):
        assert call(**kw) == -1, kw


# ---- LocusRows on hand-made tables ---------------------------------------------------------------------------------------------------------
class _RestatedHandle:
    """Stands in for ``_native.Distances``: the restatement instead of the device."""

    made = 0

    def __init__(self, ctx, rows_matrix):
        type(self).made += 1
        self.ctx, self._h, self.codes = ctx, True, D.unpack(np.asarray(rows_matrix, np.uint64))

    def clusters(self, levels=CU.LEVELS, min_compared=D.MIN_COMPARED, nearest=True):
        return CU.clusters(self.codes, levels, min_compared)

    def pairs(self, max_diff=None, min_compared=0):
        return D.all_pairs(self.codes, max_diff, min_compared)

    def close(self):
        self._h = None


def _two_batches(db):
    return _hand_batch(db, 1, ["a0", "a1", "a2", "a3"], PLAN_1, [0, 0, 1, 1]), _hand_batch(db, 2, ["b0", "b1", "b2"], PLAN_2, [0, 1, 0])


def test_locus_rows_clusters_from_hand_made_tables(monkeypatch):
    monkeypatch.setattr(_native, "Distances", _RestatedHandle)
    db = _hand_db()
    b1, b2 = _two_batches(db)
    lr = LocusRows(db)
    lr.add(b1)
    lr.add(b2)  # L0: assemblies 0, 1, 4, 6; L1: 2, 3, 5
    ctx = object()
    for levels, mc in ((CU.LEVELS, 1), ((0, 40), 0), ((), 1), (CU.EIGHT, 3)):
        rec = lr.clusters(ctx, levels, mc)
        assert rec.dtype == clust_record_dtype(len(levels)) and rec["locus"].tolist() == [0, 0, 0, 0, 1, 1, 1] and rec["assembly"].tolist() == [0, 1, 4, 6, 2, 3, 5]
        got = [(int(r["locus"]), int(r["assembly"]), [int(x) for x in r["labels"]], int(r["nearest"]), int(r["compared"]), int(r["differences"]), int(r["unshared"])) for r in rec]
        assert got == CU.run_records(lr, levels, mc)
        assert all(lab <= a and lab in (0, 1, 4, 6) if L == 0 else lab in (2, 3, 5) for L, a, labs, *_ in got for lab in labs)  # assembly numbers, not rows
        assert all(n == -1 or (n != a and n in ((0, 1, 4, 6) if L == 0 else (2, 3, 5))) for L, a, _, n, *_ in got)
        assert lr.clusters_tsv(ctx, levels, mc) == CU.run_tsv(lr, levels, mc)
    assert lr.clusters_tsv(ctx).count(b"\n") == 7 and lr.clusters_tsv(ctx).startswith(b"L0\ta0\t")
    made = _RestatedHandle.made
    assert lr.tsv(ctx, None, 0).count(b"\n") == 6 + 3 and _RestatedHandle.made == made  # one handle per locus serves both tables
    lr.close()
    lr.clusters(ctx)
    assert _RestatedHandle.made == made + 2


def test_two_loci_one_of_them_with_a_single_row(monkeypatch):
    monkeypatch.setattr(_native, "Distances", _RestatedHandle)
    db = _hand_db()
    b = _hand_batch(db, 1, ["a0", "a1", "a2"], PLAN_1[:3], [0, 0, 1])
    lr = LocusRows(db)
    lr.add(b)
    made = _RestatedHandle.made
    rec = lr.clusters(object(), (0, 5, 64), 0)
    assert _RestatedHandle.made == made + 1  # the single row needs no handle
    assert rec["locus"].tolist() == [0, 0, 1] and rec["labels"][2].tolist() == [2, 2, 2] and rec["nearest"].tolist()[2] == -1 and rec["nearest"].tolist()[:2] == [1, 0]
    lines = lr.clusters_tsv(object(), (0, 5, 64), 0).splitlines()
    assert lines[2] == b"L1\ta2\t1\t1\t1\t.\t.\t.\t." and lines[0].startswith(b"L0\ta0\t1\t") and lines[0].split(b"\t")[5] == b"a1"
    assert lr.clusters_tsv(object(), (0, 5, 64), 0) == CU.run_tsv(lr, (0, 5, 64), 0)


def test_clusters_after_a_state_and_merge_round_trip(monkeypatch):
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
    assert merged.clusters(ctx).tobytes() == whole.clusters(ctx).tobytes() and merged.clusters_tsv(ctx) == whole.clusters_tsv(ctx) == CU.run_tsv(whole)
    merged.clusters(ctx)
    made = _RestatedHandle.made
    merged.merge(whole.state())  # the rows change: the handles go, the next table is made of all fourteen rows
    assert merged.clusters_tsv(ctx).count(b"\n") == 14 and _RestatedHandle.made == made + 2


# ---- the command line's flags ---------------------------------------------------------------------------------------------------------------
def test_command_line_flags():
    from kaptive_amd.cli import build_parser

    ap = build_parser()
    base = ["assembly", "db.npz", "a.fasta"]
    ns = ap.parse_args([*base, "--clusters", "c.tsv"])
    assert ns.clusters == "c.tsv" and not any(hasattr(ns, f) for f in ("cluster_levels", "min_compared", "distances", "aligned", "max_distance"))
    ns = ap.parse_args([*base, "--clusters", "c.tsv", "--cluster-levels", "0,3,7", "--min-compared", "100"])  # --min-compared with --clusters alone
    assert ns.cluster_levels == (0, 3, 7) and ns.min_compared == 100 and not hasattr(ns, "distances")
    ns = ap.parse_args([*base, "--clusters", "c.tsv", "--distances", "d.tsv", "--cluster-levels", "0,1,2,3,4,5,6,7", "--max-distance", "4"])
    assert (ns.clusters, ns.distances, len(ns.cluster_levels), ns.max_distance) == ("c.tsv", "d.tsv", 8, 4)
    assert ap.parse_args([*base, "--clusters", "c.tsv", "--cluster-levels", "5"]).cluster_levels == (5,)
    for bad in (["--cluster-levels", "0,1"], ["--distances", "d.tsv", "--cluster-levels", "0,1"], ["--clusters", "c.tsv", "--cluster-levels", "1,1"],
                ["--clusters", "c.tsv", "--cluster-levels", "2,1"], ["--clusters", "c.tsv", "--cluster-levels", "-1,1"], ["--clusters", "c.tsv", "--cluster-levels", "0,1,2,3,4,5,6,7,8"],
                ["--clusters", "c.tsv", "--cluster-levels", "a,b"], ["--clusters", "c.tsv", "--cluster-levels", ""], ["--clusters", "c.tsv", "--max-distance", "3"],
                ["--min-compared", "3"], ["--clusters", "c.tsv", "--min-compared", "-1"]):  # fmt: skip
        with pytest.raises(SystemExit):
            ap.parse_args([*base, *bad])
