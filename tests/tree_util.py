"""The yardstick of the minimum spanning forest of locus rows (include/kp_spec.h, TREE): a restatement that shares nothing with
kaptive_amd/csrc/kp_tree.h or kaptive_amd/distances.py.  Kruskal over ``distances_util.all_pairs`` sorted by (differences, a, b) with a
plain serial union-find, components as smallest rows, a Newick writer and a line formatter.  Equality with this file is exact:
integers, order, bytes."""

from __future__ import annotations

import ctypes as C
import re

import numpy as np

from tests import distances_util as D

NEWICK_HEADER = b"Locus\tTree\tAssemblies\tNewick\n"
ROW_BITS, DIFF_BITS, MAX_COLUMNS = 18, 28, 1 << 28  # the constants the headers must hold
BARE = re.compile(rb"[A-Za-z0-9_.\-]*\Z")


def forest_of(n_rows: int, every, min_compared: int):
    """(edges PAIR_DTYPE [E], component int32 [R]): Kruskal over ``every`` (all pairs) among the pairs with compared >= min_compared."""
    parent = list(range(n_rows))

    def root(x):
        while parent[x] != x:
            x = parent[x]
        return x

    ok = every[every["compared"] >= min_compared]
    ok = ok[np.lexsort((ok["b"], ok["a"], ok["differences"]))]
    keep = []
    for i, (a, b) in enumerate(zip(ok["a"].tolist(), ok["b"].tolist())):
        a, b = root(a), root(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
            keep.append(i)
    return ok[keep].copy(), np.array([root(r) for r in range(n_rows)], np.int32).reshape(n_rows)


def forest(codes, min_compared: int):
    codes = np.asarray(codes, np.uint8)
    return forest_of(codes.shape[0], D.all_pairs(codes), min_compared)


def components_under(n_rows: int, edges, limit: int) -> np.ndarray:
    """int32 [R]: the smallest row of every row's component under the edges with differences <= limit."""
    parent = list(range(n_rows))

    def root(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for e in edges:
        if e["differences"] <= limit:
            a, b = root(int(e["a"])), root(int(e["b"]))
            parent[max(a, b)] = min(a, b)
    return np.array([root(r) for r in range(n_rows)], np.int32).reshape(n_rows)


def newick_name(name) -> bytes:
    raw = name if isinstance(name, bytes) else str(name).encode("utf-8")
    return raw if BARE.match(raw) else b"'" + raw.replace(b"'", b"''") + b"'"


def newick_of(root: int, edges, names) -> bytes:
    """The Newick text of the tree of ``root``: children ascending by (differences, row), every node named, integer lengths."""
    near = {}
    for e in edges:
        near.setdefault(int(e["a"]), []).append((int(e["differences"]), int(e["b"])))
        near.setdefault(int(e["b"]), []).append((int(e["differences"]), int(e["a"])))
    # children lists from the root outwards, then the text as a list of tokens off a stack: no recursion, so a long chain is fine
    order, above, kids = [root], {root: None}, {}
    for v in order:
        kids[v] = [(d, w) for d, w in sorted(near.get(v, [])) if w != above[v]]
        for _, w in kids[v]:
            above[w] = v
            order.append(w)
    out, todo = [], [("node", root)]
    while todo:
        kind, v = todo.pop()
        if kind == "text":
            out.append(v)
        elif not kids[v]:
            out.append(newick_name(names[v]))
        else:
            out.append(b"(")
            seq = []
            for i, (d, w) in enumerate(kids[v]):
                seq += ([("text", b",")] if i else []) + [("node", w), ("text", b":" + str(d).encode())]
            todo.extend(reversed(seq + [("text", b")" + newick_name(names[v]))]))
    return b"".join(out) + b";"


def newick_lines(locus: str, names, edges, component) -> bytes:
    component = np.asarray(component, np.int32)
    out = []
    for rank, lab in enumerate(sorted(set(component.tolist()))):
        out.append(f"{locus}\t{rank + 1}\t{int((component == lab).sum())}\t".encode() + newick_of(lab, [e for e in edges if component[e["a"]] == lab], names) + b"\n")
    return b"".join(out)


def run_edges(rows, min_compared=D.MIN_COMPARED) -> list:
    """[(locus, a, b, compared, differences, unshared)] of a ``LocusRows``, a and b assembly numbers."""
    out = []
    for L in rows.loci():
        idx, mat = rows.locus_matrix(L)
        for e in forest(D.unpack(mat), min_compared)[0]:
            out.append((L, int(idx[e["a"]]), int(idx[e["b"]]), int(e["compared"]), int(e["differences"]), int(e["unshared"])))
    return out


def run_tree_tsv(rows, min_compared=D.MIN_COMPARED) -> bytes:
    out = []
    for L in rows.loci():
        idx, mat = rows.locus_matrix(L)
        out.append(D.format_lines(rows.db.loci.ids[L], rows.columns(L), [rows.ids[i] for i in idx], forest(D.unpack(mat), min_compared)[0]))
    return b"".join(out)


def run_newick_tsv(rows, min_compared=D.MIN_COMPARED) -> bytes:
    out = []
    for L in rows.loci():
        idx, mat = rows.locus_matrix(L)
        out.append(newick_lines(rows.db.loci.ids[L], [rows.ids[i] for i in idx], *forest(D.unpack(mat), min_compared)))
    return b"".join(out)


# ---- kp_tree.h under g++ -----------------------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness() -> C.CDLL:
    from tests.harness_util import build_harness

    h = build_harness("tree_harness", "kp_tree.h")
    h.kpy_tree_key.restype = h.kpy_tree_key_none.restype = C.c_uint64
    h.kpy_tree_key.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    h.kpy_tree_unpack.argtypes = [C.c_uint64, C.c_void_p]
    h.kpy_tree_fits.argtypes = h.kpy_tree_max_rounds.argtypes = [C.c_int64]
    h.kpy_tree_host.restype = C.c_int64
    return h


def harness_unpack(key: int) -> tuple:
    out = np.zeros(3, np.int32)
    harness().kpy_tree_unpack(key, _p(out))
    return tuple(int(x) for x in out)


def harness_unite(n_rows: int, edges):
    e = np.ascontiguousarray(np.asarray(edges, np.int32).reshape(-1, 2))
    moved, label = np.zeros(len(e), np.int32), np.zeros(n_rows, np.int32)
    harness().kpy_tree_unite(C.c_int32(n_rows), _p(e), C.c_int64(len(e)), _p(moved), _p(label))
    return moved, label


def harness_forest(blocks_matrix, min_compared: int):
    """(edges, component, rounds) of a [R, NB] matrix of blocks through the header alone (kp_tree_host)."""
    m = np.ascontiguousarray(blocks_matrix, np.uint64)
    edges, comp, rounds = np.zeros(max(m.shape[0] - 1, 0), D.PAIR_DTYPE), np.zeros(m.shape[0], np.int32), C.c_int32(0)
    n = harness().kpy_tree_host(_p(m), C.c_int32(m.shape[0]), C.c_int64(m.shape[1]), C.c_int32(min_compared), _p(edges), _p(comp), C.byref(rounds))
    assert n >= 0, "the round bound was reached"
    return edges[:n].copy(), comp, rounds.value
