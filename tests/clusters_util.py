"""The yardstick of the clusters and nearest neighbours of locus rows (include/kp_spec.h, CLUSTERS): a numpy restatement that shares
nothing with kaptive_amd/csrc/kp_clust.h or kaptive_amd/distances.py.  A serial union-find over ``distances_util.all_pairs`` per
level, an argmin over (differences, s) per row, and a line formatter.  Equality with this file is exact: integers, order, bytes."""

from __future__ import annotations

import ctypes as C

import numpy as np

from tests import distances_util as D

NEAREST_DTYPE = np.dtype([("row", "<i4"), ("compared", "<i4"), ("differences", "<i4"), ("unshared", "<i4")])
MAX_LEVELS, LEVELS = 8, (0, 1, 2, 5, 10)  # the constants the headers must hold
EIGHT = (0, 1, 2, 3, 5, 6, 10, 40)  # eight levels: below, at and above distances_util's SPLIT of the device tests


def labels_of(n_rows: int, every, levels, min_compared: int) -> np.ndarray:
    """int32 [K, R]: every row's label (the smallest row of its component) under the edges of each level; ``every`` holds all pairs."""
    out = np.zeros((len(levels), n_rows), np.int32)
    for k, t in enumerate(levels):
        parent = list(range(n_rows))

        def root(x):
            while parent[x] != x:
                x = parent[x]
            return x

        edges = every[(every["differences"] <= t) & (every["compared"] >= min_compared)]
        for a, b in zip(edges["a"].tolist(), edges["b"].tolist()):
            a, b = root(a), root(b)
            if a != b:
                parent[max(a, b)] = min(a, b)
        out[k] = [root(r) for r in range(n_rows)]
    return out


def nearest_of(n_rows: int, every, min_compared: int) -> np.ndarray:
    """NEAREST_DTYPE [R]: for every row the partner with the smallest (differences, partner) among compared >= min_compared."""
    out = np.zeros(n_rows, NEAREST_DTYPE)
    out["row"] = -1
    ok = every[every["compared"] >= min_compared]
    for r in range(n_rows):
        mine = ok[(ok["a"] == r) | (ok["b"] == r)]
        if len(mine):
            other = np.where(mine["a"] == r, mine["b"], mine["a"])
            best = np.lexsort((other, mine["differences"]))[0]
            out[r] = (other[best], mine["compared"][best], mine["differences"][best], mine["unshared"][best])
    return out


def clusters(codes, levels, min_compared: int):
    """(labels int32 [K, R], nearest NEAREST_DTYPE [R]) of the rows of ``codes`` [R, columns]."""
    codes = np.asarray(codes, np.uint8)
    every = D.all_pairs(codes)
    return labels_of(codes.shape[0], every, levels, min_compared), nearest_of(codes.shape[0], every, min_compared)


def numbers_of(labels) -> np.ndarray:
    """Cluster numbers [K, R]: the 1-based rank of every label among the distinct labels of its level."""
    labels = np.asarray(labels, np.int32)
    out = np.zeros(labels.shape, np.int64)
    for k in range(labels.shape[0]):
        rank = {int(v): i + 1 for i, v in enumerate(sorted(set(labels[k].tolist())))}
        out[k] = [rank[int(v)] for v in labels[k]]
    return out


def header(levels) -> bytes:
    return ("\t".join(["Locus", "Assembly", *(f"HC{t}" for t in levels), "Nearest", "Differences", "Compared", "Unshared"]) + "\n").encode()


def format_lines(locus: str, names, labels, nearest) -> bytes:
    num = numbers_of(np.asarray(labels, np.int32).reshape(-1, len(nearest)))
    lines = []
    for r, n in enumerate(nearest):
        tail = [names[n["row"]], n["differences"], n["compared"], n["unshared"]] if n["row"] >= 0 else [".", ".", ".", "."]
        lines.append("\t".join(str(x) for x in [locus, names[r], *num[:, r], *tail]) + "\n")
    return "".join(lines).encode()


def run_records(rows, levels=LEVELS, min_compared=D.MIN_COMPARED) -> list:
    """[(locus, assembly, labels as assembly numbers, nearest assembly or -1, compared, differences, unshared)] of a ``LocusRows``."""
    out = []
    for L in rows.loci():
        idx, mat = rows.locus_matrix(L)
        labels, near = clusters(D.unpack(mat), levels, min_compared)
        for r in range(len(idx)):
            n = near[r]
            out.append((L, int(idx[r]), [int(idx[x]) for x in labels[:, r]], int(idx[n["row"]]) if n["row"] >= 0 else -1, int(n["compared"]),
                        int(n["differences"]), int(n["unshared"])))  # fmt: skip
    return out


def run_tsv(rows, levels=LEVELS, min_compared=D.MIN_COMPARED) -> bytes:
    out = []
    for L in rows.loci():
        idx, mat = rows.locus_matrix(L)
        out.append(format_lines(rows.db.loci.ids[L], [rows.ids[i] for i in idx], *clusters(D.unpack(mat), levels, min_compared)))
    return b"".join(out)


# ---- kp_clust.h under g++ ----------------------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness() -> C.CDLL:
    from tests.harness_util import build_harness

    h = build_harness("clust_harness", "kp_clust.h")
    h.kpy_clust_key.restype = C.c_uint64
    h.kpy_clust_key.argtypes = [C.c_int32, C.c_int32]
    h.kpy_clust_key_none.restype = C.c_uint64
    h.kpy_clust_key_row.argtypes = h.kpy_clust_key_differences.argtypes = [C.c_uint64]
    return h


def harness_first_level(levels, differences: int) -> int:
    lv = np.ascontiguousarray(levels, np.int32)
    return int(harness().kpy_clust_first_level(_p(lv), C.c_int32(len(lv)), C.c_int32(differences)))


def harness_labels(n_rows: int, edges, levels, check_invariant: bool = True) -> np.ndarray:
    """int32 [K, R]: the labels after uniting ``edges`` [(a, b, differences)] in the order given (kp_clust_edge, then kp_clust_find
    of every row); with ``check_invariant`` the harness checks parent[x] <= x after every call; a breach fails the assertion below."""
    lv = np.ascontiguousarray(levels, np.int32)
    e = np.ascontiguousarray(np.asarray(edges, np.int32).reshape(-1, 3))
    out = np.zeros((len(lv), n_rows), np.int32)
    rc = harness().kpy_clust_labels(C.c_int32(n_rows), _p(e), C.c_int64(len(e)), _p(lv), C.c_int32(len(lv)), C.c_int32(int(check_invariant)), _p(out))
    assert rc == 0, "parent[x] <= x was broken"
    return out


def harness_clusters(blocks_matrix, levels, min_compared: int):
    """(labels, nearest) of a [R, NB] matrix of blocks through the header alone: counts word by word, first level, unite, keys."""
    m = np.ascontiguousarray(blocks_matrix, np.uint64)
    lv = np.ascontiguousarray(levels, np.int32)
    labels, near = np.zeros((len(lv), m.shape[0]), np.int32), np.zeros(m.shape[0], NEAREST_DTYPE)
    rc = harness().kpy_clust_matrix(_p(m), C.c_int32(m.shape[0]), C.c_int64(m.shape[1]), _p(lv), C.c_int32(len(lv)), C.c_int32(min_compared), _p(labels), _p(near))
    assert rc == 0
    return labels, near
