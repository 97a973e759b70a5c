"""The yardstick of the bootstrap support of the neighbour-joining tree (include/kp_spec.h, BOOTSTRAP): a NumPy restatement that shares
nothing with kaptive_amd/csrc/kp_boot.h or kaptive_amd/distances.py.  The mixer runs on ``np.uint64`` arrays, the 128-bit product of a
draw on Python integers, the weights are a ``np.bincount``, the weighted counts come from code arrays, the trees from
``tests.nj_util.nj``, and support compares exact sets of taxa: no key.  Equality with this file is exact: bytes."""

from __future__ import annotations

import ctypes as C

import numpy as np

from tests import distances_util as D
from tests import nj_util as NJ
from tests.tree_util import newick_name

HEADER = b"Locus\tAssemblies\tTaxa\tReplicates\tNewick\n"
MAX_REPLICATES, MATRIX_BYTES, MAX_BATCH, PLANES = 10000, 2 << 30, 65535, 8  # the constants the headers must hold
MASK = (1 << 64) - 1


def mix(x) -> np.ndarray:
    """MIX of every entry of ``x`` (uint64, any shape)."""
    with np.errstate(over="ignore"):
        z = np.asarray(x, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def draws(seed: int, r: int, W: int) -> np.ndarray:
    """int64 [W]: the columns replicate ``r`` of ``seed`` draws, in draw order."""
    with np.errstate(over="ignore"):
        stream = mix(mix(np.array([seed & MASK], np.uint64)) + np.uint64(r))
        m = mix(stream + np.arange(W, dtype=np.uint64))
    return np.array([(int(v) * W) >> 64 for v in m], np.int64)


def clamp(count) -> np.ndarray:
    return np.minimum(np.asarray(count, np.int64), 255)


def weights(seed: int, r: int, W: int) -> np.ndarray:
    """uint8 [W]: how often every column is drawn, clamped."""
    return clamp(np.bincount(draws(seed, r, W), minlength=W)).astype(np.uint8)


def weighted_counts(ca, cb, w) -> tuple[int, int]:
    """(compared_w, differences_w) of two code arrays under the weights ``w``."""
    ca, cb, w = np.asarray(ca), np.asarray(cb), np.asarray(w, np.int64)
    both = (ca < 4) & (cb < 4)
    return int((w * both).sum()), int((w * (both & (ca != cb))).sum())


def matrix_of(codes, taxa, w) -> np.ndarray:
    """float64 [n, n]: the distances of the taxa under the weights ``w``; a pair without a compared column is 0 apart."""
    c = np.asarray(codes, np.uint8)[np.asarray(taxa, np.int64)]
    w = np.asarray(w, np.int64)[None, :]
    n = len(c)
    out = np.zeros((n, n), np.float64)
    for a in range(n - 1):
        x, y = c[a][None, :], c[a + 1 :]
        both = (x < 4) & (y < 4)
        comp, diff = (w * both).sum(axis=1).astype(np.float64), (w * (both & (x != y))).sum(axis=1).astype(np.float64)
        d = np.zeros(len(comp), np.float64)
        np.divide(diff, comp, out=d, where=comp > 0)
        out[a, a + 1 :] = out[a + 1 :, a] = d
    return out


def record_splits(n: int, nodes) -> list:
    """For every record of a tree of n taxa: the set of taxa below the node it made, on the side without taxon 0, as a frozenset --
    or None for a record without an inner edge (the last; every record of fewer than four taxa)."""
    below = {k: frozenset([k]) for k in range(n)}
    everyone = frozenset(range(n))
    out = []
    for t, rec in enumerate(nodes):
        if n < 4 or t >= n - 3:
            out.append(None)
            continue
        s = below[int(rec["a"])] | below[int(rec["b"])]
        below[n + t] = s
        out.append(everyone - s if 0 in s else s)
    return out


def support_of(n: int, ref_nodes, replicate_nodes) -> np.ndarray:
    """int32 [len(ref_nodes)]: the replicate trees that hold every record's split; -1 where there is none to hold."""
    held = [set(s for s in record_splits(n, nodes) if s is not None) for nodes in replicate_nodes]
    return np.array([-1 if s is None else sum(s in h for h in held) for s in record_splits(n, ref_nodes)], np.int32).reshape(-1)


def bootstrap(codes, min_compared: int, seed: int, replicates: int):
    """(taxa, nodes of the tree, NODE_DTYPE [replicates, records] of the replicates' trees, support int32 [records])."""
    codes = np.asarray(codes, np.uint8)
    taxa, nodes = NJ.tree(codes, min_compared)
    W = codes.shape[1]
    reps = [NJ.nj(matrix_of(codes, taxa, weights(seed, r, W))) for r in range(replicates)]
    trees = np.stack(reps).reshape(replicates, len(nodes)) if len(nodes) else np.zeros((replicates, 0), NJ.NODE_DTYPE)
    return taxa, nodes, trees, support_of(len(taxa), nodes, reps)


def newick(names, taxa, nodes, support) -> bytes:
    """``NJ.newick`` with the support of every record that has one behind its node's closing parenthesis."""
    n = len(taxa)
    if len(nodes) == 0:
        return b""
    out, todo = [], [("node", n + len(nodes) - 1)]
    while todo:
        kind, v = todo.pop()
        if kind == "text":
            out.append(v)
        elif v < n:
            out.append(newick_name(names[int(taxa[v])]))
        else:
            r = nodes[v - n]
            kids = [(int(r["a"]), float(r["la"])), (int(r["b"]), float(r["lb"]))] + ([(int(r["c"]), float(r["lc"]))] if r["c"] >= 0 else [])
            seq = [("text", b"(")]
            for i, (w, length) in enumerate(kids):
                seq += ([("text", b",")] if i else []) + [("node", w), ("text", b":" + format(length, ".9g").encode())]
            label = str(int(support[v - n])).encode() if n >= 4 and v - n < n - 3 else b""
            todo.extend(reversed(seq + [("text", b")" + label)]))
    return b"".join(out) + b";"


def line(locus: str, names, taxa, nodes, support, replicates: int) -> bytes:
    return b"" if len(nodes) == 0 else f"{locus}\t{len(names)}\t{len(taxa)}\t{replicates}\t".encode() + newick(names, taxa, nodes, support) + b"\n"


def run_tsv(rows, replicates: int, seed: int, min_compared=D.MIN_COMPARED) -> bytes:
    """The lines of the table of a ``LocusRows`` with support values, from its matrices alone."""
    out = []
    for L in rows.loci():
        idx, mat = rows.locus_matrix(L)
        if len(idx) < 2:
            continue
        taxa, nodes, _, support = bootstrap(D.unpack(mat), min_compared, seed, replicates)
        out.append(line(rows.db.loci.ids[L], [rows.ids[i] for i in idx], taxa, nodes, support, replicates))
    return b"".join(out)


# ---- kp_boot.h under g++ ---------------------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness() -> C.CDLL:
    from tests.harness_util import build_harness

    h = build_harness("boot_harness", "kp_boot.h")
    h.kpy_boot_mix.restype = C.c_uint64
    h.kpy_boot_mix.argtypes = [C.c_uint64]
    h.kpy_boot_key.restype = C.c_uint64
    h.kpy_boot_total.restype = C.c_uint64
    h.kpy_boot_batch.restype = C.c_int32
    h.kpy_boot_batch.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    return h


def harness_draws(seed: int, r: int, W: int) -> np.ndarray:
    out = np.zeros(W, np.int64)
    harness().kpy_boot_draws(C.c_uint64(seed & MASK), C.c_int64(r), C.c_int64(W), _p(out))
    return out


def harness_weights(seed: int, r: int, W: int) -> np.ndarray:
    out = np.zeros(W, np.uint8)
    harness().kpy_boot_weights(C.c_uint64(seed & MASK), C.c_int64(r), C.c_int64(W), _p(out))
    return out


def harness_clamp(count) -> np.ndarray:
    c = np.ascontiguousarray(count, np.uint32)
    out = np.zeros(len(c), np.uint32)
    harness().kpy_boot_clamp(_p(c), C.c_int64(len(c)), _p(out))
    return out


def harness_counts(a_blocks, b_blocks, w) -> tuple[int, int]:
    a, b, w = np.ascontiguousarray(a_blocks, np.uint64), np.ascontiguousarray(b_blocks, np.uint64), np.ascontiguousarray(w, np.uint8)
    out = np.zeros(2, np.int32)
    harness().kpy_boot_row_counts(_p(a), _p(b), C.c_int64(len(a)), _p(w), _p(out))
    return int(out[0]), int(out[1])


def harness_key(taxa) -> int:
    t = np.ascontiguousarray(taxa, np.int32)
    return int(harness().kpy_boot_key(_p(t), C.c_int64(len(t))))


def harness_walk(n: int, nodes) -> np.ndarray:
    """uint64 [n - 3, 3]: (key, size, holds taxon 0 below the node) of every record with an inner edge."""
    nd = np.ascontiguousarray(nodes, NJ.NODE_DTYPE)
    out = np.zeros((max(n - 3, 0), 3), np.uint64)
    harness().kpy_boot_walk(_p(nd), C.c_int32(n), _p(out))
    return out
