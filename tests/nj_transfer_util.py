"""The yardstick of the transfer bootstrap of the neighbour-joining tree (include/kp_spec.h, TRANSFER): a restatement on Python sets that
shares nothing with kaptive_amd/csrc/kp_transfer.h or kaptive_amd/distances.py.  The splits are ``tests.nj_boot_util.record_splits``'
frozensets, a transfer distance is brute force over every split of the replicate's tree with ``len(A ^ B)``, the sum is a sum, the
label a ``fractions.Fraction``.  Equality with this file is exact: integers and bytes."""

from __future__ import annotations

import ctypes as C
from fractions import Fraction

import numpy as np

from tests import distances_util as D
from tests import nj_boot_util as B
from tests import nj_util as NJ
from tests.tree_util import newick_name

# the known answer of the spec: six taxa
KNOWN_REF = ((0, 1, -1), (6, 2, -1), (7, 3, -1), (8, 4, 5))
KNOWN_REP = ((0, 3, -1), (6, 1, -1), (7, 2, -1), (8, 4, 5))
KNOWN_PHI, KNOWN_LABELS = [1, 1, 0, -1], [b"0.000", b"0.500", b"1.000"]


def records(rows) -> np.ndarray:
    """NODE_DTYPE records of (a, b, c) triples, every length 0."""
    out = np.zeros(len(rows), NJ.NODE_DTYPE)
    for t, (a, b, c) in enumerate(rows):
        out[t]["a"], out[t]["b"], out[t]["c"] = a, b, c
    return out


def caterpillar(n: int) -> np.ndarray:
    """(0, 1), (n, 2), (n + 1, 3), ...: every split is a prefix of the taxa; depths 2, 3, .. n / 2 and down again."""
    return records([(0, 1, -1)] + [(n + t - 1, t + 1, -1) for t in range(1, n - 3)] + [(2 * n - 4, n - 2, n - 1)])


def grown(n: int, rng=None) -> np.ndarray:
    """A valid record list of n >= 4 taxa: the first two open nodes are joined and the new node queues behind the others -- a balanced
    tree --, or with ``rng`` two random ones are."""
    todo, out = list(range(n)), []
    while len(todo) > 3:
        i, j = (0, 1) if rng is None else sorted(rng.choice(len(todo), 2, replace=False).tolist())
        b, a = todo.pop(j), todo.pop(i)
        out.append((a, b, -1))
        todo.append(n + len(out) - 1)
    return records(out + [tuple(todo)])


def depths(n: int, nodes) -> list:
    """min(|A|, n - |A|) of every record's split; None without an inner edge."""
    return [None if s is None else min(len(s), n - len(s)) for s in B.record_splits(n, nodes)]


def phi_of(n: int, ref_nodes, replicate_nodes) -> np.ndarray:
    """int32 [len(ref_nodes)]: the transfer distance of every record of the supported tree to one replicate's tree; -1 without an
    inner edge."""
    theirs = [s for s in B.record_splits(n, replicate_nodes) if s is not None]
    out = []
    for A in B.record_splits(n, ref_nodes):
        if A is None:
            out.append(-1)
            continue
        best = min(len(A), n - len(A)) - 1
        for S in theirs:
            H = len(A ^ S)
            best = min(best, H, n - H)
        out.append(best)
    return np.array(out, np.int32).reshape(-1)


def sums_of(n: int, ref_nodes, replicate_trees):
    """(support int32, transfer int64, phi int32 [replicates, records]) of a supported tree against replicate trees."""
    phi = np.stack([phi_of(n, ref_nodes, t) for t in replicate_trees]).reshape(len(replicate_trees), len(ref_nodes))
    inner = np.array([s is not None for s in B.record_splits(n, ref_nodes)], bool).reshape(-1)
    support = np.where(inner, (phi == 0).sum(axis=0), -1).astype(np.int32)
    transfer = np.where(inner, phi.astype(np.int64).sum(axis=0), -1).astype(np.int64)
    return support, transfer, phi


def transfer(codes, min_compared: int, seed: int, replicates: int, ref_nodes=None):
    """(taxa, nodes, trees, support, transfer, phi): ``nj_boot_util.bootstrap``'s replicates against the tree itself or ``ref_nodes``."""
    taxa, nodes, trees, support = B.bootstrap(codes, min_compared, seed, replicates)
    if ref_nodes is None and len(taxa) >= 4:
        s, tr, phi = sums_of(len(taxa), nodes, trees)
        assert s.tolist() == support.tolist()  # the support relation of the spec
        return taxa, nodes, trees, s, tr, phi
    if len(taxa) < 4:
        k = len(nodes)
        return taxa, nodes, trees, np.full(k, -1, np.int32), np.full(k, -1, np.int64), np.full((replicates, k), -1, np.int32)
    return (taxa, ref_nodes, trees, *sums_of(len(taxa), ref_nodes, trees))


def label(transfer_sum: int, replicates: int, depth: int) -> bytes:
    """1 - transfer / (replicates * (depth - 1)) rounded half up to thousandths, three decimals."""
    tbe = 1 - Fraction(int(transfer_sum), int(replicates) * (int(depth) - 1))
    k = (tbe * 1000 + Fraction(1, 2)).__floor__()
    return f"{k // 1000}.{k % 1000:03d}".encode()


def newick(names, taxa, nodes, transfer_sums, replicates: int) -> bytes:
    """``nj_boot_util.newick`` with the transfer label of every record that has one behind its node's closing parenthesis."""
    n = len(taxa)
    if len(nodes) == 0:
        return b""
    deep = depths(n, nodes)
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
            mark = label(transfer_sums[v - n], replicates, deep[v - n]) if n >= 4 and v - n < n - 3 else b""
            todo.extend(reversed(seq + [("text", b")" + mark)]))
    return b"".join(out) + b";"


def line(locus: str, names, taxa, nodes, transfer_sums, replicates: int) -> bytes:
    return b"" if len(nodes) == 0 else f"{locus}\t{len(names)}\t{len(taxa)}\t{replicates}\t".encode() + newick(names, taxa, nodes, transfer_sums, replicates) + b"\n"


def run_tsv(rows, replicates: int, seed: int, min_compared=D.MIN_COMPARED) -> bytes:
    """The lines of the table of a ``LocusRows`` with transfer support, from its matrices alone."""
    out = []
    for L in rows.loci():
        idx, mat = rows.locus_matrix(L)
        if len(idx) < 2:
            continue
        taxa, nodes, _, _, sums, _ = transfer(D.unpack(mat), min_compared, seed, replicates)
        out.append(line(rows.db.loci.ids[L], [rows.ids[i] for i in idx], taxa, nodes, sums, replicates))
    return b"".join(out)


# ---- kp_transfer.h under g++ -----------------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness() -> C.CDLL:
    from tests.harness_util import build_harness

    h = build_harness("transfer_harness", "kp_transfer.h")
    h.kpy_transfer_label.restype = C.c_int64
    h.kpy_transfer_label.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    for f in (h.kpy_transfer_depth, h.kpy_transfer_delta):
        f.restype = C.c_int32
    h.kpy_transfer_depth.argtypes = [C.c_int32] * 2
    h.kpy_transfer_delta.argtypes = [C.c_int32] * 4
    return h


def harness_phi(n: int, ref_nodes, replicate_nodes) -> np.ndarray:
    """int32 [n - 3]: kp_transfer_host's distances."""
    ref, rep = np.ascontiguousarray(ref_nodes, NJ.NODE_DTYPE), np.ascontiguousarray(replicate_nodes, NJ.NODE_DTYPE)
    out = np.full(max(n - 3, 0), -9, np.int32)
    harness().kpy_transfer_phi(_p(ref), _p(rep), C.c_int32(n), _p(out))
    return out


def harness_sizes(n: int, nodes) -> np.ndarray:
    nd = np.ascontiguousarray(nodes, NJ.NODE_DTYPE)
    out = np.zeros(max(n - 3, 0), np.int32)
    harness().kpy_transfer_sizes(_p(nd), C.c_int32(n), _p(out))
    return out
