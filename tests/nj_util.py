"""The yardstick of the neighbour-joining tree of locus rows (include/kp_spec.h, NJ): a NumPy restatement that shares nothing with
kaptive_amd/csrc/kp_nj.h or kaptive_amd/distances.py.  The taxa and the matrix come from code arrays, SUM64 is ``reshape(-1, 64)`` row
adds, a join is one ``argmin`` over the masked upper triangle in row-major order, and the Newick writer and the split set work on the
record list.  NumPy rounds every operation to binary64 and fuses none, so equality with this file is exact: bytes."""

from __future__ import annotations

import ctypes as C

import numpy as np

from tests import distances_util as D
from tests.tree_util import newick_name

NODE_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("c", "<i4"), ("pad", "<i4"), ("la", "<f8"), ("lb", "<f8"), ("lc", "<f8")])
HEADER = b"Locus\tAssemblies\tTaxa\tNewick\n"
MAX_TAXA = 16384  # the constant the headers must hold


def sum64(v) -> np.ndarray:
    """SUM64 along the last axis of ``v`` [..., m]: float64 [...]."""
    v = np.asarray(v, np.float64)
    m = v.shape[-1]
    pad = np.zeros(v.shape[:-1] + (-m % 64,), np.float64)  # (a partial sum is never -0.0, so a trailing + 0.0 changes no bit)
    rows = np.concatenate([v, pad], axis=-1).reshape(v.shape[:-1] + (-1, 64))
    s = np.zeros(v.shape[:-1] + (64,), np.float64)
    for k in range(rows.shape[-2]):
        s = s + rows[..., k, :]
    o = 32
    while o >= 1:
        s = s[..., :o] + s[..., o : 2 * o]
        o //= 2
    return s[..., 0]


def taxa_of(codes, min_compared: int) -> np.ndarray:
    """int32 rows of ``codes`` [R, W] that are taxa: 2 bases >= W + max(min_compared, 1)."""
    codes = np.asarray(codes, np.uint8)
    bases = (codes < 4).sum(axis=1)
    return np.flatnonzero(2 * bases >= codes.shape[1] + max(int(min_compared), 1)).astype(np.int32)


def matrix_of(codes, taxa) -> np.ndarray:
    """float64 [n, n]: the p-distances of the taxa, one division each."""
    c = np.asarray(codes, np.uint8)[np.asarray(taxa, np.int64)]
    n = len(c)
    out = np.zeros((n, n), np.float64)
    for a in range(n - 1):
        x, y = c[a][None, :], c[a + 1 :]
        both = (x < 4) & (y < 4)
        comp, diff = both.sum(axis=1).astype(np.float64), (both & (x != y)).sum(axis=1).astype(np.float64)
        assert (comp > 0).all()  # the taxon rule's reason
        out[a, a + 1 :] = out[a + 1 :, a] = diff / comp
    return out


def nj(dist) -> np.ndarray:
    """NODE_DTYPE records of the tree of a dense matrix, by the section's rule."""
    d = np.array(dist, np.float64)
    n = d.shape[0]
    if n <= 1:
        return np.zeros(0, NODE_DTYPE)
    if n == 2:
        return np.array([(0, 1, -1, 0, 0.5 * d[0, 1], 0.5 * d[0, 1], 0.0)], NODE_DTYPE)
    node = list(range(n))
    R = sum64(d)
    out, m, nxt = [], n, n
    while m > 3:
        f = np.float64(m - 2)
        q = ((f * d[:m, :m]) - R[:m, None]) - R[None, :m]
        q[np.tril_indices(m)] = np.inf
        i, j = divmod(int(np.argmin(q)), m)  # the first minimum in row-major order: the smallest (Q, a, b)
        dij = d[i, j]
        delta = (R[i] - R[j]) / f
        li = 0.5 * (dij + delta)
        out.append((node[i], node[j], -1, 0, li, dij - li, 0.0))
        k = np.array([x for x in range(m) if x != i and x != j], np.int64)
        u = 0.5 * ((d[i, k] + d[j, k]) - dij)
        R[k] = ((R[k] - d[i, k]) - d[j, k]) + u
        d[i, k] = d[k, i] = u
        d[i, i] = 0.0
        node[i] = nxt
        nxt += 1
        if j != m - 1:
            d[j, :m] = d[m - 1, :m]
            d[:m, j] = d[:m, m - 1]
            d[j, j] = 0.0
            R[j] = R[m - 1]
            node[j] = node[m - 1]
        m -= 1
        R[i] = sum64(d[i, :m])
    lx = 0.5 * ((d[0, 1] + d[0, 2]) - d[1, 2])
    ly = 0.5 * ((d[0, 1] + d[1, 2]) - d[0, 2])
    lz = 0.5 * ((d[0, 2] + d[1, 2]) - d[0, 1])
    out.append((node[0], node[1], node[2], 0, lx, ly, lz))
    return np.array(out, NODE_DTYPE)


def tree(codes, min_compared: int):
    """(taxa int32 [n], records) of a code matrix."""
    t = taxa_of(codes, min_compared)
    return t, nj(matrix_of(codes, t))


def newick(names, taxa, nodes) -> bytes:
    """The Newick text of a record list (``names`` by row of the matrix), without recursion; b"" for no record."""
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
            todo.extend(reversed(seq + [("text", b")")]))
    return b"".join(out) + b";"


def line(locus: str, names, taxa, nodes) -> bytes:
    return b"" if len(nodes) == 0 else f"{locus}\t{len(names)}\t{len(taxa)}\t".encode() + newick(names, taxa, nodes) + b"\n"


def splits(n: int, nodes) -> set:
    """The non-trivial splits of a record list as frozensets of the taxa on the side without taxon 0."""
    below = {k: frozenset([k]) for k in range(n)}
    out = set()
    for r, rec in enumerate(nodes):
        kids = [int(rec["a"]), int(rec["b"])] + ([int(rec["c"])] if rec["c"] >= 0 else [])
        if r < len(nodes) - 1 or len(kids) == 2:
            below[n + r] = below[kids[0]] | below[kids[1]]
    for v, s in below.items():
        if 1 < len(s) < n - 1:
            out.add(s if 0 not in s else frozenset(range(n)) - s)
    return out


def total_length(nodes) -> float:
    return float(nodes["la"].sum() + nodes["lb"].sum() + nodes["lc"].sum())


def run_tsv(rows, min_compared=D.MIN_COMPARED) -> bytes:
    """The lines of the table of a ``LocusRows``, from its matrices alone."""
    out = []
    for L in rows.loci():
        idx, mat = rows.locus_matrix(L)
        if len(idx) < 2:
            continue
        taxa, nodes = tree(D.unpack(mat), min_compared)
        out.append(line(rows.db.loci.ids[L], [rows.ids[i] for i in idx], taxa, nodes))
    return b"".join(out)


# ---- a planted additive tree ---------------------------------------------------------------------------------------------------------
def additive(rng, n: int, cols_per_branch=(1, 4)):
    """(codes [n, W], splits, mutations, W): a random unrooted binary tree of n >= 4 leaves whose every branch owns columns of its
    own, in which the leaves on one side differ from the founder -- fully covered rows, so d = (branches between) / W exactly
    additive.  W is padded up to a multiple of 16 with columns nobody mutates."""
    # random pairs of clusters are merged until three are left: every cluster ever made hangs on a branch of its own
    clusters = [frozenset([k]) for k in range(n)]
    branches = [frozenset([k]) for k in range(n)]  # a branch as the leaves on one side of it; first every leaf's own
    while len(clusters) > 3:
        i, j = sorted(rng.choice(len(clusters), 2, replace=False).tolist())
        merged = clusters[i] | clusters[j]
        clusters = [c for k, c in enumerate(clusters) if k not in (i, j)] + [merged]
        branches.append(merged)
    widths = rng.integers(cols_per_branch[0], cols_per_branch[1] + 1, len(branches))
    used = int(widths.sum())
    W = -(-used // 16) * 16
    founder = rng.integers(0, 4, W).astype(np.uint8)
    codes = np.tile(founder, (n, 1))
    at = 0
    for side, w in zip(branches, widths):
        rows = np.array(sorted(side), np.int64)
        codes[rows[:, None], np.arange(at, at + w)[None, :]] = (founder[at : at + w] + 1) % 4
        at += int(w)
    planted = {s if 0 not in s else frozenset(range(n)) - s for s in branches if 1 < len(s) < n - 1}
    return codes, planted, used, W


# ---- kp_nj.h under g++ -----------------------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness() -> C.CDLL:
    from tests.harness_util import build_harness

    h = build_harness("nj_harness", "kp_nj.h")
    h.kpy_nj_sum64.restype = C.c_double
    h.kpy_nj_host.restype = C.c_int64
    h.kpy_nj_max_taxa.restype = C.c_int32
    h.kpy_nj_taxon.argtypes = [C.c_int64, C.c_int64, C.c_int32]
    return h


def harness_sum64(v) -> float:
    v = np.ascontiguousarray(v, np.float64)
    return float(harness().kpy_nj_sum64(_p(v), C.c_int64(len(v))))


def harness_nj(dist) -> np.ndarray:
    d = np.ascontiguousarray(dist, np.float64)
    n = d.shape[0] if d.ndim == 2 else 0
    out = np.zeros(max(n - 2, 1), NODE_DTYPE)
    made = harness().kpy_nj_host(_p(d), C.c_int32(n), _p(out))
    return out[:made].copy()


def harness_matrix(blocks_matrix, min_compared: int):
    """(taxa, D) of a [R, NB] matrix of blocks through the header alone (kp_nj_matrix_host)."""
    m = np.ascontiguousarray(blocks_matrix, np.uint64)
    taxa = np.zeros(max(m.shape[0], 1), np.int32)
    h = harness()
    n = h.kpy_nj_matrix_host(_p(m), C.c_int32(m.shape[0]), C.c_int64(m.shape[1]), C.c_int32(min_compared), _p(taxa), None)
    dist = np.zeros((n, n), np.float64)
    assert h.kpy_nj_matrix_host(_p(m), C.c_int32(m.shape[0]), C.c_int64(m.shape[1]), C.c_int32(min_compared), _p(taxa), _p(dist)) == n
    return taxa[:n].copy(), dist
