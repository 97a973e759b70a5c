"""The yardstick of small parsimony on the neighbour-joining tree (include/kp_spec.h, PARSIMONY): a restatement on Python sets, one
column at a time, that shares nothing with kaptive_amd/csrc/kp_pars.h or kaptive_amd/distances.py -- no bit plane, no machine word.
A leaf's set is ``{code}`` or all four bases, a node's set comes from counting its children's sets, the states from one walk down, a
change from comparing two states; the exhaustive minimum tries every assignment of the inner nodes.  Equality with this file is
exact: integers and bytes."""

from __future__ import annotations

import ctypes as C
import itertools

import numpy as np

from tests import distances_util as D
from tests import nj_transfer_util as TR
from tests import nj_util as NJ
from tests.tree_util import newick_name

SITE_DTYPE = np.dtype([("column", "<i4"), ("steps", "<i4"), ("alleles", "<i4"), ("pad", "<i4")])
CHANGE_DTYPE = np.dtype([("column", "<i4"), ("node", "<i4"), ("parent", "<i4"), ("from", "u1"), ("to", "u1"), ("pad", "<u2")])
HOMOPLASY_HEADER = b"Locus\tGene\tPosition\tColumn\tAlleles\tSteps\tExcess\n"
CHANGES_HEADER = b"Locus\tNode\tTip A\tTip B\tTips\tGene\tPosition\tColumn\tFrom\tTo\n"
ALL = frozenset(range(4))

# the known answers of the spec: NJ's five-taxon tree and five columns, the taxa's bases in order
KNOWN_TREE = ((0, 1, -1), (5, 2, -1), (6, 4, 3))
KNOWN = {  # column -> (steps, alleles, [(node, parent, from, to)])
    "aaaaa": (0, 1, []),
    "ccaaa": (1, 3, [(5, 6, "a", "c")]),
    "gagaa": (2, 5, [(1, 5, "g", "a"), (6, 7, "a", "g")]),
    "ccctg": (2, 14, [(3, 7, "c", "t"), (4, 7, "c", "g")]),
    "ccnaa": (1, 3, [(6, 7, "a", "c")]),
}


# ---- trees ---------------------------------------------------------------------------------------------------------------------------
def kids(rec) -> list:
    return [int(rec["a"]), int(rec["b"])] + ([int(rec["c"])] if rec["c"] >= 0 else [])


def tree_of(n: int, rng=None, shape: str = "grown") -> np.ndarray:
    """A valid record list of n >= 2 taxa: ``grown`` balanced, or random with ``rng``; ``caterpillar``."""
    if n == 2:
        return TR.records([(0, 1, -1)])
    if n == 3:
        return TR.records([(0, 1, 2)])
    return TR.caterpillar(n) if shape == "caterpillar" else TR.grown(n, rng)


def parents(n: int, nodes) -> dict:
    return {w: n + t for t, rec in enumerate(nodes) for w in kids(rec)}


def below(n: int, nodes) -> dict:
    """node -> frozenset of the taxa below it."""
    out = {k: frozenset([k]) for k in range(n)}
    for t, rec in enumerate(nodes):
        out[n + t] = frozenset().union(*(out[w] for w in kids(rec)))
    return out


# ---- one column ----------------------------------------------------------------------------------------------------------------------------
def column(n: int, nodes, col):
    """(steps, alleles, states {node: state}, changes [(node, parent, from, to)] ascending by node) of one column: ``col[k]`` the
    code of taxon k, 0..3 a base, anything else missing."""
    sets = {k: frozenset([int(col[k])]) if col[k] < 4 else ALL for k in range(n)}
    alleles = sum(1 << b for b in {int(c) for c in col if c < 4})
    steps = 0
    for t, rec in enumerate(nodes):
        ch = kids(rec)
        count = {s: sum(s in sets[w] for w in ch) for s in range(4)}
        most = max(count.values())
        sets[n + t] = frozenset(s for s in range(4) if count[s] == most)
        steps += len(ch) - most
    top = n + len(nodes) - 1
    state = {top: min(sets[top])}
    changes = []
    for t in range(len(nodes) - 1, -1, -1):
        for w in kids(nodes[t]):
            state[w] = state[n + t] if state[n + t] in sets[w] else min(sets[w])
            if state[w] != state[n + t]:
                changes.append((w, n + t, state[n + t], state[w]))
    return steps, alleles, state, sorted(changes)


def exhaustive(n: int, nodes, col) -> int:
    """The fewest changes over every assignment of states to the inner nodes (n <= 7); a missing leaf costs nothing."""
    edges = [(n + t, w) for t, rec in enumerate(nodes) for w in kids(rec)]
    best = None
    for inner in itertools.product(range(4), repeat=len(nodes)):
        cost = 0
        for p, w in edges:
            if w >= n:
                cost += inner[p - n] != inner[w - n]
            elif col[w] < 4:
                cost += inner[p - n] != int(col[w])
        best = cost if best is None else min(best, cost)
    return best


# ---- a whole matrix --------------------------------------------------------------------------------------------------------------------------
def parsimony(codes, taxa, nodes):
    """(sites SITE_DTYPE, changes CHANGE_DTYPE) of the rows ``taxa`` of ``codes`` [R, W] on the tree ``nodes``."""
    c = np.asarray(codes, np.uint8)[np.asarray(taxa, np.int64)]
    n = len(c)
    sites, changes = [], []
    if len(nodes):
        for j in range(c.shape[1]):
            steps, alleles, _, ch = column(n, nodes, c[:, j])
            assert len(ch) == steps  # the first property of the spec
            if steps >= 1:
                sites.append((j, steps, alleles, 0))
            changes += [(j, w, p, f, t, 0) for w, p, f, t in ch]
    changes.sort(key=lambda r: (r[1], r[0]))
    return (np.array(sites, SITE_DTYPE) if sites else np.zeros(0, SITE_DTYPE)), (np.array(changes, CHANGE_DTYPE) if changes else np.zeros(0, CHANGE_DTYPE))


def of_codes(codes, min_compared: int = 1, nodes=None):
    """(taxa, nodes, sites, changes) of a code matrix on NJ's own tree, or on ``nodes``."""
    taxa, own = NJ.tree(codes, min_compared)
    nodes = own if nodes is None else nodes
    return (taxa, nodes, *parsimony(codes, taxa, nodes))


# ---- planted trees --------------------------------------------------------------------------------------------------------------------------
def bipartition(col) -> frozenset:
    """The two groups of taxa a column of two bases makes, as a frozenset of two frozensets."""
    first = frozenset(np.flatnonzero(np.asarray(col) == col[0]).tolist())
    return frozenset([first, frozenset(range(len(col))) - first])


def planted_homoplasy(rng, n: int):
    """(codes [n, W + 16], planted splits, the extra column, its two leaves): ``NJ.additive`` with branches of three or four columns
    and one more block of columns nobody mutates, but for its first: there two leaves on different sides of an inner branch hold the
    same other base.  One column moves every distance by less than half the shortest branch: the tree stays the planted one."""
    codes, planted, used, W = NJ.additive(rng, n, cols_per_branch=(3, 4))
    extra = np.tile(rng.integers(0, 4, 16).astype(np.uint8), (n, 1))
    side = sorted(planted, key=sorted)[int(rng.integers(0, len(planted)))]
    a, b = sorted(side)[0], sorted(frozenset(range(n)) - side)[-1]
    extra[[a, b], 0] = (int(extra[0, 0]) + 2) % 4  # (read before the store: every row holds the same base there)
    return np.concatenate([codes, extra], axis=1), planted, W, (a, b)


# ---- the two tables ---------------------------------------------------------------------------------------------------------------------------
def _gene_of(gene_lengths, col: int):
    """(gene, 0-based position, 0-based column among the real columns) of a matrix column."""
    first = real = 0
    for g, L in enumerate(gene_lengths):
        cols = -(-int(L) // 16) * 16
        if col < first + cols:
            assert col - first < L  # no site in padding
            return g, col - first, real + col - first
        first, real = first + cols, real + int(L)
    raise AssertionError("a column outside the matrix")


def homoplasy_lines(locus: str, gene_names, gene_lengths, sites) -> bytes:
    out = []
    for s in sites:
        g, pos, col = _gene_of(gene_lengths, int(s["column"]))
        held = bin(int(s["alleles"])).count("1")
        out.append(f"{locus}\t{gene_names[g]}\t{pos + 1}\t{col + 1}\t{held}\t{int(s['steps'])}\t{int(s['steps']) - (held - 1)}\n".encode())
    return b"".join(out)


def changes_lines(locus: str, names, taxa, nodes, gene_names, gene_lengths, changes) -> bytes:
    n = len(taxa)
    under = below(n, nodes)
    tip = lambda k: newick_name(names[int(taxa[k])])  # noqa: E731
    out = []
    for c in changes:
        v = int(c["node"])
        g, pos, col = _gene_of(gene_lengths, int(c["column"]))
        if v < n:
            who = [tip(v), tip(v), b".", b"1"]
        else:
            a, b = kids(nodes[v - n])[:2]
            who = [f"#{v - n + 1}".encode(), tip(min(under[a])), tip(min(under[b])), str(len(under[v])).encode()]
        out.append(b"\t".join([locus.encode(), *who, gene_names[g].encode(), str(pos + 1).encode(), str(col + 1).encode(), b"acgt"[int(c["from"])].to_bytes(1, "little"),
                               b"acgt"[int(c["to"])].to_bytes(1, "little")]) + b"\n")  # fmt: skip
    return b"".join(out)


def run_tsv(rows, min_compared=D.MIN_COMPARED) -> tuple[bytes, bytes]:
    """(the lines of the homoplasy table, those of the change table) of a ``LocusRows``, from its matrices alone."""
    homoplasy, changed = [], []
    for L in rows.loci():
        idx, mat = rows.locus_matrix(L)
        if len(idx) < 2:
            continue
        taxa, nodes, sites, changes = of_codes(D.unpack(mat), min_compared)
        g0, g1 = rows.locus_genes(L)
        genes, lengths = list(rows.db.genes.ids[g0:g1]), [int(x) for x in rows.db.genes.lengths[g0:g1]]
        homoplasy.append(homoplasy_lines(rows.db.loci.ids[L], genes, lengths, sites))
        changed.append(changes_lines(rows.db.loci.ids[L], [rows.ids[i] for i in idx], taxa, nodes, genes, lengths, changes))
    return b"".join(homoplasy), b"".join(changed)


# ---- kp_pars.h under g++ -------------------------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness() -> C.CDLL:
    from tests.harness_util import build_harness

    h = build_harness("pars_harness", "kp_pars.h")
    h.kpy_pars_host.restype = C.c_int64
    h.kpy_pars_tree_ok.restype = C.c_int32
    h.kpy_pars_step_planes.restype = C.c_int32
    h.kpy_pars_node_planes.restype = C.c_int64
    h.kpy_pars_node_planes.argtypes = [C.c_int64, C.c_int64]
    return h


def harness_parsimony(codes, taxa, nodes):
    """(sites, changes) through kp_pars_host: the header's plane-word pass over the packed rows."""
    codes = np.asarray(codes, np.uint8)
    blocks = np.ascontiguousarray(D.pack(codes).reshape(codes.shape[0], -1), np.uint64)
    taxa, nodes = np.ascontiguousarray(taxa, np.int32), np.ascontiguousarray(nodes, NJ.NODE_DTYPE)
    h = harness()
    ns, nc = C.c_int64(0), C.c_int64(0)
    call = lambda s, c, cs, cc: h.kpy_pars_host(_p(blocks), C.c_int64(blocks.shape[1]), _p(taxa), C.c_int32(len(taxa)), _p(nodes), C.c_int64(len(nodes)), s, C.c_int64(cs), c,  # noqa: E731
                                                C.c_int64(cc), C.byref(ns), C.byref(nc))  # fmt: skip
    assert call(None, None, 0, 0) == 0
    sites, changes = np.zeros(ns.value, SITE_DTYPE), np.zeros(nc.value, CHANGE_DTYPE)
    assert call(_p(sites), _p(changes), len(sites), len(changes)) == 0
    return sites, changes


def harness_tree_ok(n: int, nodes) -> bool:
    nd = np.ascontiguousarray(nodes, NJ.NODE_DTYPE)
    return bool(harness().kpy_pars_tree_ok(_p(nd), C.c_int64(len(nd)), C.c_int32(n)))
