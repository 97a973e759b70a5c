"""Pairwise locus distances between the isolates of a run (include/kp_spec.h, DISTANCES).

Every other report answers a question about one assembly; this one is about pairs: which isolates carry the same or nearly the same
locus, and how many bases apart they are.  ``LocusRows`` collects, batch after batch, one LOCUS ROW per assembly -- the aligned rows of
the primary kept records of its best locus's genes, strung together in database order, padding flagged -- and, when the run is over,
hands the rows of every locus to the device as one matrix (``_native.Distances``: kp_dist.hip compares them all against all; kp_dist_graph.hip, kp_dist_nj.hip, kp_dist_boot.hip, kp_dist_transfer.hip, kp_dist_pars.hip and kp_dist_sites.hip hold the reports below).  Two
tables come of a matrix: the listed pairs (``distances`` / ``tsv``) and, with no pair listed, every row's single-linkage cluster at a
few thresholds and its nearest neighbour (``clusters`` / ``clusters_tsv``; include/kp_spec.h, CLUSTERS), and the minimum spanning forest
of the rows as an edge table and as Newick text (``tree`` / ``tree_tsv`` / ``newick_tsv``; include/kp_spec.h, TREE), and the
neighbour-joining tree of the rows that hold most of the locus (``nj`` / ``nj_tsv``; include/kp_spec.h, NJ).  Another reads
the matrix by columns, not by pairs: the variable sites of a locus with every base's count, and the rows cut down to those sites
(``profile`` / ``sites`` / ``site_rows`` / ``sites_tsv`` / ``snp_alignment_tsv``; include/kp_spec.h, SITES).  The last puts those
columns on the neighbour-joining tree: on which branch a base changes, and which columns the tree cannot explain with one change per
base (``nj_parsimony`` / ``nj_changes_tsv`` / ``nj_homoplasy_tsv``; include/kp_spec.h, PARSIMONY).  One device handle
per locus serves them all: it is kept until the rows change or ``close()``.

It spans batches and, on a multi-GPU run, processes: ``state()`` is a picklable payload of what was added, ``merge()`` absorbs one.
"""

from __future__ import annotations

import numpy as np

from kaptive_amd import _native
from kaptive_amd.serotyping.batch import F_PRIMARY

GAP_BLOCK = np.uint64(0xFFFF << 48)  # sixteen GAP columns: a gene without a primary record, and what padding adds to a last block
DIST_RECORD_DTYPE = np.dtype([("locus", "<i4"), ("a", "<i4"), ("b", "<i4"), ("compared", "<i4"), ("differences", "<i4"), ("unshared", "<i4")])


SITE_RECORD_DTYPE = np.dtype([("locus", "<i4"), ("gene", "<i4"), ("position", "<i4"), ("column", "<i4"), ("n", "<i4", (4,)), ("n_n", "<i4")])


def clust_record_dtype(n_levels: int) -> np.dtype:
    """The records of ``LocusRows.clusters`` for ``n_levels`` levels: assembly numbers throughout, ``nearest`` -1 for none."""
    return np.dtype([("locus", "<i4"), ("assembly", "<i4"), ("labels", "<i4", (int(n_levels),)), ("nearest", "<i4"), ("compared", "<i4"),
                     ("differences", "<i4"), ("unshared", "<i4")])  # fmt: skip


def pad_masks(gene_lengths) -> np.ndarray:
    """uint64 per gene: the GAP bits of the columns at or beyond the gene's length in its last block (kp_dist_pad_mask)."""
    n = np.asarray(gene_lengths, np.int64) & 15
    return np.where(n > 0, ((0xFFFF << n) & 0xFFFF).astype(np.uint64) << np.uint64(48), np.uint64(0))


class LocusRows:
    """The locus rows of a run, for one database.

    ``add(bt)`` takes a ``BatchTyping`` of an engine made with ``aligned=True``; ``distances(ctx)`` / ``tsv(ctx)`` / ``matrix(ctx,
    locus)``, ``clusters(ctx)`` / ``clusters_tsv(ctx)``, ``tree(ctx)`` / ``tree_tsv(ctx)`` / ``newick_tsv(ctx)`` and ``nj(ctx, locus)`` / ``nj_tsv(ctx)`` compare them on the device of ``ctx`` (a ``_native.Context``; no database
    needs to be resident in it).  Assemblies are numbered in the order they were added.  A locus's matrix is uploaded once, by the
    first of these calls that needs it; ``close()`` -- or another ``add`` / ``merge`` -- frees the handles."""

    def __init__(self, db) -> None:
        self.db = db
        self.ids: list = []
        self.best = np.zeros(0, np.int32)
        self._parts: dict = {}  # locus -> [(assembly numbers int64 [k], matrix uint64 [k, NB])]
        self._handles: dict = {}  # locus -> _native.Distances of its matrix as it stands
        lengths = np.asarray(db.genes.lengths, np.int64)
        self._gene_blocks = (lengths + 15) // 16
        self._gene_pad = pad_masks(lengths)
        self._gene_lengths = lengths

    def __len__(self) -> int:
        return len(self.ids)

    # -- geometry of a locus -----------------------------------------------------------------------------------------------------
    def locus_genes(self, locus: int) -> tuple[int, int]:
        g0 = int(self.db.locus_gene_offsets[locus])
        return g0, g0 + int(self.db.locus_gene_lengths[locus])

    def n_blocks(self, locus: int) -> int:
        g0, g1 = self.locus_genes(locus)
        return int(self._gene_blocks[g0:g1].sum())

    def columns(self, locus: int) -> int:
        """The locus's total gene length: the table's ``Columns``."""
        g0, g1 = self.locus_genes(locus)
        return int(self._gene_lengths[g0:g1].sum())

    # -- building --------------------------------------------------------------------------------------------------------------------
    def rows_of(self, locus: int, members, n_kept, kept, rows, blocks) -> np.ndarray:
        """uint64 [len(members), NB]: the locus rows of assemblies ``members`` (indices into the batch's tables) for ``locus``."""
        members = np.asarray(members, np.int64)
        g0, g1 = self.locus_genes(locus)
        nbg = self._gene_blocks[g0:g1]
        first = np.concatenate([[0], np.cumsum(nbg)]).astype(np.int64)  # first block of every gene in the row
        nb = int(first[-1])
        mat = np.full((len(members), nb), GAP_BLOCK, np.uint64)
        if len(members) == 0 or nb == 0:
            return mat
        k = kept[members]
        live = (np.arange(kept.shape[1])[None, :] < np.asarray(n_kept)[members, None]) & ((k["flags"] & F_PRIMARY) != 0)
        live &= (k["gene"] >= g0) & (k["gene"] < g1)
        m, i = np.nonzero(live)  # member, kept index of every contributing record
        if len(m):
            gene = k["gene"][m, i].astype(np.int64) - g0
            r = rows[members[m], i]
            n = nbg[gene]
            ok = (r["gene_len"] == self._gene_lengths[g0 + gene]) & (r["off"] >= 0) & (r["off"] + n <= len(blocks))
            if not ok.all():
                raise ValueError("an aligned row does not have its gene's length, or lies outside the block array")
            # every block of every record: one gather, one scatter
            rec = np.repeat(np.arange(len(m)), n)
            within = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
            mat[m[rec], first[gene][rec] + within] = np.asarray(blocks, np.uint64)[r["off"][rec] + within]
        has = nbg > 0
        mat[:, (first[1:] - 1)[has]] |= self._gene_pad[g0:g1][has][None, :]
        return mat

    def add(self, bt) -> None:
        """The assemblies of one typed batch (``BatchTyping``; its engine must have been made with ``aligned=True``)."""
        self.close()
        rows, blocks = bt.aligned()
        n = len(bt.sums)
        base = len(self.ids)
        best = np.asarray(bt.best_locus, np.int32)
        for locus in np.unique(best):
            members = np.flatnonzero(best == locus)
            self._parts.setdefault(int(locus), []).append((members + base, self.rows_of(int(locus), members, bt.sums["n_kept"], bt.kept, rows, blocks)))
        self.ids.extend(bt.ids[:n])
        self.best = np.concatenate([self.best, best])

    def locus_matrix(self, locus: int) -> tuple[np.ndarray, np.ndarray]:
        """(assembly numbers int64 [R], matrix uint64 [R, NB]) of ``locus``, ascending in assembly number."""
        parts = self._parts.get(int(locus), [])
        if not parts:
            return np.zeros(0, np.int64), np.zeros((0, self.n_blocks(locus)), np.uint64)
        idx, mat = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        order = np.argsort(idx, kind="stable")
        self._parts[int(locus)] = [(idx[order], mat[order])]
        return self._parts[int(locus)][0]

    def loci(self) -> list:
        """The loci that have a row, in database order."""
        return sorted(self._parts)

    # -- across processes ------------------------------------------------------------------------------------------------------------
    def state(self) -> dict:
        """What was added, as plain picklable data (ids, best loci, per locus the assembly numbers and the matrix)."""
        return {"ids": list(self.ids), "best": self.best.copy(), "loci": {L: self.locus_matrix(L) for L in self.loci()}}

    def merge(self, state: dict) -> None:
        """Absorbs the ``state()`` of another accumulator of the same database: its assemblies follow the ones already here."""
        self.close()
        base = len(self.ids)
        for L, (idx, mat) in state["loci"].items():
            if mat.shape[1] != self.n_blocks(L):
                raise ValueError(f"locus {L}: rows of {mat.shape[1]} blocks, the database gives {self.n_blocks(L)}")
            self._parts.setdefault(int(L), []).append((np.asarray(idx, np.int64) + base, np.ascontiguousarray(mat, np.uint64)))
        self.ids.extend(state["ids"])
        self.best = np.concatenate([self.best, np.asarray(state["best"], np.int32)])

    # -- comparing -------------------------------------------------------------------------------------------------------------------
    def _handle(self, ctx, locus: int):
        """The device handle of ``locus``'s matrix on ``ctx``: made on first use, then shared by every table."""
        h = self._handles.get(int(locus))
        if h is None or h.ctx is not ctx or not h._h:
            if h is not None:
                h.close()
            h = self._handles[int(locus)] = _native.Distances(ctx, self.locus_matrix(locus)[1])
        return h

    def close(self) -> None:
        """Frees the device handles (the rows stay: a later call uploads them again)."""
        for h in self._handles.values():
            h.close()
        self._handles.clear()

    def _locus_pairs(self, ctx, locus: int, max_diff, min_compared):
        idx, mat = self.locus_matrix(locus)
        if len(idx) < 2:
            return idx, np.zeros(0, _native.DIST_PAIR_DTYPE)
        return idx, self._handle(ctx, locus).pairs(max_diff, min_compared)

    def _locus_clusters(self, ctx, locus: int, levels, min_compared):
        """(assembly numbers [R], labels int32 [K, R] as rows of the matrix, nearest records [R]) of one locus."""
        idx, mat = self.locus_matrix(locus)
        if len(idx) < 2:  # one row: its own cluster at every level, no neighbour
            near = np.zeros(len(idx), _native.DIST_NEAREST_DTYPE)
            near["row"] = -1
            return idx, np.zeros((len(_native.check_cluster_levels(levels)), len(idx)), np.int32), near
        return (idx, *self._handle(ctx, locus).clusters(levels, min_compared))

    def _locus_tree(self, ctx, locus: int, min_compared):
        """(assembly numbers [R], edges as rows of the matrix, component int32 [R]) of one locus."""
        idx, mat = self.locus_matrix(locus)
        if len(idx) < 2:  # one row: its own tree, no edge
            return idx, np.zeros(0, _native.DIST_PAIR_DTYPE), np.zeros(len(idx), np.int32)
        return (idx, *self._handle(ctx, locus).tree(min_compared))

    def _per_locus(self, table, empty):
        """``table(L)`` of every locus that has a row, in database order, joined; ``empty`` where there is none."""
        out = [table(L) for L in self.loci()]
        return empty if not out else b"".join(out) if isinstance(empty, bytes) else np.concatenate(out)

    @staticmethod
    def _pair_records(locus: int, idx, p) -> np.ndarray:
        """DIST_RECORD_DTYPE records of one locus's pair records ``p`` (rows of its matrix -> the assembly numbers ``idx``)."""
        rec = np.zeros(len(p), DIST_RECORD_DTYPE)
        rec["locus"] = locus
        rec["a"], rec["b"] = idx[p["a"]], idx[p["b"]]
        for f in ("compared", "differences", "unshared"):
            rec[f] = p[f]
        return rec

    def _pair_lines(self, locus: int, idx, p) -> bytes:
        return _native.format_distances(self.db.loci.ids[locus], self.columns(locus), [self.ids[i] for i in idx], p)

    def distances(self, ctx, max_diff: "int | None" = _native.DIST_MAX_DIFF, min_compared: int = _native.DIST_MIN_COMPARED) -> np.ndarray:
        """DIST_RECORD_DTYPE records ``(locus, a, b, compared, differences, unshared)`` of the listed pairs: loci in database order, one
        ``Distances`` handle each; a and b number the assemblies in the order they were added, a < b, ascending within a locus."""
        return self._per_locus(lambda L: self._pair_records(L, *self._locus_pairs(ctx, L, max_diff, min_compared)), np.zeros(0, DIST_RECORD_DTYPE))

    def tsv(self, ctx, max_diff: "int | None" = _native.DIST_MAX_DIFF, min_compared: int = _native.DIST_MIN_COMPARED) -> bytes:
        """The lines of the distance table (``--distances``; no header: ``_native.DISTANCES_HEADER``), formatted by the native library
        (kp_format_distances): loci in database order, pairs in input order with A before B."""
        return self._per_locus(lambda L: self._pair_lines(L, *self._locus_pairs(ctx, L, max_diff, min_compared)), b"")

    def clusters(self, ctx, levels=_native.CLUSTER_LEVELS, min_compared: int = _native.DIST_MIN_COMPARED) -> np.ndarray:
        """``clust_record_dtype(len(levels))`` records, one per assembly: loci in database order, assemblies in input order within a
        locus; ``labels[k]`` is the smallest assembly number of the assembly's cluster at ``levels[k]``, ``nearest`` the number of
        its nearest assembly (-1: none) with the pair's three counts."""
        dt = clust_record_dtype(len(_native.check_cluster_levels(levels)))

        def table(L):
            idx, labels, near = self._locus_clusters(ctx, L, levels, min_compared)
            rec = np.zeros(len(idx), dt)
            rec["locus"], rec["assembly"] = L, idx
            rec["labels"] = idx[labels].T
            rec["nearest"] = np.where(near["row"] >= 0, idx[np.maximum(near["row"], 0)], -1)
            for f in ("compared", "differences", "unshared"):
                rec[f] = near[f]
            return rec

        return self._per_locus(table, np.zeros(0, dt))

    def clusters_tsv(self, ctx, levels=_native.CLUSTER_LEVELS, min_compared: int = _native.DIST_MIN_COMPARED) -> bytes:
        """The lines of the cluster table (``--clusters``; no header: ``_native.clusters_header(levels)``), formatted by the native
        library (kp_format_clusters): loci in database order, a line per assembly in input order."""

        def table(L):
            idx, labels, near = self._locus_clusters(ctx, L, levels, min_compared)
            return _native.format_clusters(self.db.loci.ids[L], [self.ids[i] for i in idx], labels, near)

        return self._per_locus(table, b"")

    def tree(self, ctx, min_compared: int = _native.DIST_MIN_COMPARED) -> np.ndarray:
        """DIST_RECORD_DTYPE records ``(locus, a, b, compared, differences, unshared)`` of the edges of every locus's minimum spanning
        forest (include/kp_spec.h, TREE): loci in database order, a and b assembly numbers, a < b, ascending by (differences, a, b)
        within a locus."""
        return self._per_locus(lambda L: self._pair_records(L, *self._locus_tree(ctx, L, min_compared)[:2]), np.zeros(0, DIST_RECORD_DTYPE))

    def tree_tsv(self, ctx, min_compared: int = _native.DIST_MIN_COMPARED) -> bytes:
        """The lines of the edge table (``--mst``; no header: ``_native.DISTANCES_HEADER``, the columns of the distance table),
        formatted by the native library (kp_format_distances): loci in database order, edges in key order within a locus."""
        return self._per_locus(lambda L: self._pair_lines(L, *self._locus_tree(ctx, L, min_compared)[:2]), b"")

    def newick_tsv(self, ctx, min_compared: int = _native.DIST_MIN_COMPARED) -> bytes:
        """The lines of the Newick table (``--newick``; no header: ``_native.newick_header()``), formatted by the native library
        (kp_format_newick): loci in database order, a line per tree, ascending in the tree's first assembly."""

        def table(L):
            idx, p, comp = self._locus_tree(ctx, L, min_compared)
            return _native.format_newick(self.db.loci.ids[L], [self.ids[i] for i in idx], p, comp)

        return self._per_locus(table, b"")

    def nj(self, ctx, locus: int, min_compared: int = _native.DIST_MIN_COMPARED) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(assembly numbers [R], taxa int32 [n] as rows of the matrix, nodes ``_native.NJ_NODE_DTYPE``) of one locus's
        neighbour-joining tree (include/kp_spec.h, NJ): node ids below n index ``taxa``, the id n + r is the node record r made."""
        idx, mat = self.locus_matrix(locus)
        if len(idx) == 0:
            return idx, np.zeros(0, np.int32), np.zeros(0, _native.NJ_NODE_DTYPE)
        return (idx, *self._handle(ctx, locus).nj(min_compared))

    def nj_support(self, ctx, locus: int, replicates: int, seed: int = 1, min_compared: int = _native.DIST_MIN_COMPARED, transfer: bool = False):
        """(assembly numbers [R], taxa, nodes, support int32 [len(nodes)]) of one locus: ``nj``'s tree and the bootstrap support of
        every record out of ``replicates`` resamplings under ``seed`` (include/kp_spec.h, BOOTSTRAP), -1 for a record without an
        inner edge.  With ``transfer`` a fifth entry, int64 [len(nodes)]: the sums of the records' transfer distances
        (include/kp_spec.h, TRANSFER), and ``support`` is counted on exact sets by the same call."""
        idx, taxa, nodes = self.nj(ctx, locus, min_compared)
        if len(nodes) == 0:
            return (idx, taxa, nodes, np.zeros(0, np.int32), np.zeros(0, np.int64)) if transfer else (idx, taxa, nodes, np.zeros(0, np.int32))
        if transfer:
            return (idx, taxa, nodes, *self._handle(ctx, locus).nj_transfer(min_compared, nodes, replicates, seed))
        return idx, taxa, nodes, self._handle(ctx, locus).nj_support(min_compared, nodes, replicates, seed)

    def nj_tsv(self, ctx, min_compared: int = _native.DIST_MIN_COMPARED, bootstrap: int = 0, seed: int = 1, transfer: bool = False) -> tuple[bytes, list]:
        """(the lines of the neighbour-joining table, the loci that were skipped) (``--nj``; no header: ``_native.nj_header()``),
        formatted by the native library (kp_format_nj): loci in database order, a line for every locus with at least two taxa.  A
        locus of more than ``_native.NJ_MAX_TAXA`` taxa gets no line: its dense matrix is not built, and its number is returned.
        With ``bootstrap`` replicates (``--nj-bootstrap``; ``seed``: ``--nj-seed``) the lines carry support values
        (kp_format_nj_support; header: ``_native.nj_support_header()``); with ``transfer`` beside it (``--nj-transfer``) the labels
        are transfer support in three decimals (kp_format_nj_transfer; the same header)."""
        out, skipped = [], []
        for L in self.loci():
            idx, mat = self.locus_matrix(L)
            if len(idx) < 2:
                continue
            if self._handle(ctx, L).nj_taxa(min_compared) > _native.NJ_MAX_TAXA:
                skipped.append(L)
                continue
            names = [self.ids[i] for i in idx]
            if bootstrap and transfer:
                _, taxa, nodes, _, sums = self.nj_support(ctx, L, bootstrap, seed, min_compared, transfer=True)
                out.append(_native.format_nj_transfer(self.db.loci.ids[L], names, taxa, nodes, sums, bootstrap))
            elif bootstrap:
                _, taxa, nodes, support = self.nj_support(ctx, L, bootstrap, seed, min_compared)
                out.append(_native.format_nj_support(self.db.loci.ids[L], names, taxa, nodes, support, bootstrap))
            else:
                _, taxa, nodes = self.nj(ctx, L, min_compared)
                out.append(_native.format_nj(self.db.loci.ids[L], names, taxa, nodes))
        return b"".join(out), skipped

    def nj_parsimony(self, ctx, locus: int, min_compared: int = _native.DIST_MIN_COMPARED):
        """(assembly numbers [R], taxa, nodes, sites ``_native.PARS_SITE_DTYPE``, changes ``_native.PARS_CHANGE_DTYPE``) of one
        locus: ``nj``'s tree and small parsimony of every column of the locus's matrix on it (include/kp_spec.h, PARSIMONY) -- the
        columns the tree needs a change for, and every change by the child end of its branch.  Columns are those of the matrix,
        padding counted; states are relative to the last record, which is no root."""
        idx, taxa, nodes = self.nj(ctx, locus, min_compared)
        if len(nodes) == 0:
            return idx, taxa, nodes, np.zeros(0, _native.PARS_SITE_DTYPE), np.zeros(0, _native.PARS_CHANGE_DTYPE)
        return (idx, taxa, nodes, *self._handle(ctx, locus).nj_parsimony(min_compared, nodes))

    def _nj_parsimony_tsv(self, ctx, min_compared: int, lines) -> tuple[bytes, list]:
        """``lines(L, names, taxa, nodes, sites, changes)`` of every locus ``nj_tsv`` writes a line for, joined, and the loci skipped."""
        out, skipped = [], []
        for L in self.loci():
            idx, mat = self.locus_matrix(L)
            if len(idx) < 2:
                continue
            if self._handle(ctx, L).nj_taxa(min_compared) > _native.NJ_MAX_TAXA:
                skipped.append(L)
                continue
            _, taxa, nodes, sites, changes = self.nj_parsimony(ctx, L, min_compared)
            out.append(lines(L, [self.ids[i] for i in idx], taxa, nodes, sites, changes))
        return b"".join(out), skipped

    def nj_homoplasy_tsv(self, ctx, min_compared: int = _native.DIST_MIN_COMPARED) -> tuple[bytes, list]:
        """(the lines of the homoplasy table, the loci that were skipped) (``--nj-homoplasy``; no header:
        ``_native.nj_homoplasy_header()``), formatted by the native library (kp_format_nj_homoplasy): loci in database order -- those
        ``nj_tsv`` writes a tree for --, a line per column the locus's tree needs a change for, in column order."""

        def lines(L, names, taxa, nodes, sites, changes):
            g0, g1 = self.locus_genes(L)
            return _native.format_nj_homoplasy(self.db.loci.ids[L], list(self.db.genes.ids[g0:g1]), self._gene_lengths[g0:g1], sites)

        return self._nj_parsimony_tsv(ctx, min_compared, lines)

    def nj_changes_tsv(self, ctx, min_compared: int = _native.DIST_MIN_COMPARED) -> tuple[bytes, list]:
        """(the lines of the change table, the loci that were skipped) (``--nj-changes``; no header: ``_native.nj_changes_header()``),
        formatted by the native library (kp_format_nj_changes): loci in database order -- those ``nj_tsv`` writes a tree for --, a
        line per change, by (node, column)."""

        def lines(L, names, taxa, nodes, sites, changes):
            g0, g1 = self.locus_genes(L)
            return _native.format_nj_changes(self.db.loci.ids[L], names, taxa, nodes, list(self.db.genes.ids[g0:g1]), self._gene_lengths[g0:g1], changes)

        return self._nj_parsimony_tsv(ctx, min_compared, lines)

    # -- sites: the matrix by columns ---------------------------------------------------------------------------------------------------
    def profile(self, ctx, locus: int) -> np.ndarray:
        """``_native.SITE_DTYPE`` records of every column of ``locus``'s matrix, padding columns included: how many of its rows hold
        a, c, g, t and N there.  Fewer than two rows: counted here, without a device call."""
        idx, mat = self.locus_matrix(locus)
        if len(idx) >= 2:
            return self._handle(ctx, locus).profile()
        out = np.zeros(16 * mat.shape[1], _native.SITE_DTYPE)
        out["column"] = np.arange(len(out))
        for row in mat:
            j = np.arange(16, dtype=np.uint64)
            n, gap = ((row[:, None] >> (j + np.uint64(32))) & np.uint64(1)).ravel() != 0, ((row[:, None] >> (j + np.uint64(48))) & np.uint64(1)).ravel() != 0
            code = ((row[:, None] >> (2 * j)) & np.uint64(3)).ravel().astype(np.int64)
            base = ~n & ~gap
            out["n"][np.flatnonzero(base), code[base]] += 1
            out["n_n"] += n & ~gap
        return out

    def _locus_sites(self, ctx, locus: int, core: bool, rows: bool = False):
        """(assembly numbers [R], site records of the matrix, site rows uint64 [R, (S + 15) // 16] or None) of one locus."""
        idx, mat = self.locus_matrix(locus)
        if len(idx) < 2:  # one row differs from nobody: no site, rows of 0 blocks
            return idx, np.zeros(0, _native.SITE_DTYPE), np.zeros((len(idx), 0), np.uint64) if rows else None
        h = self._handle(ctx, locus)
        sites = h.sites(core)
        return idx, sites, h.site_rows() if rows else None

    def _site_genes(self, locus: int, columns):
        """(gene of the locus, 0-based position in it) of matrix columns of ``locus``."""
        g0, g1 = self.locus_genes(locus)
        first = np.concatenate([[0], np.cumsum(self._gene_blocks[g0:g1])]).astype(np.int64) * 16
        gene = np.searchsorted(first, np.asarray(columns, np.int64), side="right") - 1
        return gene, np.asarray(columns, np.int64) - first[gene]

    def sites(self, ctx, core: bool = False) -> np.ndarray:
        """SITE_RECORD_DTYPE records ``(locus, gene, position, column, n[4], n_n)`` of the variable sites: loci in database order,
        sites ascending within a locus.  ``gene`` is the database's gene index, ``position`` 0-based in it, ``column`` 0-based in the
        locus's genes strung together without padding; ``n`` the rows that hold a, c, g, t there and ``n_n`` those that hold an N."""

        def table(L):
            _, s, _ = self._locus_sites(ctx, L, core)
            g0, g1 = self.locus_genes(L)
            gene, pos = self._site_genes(L, s["column"])
            rec = np.zeros(len(s), SITE_RECORD_DTYPE)
            rec["locus"], rec["gene"], rec["position"] = L, g0 + gene, pos
            rec["column"] = np.concatenate([[0], np.cumsum(self._gene_lengths[g0:g1])])[gene] + pos
            rec["n"], rec["n_n"] = s["n"], s["n_n"]
            return rec

        return self._per_locus(table, np.zeros(0, SITE_RECORD_DTYPE))

    def site_rows(self, ctx, locus: int, core: bool = False) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(assembly numbers [R], site records of the matrix [S], site rows uint64 [R, (S + 15) // 16]) of one locus: every row cut
        down to the locus's sites, in the packed form of the rows themselves -- a matrix ``_native.Distances`` takes."""
        return self._locus_sites(ctx, locus, core, rows=True)

    def sites_tsv(self, ctx, core: bool = False) -> bytes:
        """The lines of the site table (``--sites``; no header: ``_native.SITES_HEADER``), formatted by the native library
        (kp_format_sites): loci in database order, a line per site in column order."""

        def table(L):
            idx, s, _ = self._locus_sites(ctx, L, core)
            g0, g1 = self.locus_genes(L)
            return _native.format_sites(self.db.loci.ids[L], list(self.db.genes.ids[g0:g1]), self._gene_lengths[g0:g1], len(idx), s)

        return self._per_locus(table, b"")

    def snp_alignment_tsv(self, ctx, core: bool = False) -> bytes:
        """The lines of the SNP alignment (``--snp-alignment``; no header: ``_native.SNP_ALIGNMENT_HEADER``), formatted by the native
        library (kp_format_site_rows): loci in database order, a line per assembly in input order; a locus without a site has none."""

        def table(L):
            idx, s, blocks = self._locus_sites(ctx, L, core, rows=True)
            return _native.format_site_rows(self.db.loci.ids[L], [self.ids[i] for i in idx], len(s), blocks)

        return self._per_locus(table, b"")

    def matrix(self, ctx, locus: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(assembly numbers [R], differences int32 [R, R], compared int32 [R, R]) of one locus, dense and symmetric, for small R."""
        idx, p = self._locus_pairs(ctx, locus, None, 0)
        R = len(idx)
        diff, comp = np.zeros((R, R), np.int32), np.zeros((R, R), np.int32)
        diff[p["a"], p["b"]] = diff[p["b"], p["a"]] = p["differences"]
        comp[p["a"], p["b"]] = comp[p["b"], p["a"]] = p["compared"]
        return idx, diff, comp
