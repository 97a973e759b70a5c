"""Yardsticks of the pair reports that scale to thousands of rows (include/kp_spec.h, DISTANCES, CLUSTERS, TREE): NumPy only, nothing
shared with kaptive_amd/csrc or kaptive_amd/distances.py, and nothing with the plain restatements either (tests/distances_util.py,
clusters_util.py, tree_util.py append a Python tuple per pair and loop over edges; tests/test_pair_scale_cpu.py proves the two sets
equal in bytes wherever the plain ones can follow).  The counts are matrix products of indicator matrices in float32 -- exact below
2^24 columns --, taken in row blocks; the listing is the upper triangle in row-major order; a level's labels are minimum-label
propagation with pointer jumping over the thresholded adjacency; the nearest partner is a row-wise argmin of (differences, partner);
the forest is Prim's algorithm under the full key (differences, a, b), one component after another -- the order is strict and total,
so the minimum spanning forest is unique and every correct algorithm returns this edge set.

Below the yardsticks: the constants of the device code that the sizes of the scale cases straddle (tests/test_pair_scale_cpu.py reads
them out of the sources and fails when a mirror is stale), the sizes, and the populations both modules use."""

from __future__ import annotations

import numpy as np

N, GAP = 4, 5
PAIR_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("compared", "<i4"), ("differences", "<i4"), ("unshared", "<i4"), ("pad", "<i4")])
NEAREST_DTYPE = np.dtype([("row", "<i4"), ("compared", "<i4"), ("differences", "<i4"), ("unshared", "<i4")])

# ---- the constants the sources must hold ------------------------------------------------------------------------------------------------
TILE = 64  # KP_DIST_TILE (kp_dist.h)
DIST_THREADS = 256  # kp_dist_handle.h
DIST_WAVES = DIST_THREADS // 64  # kp_dist.hip: rows of a workgroup of the row-sum and row-scan kernels
ROW_GRID = 4096  # kp_dist.hip: the literal of dist_grid(d->n_rows, DIST_WAVES, 4096)
GRID_CAP = 1 << 16  # kp_dist_handle.h: dist_grid's default cap
SCAN_THREADS = 1024  # kp_cigar.hip: lanes of the one-block scan
NJ_THREADS, NJ_MAX_PARTS, NJ_AHEAD, NJ_LANES = 256, 1024, 8, 64  # kp_dist_nj.hip, kp_nj.h
NJ_MAX_TAXA = 16384  # kp_caps.h

# ---- the sizes: the last one that stays on a path and the first one that leaves it ---------------------------------------------------------
SCAN = (SCAN_THREADS, SCAN_THREADS + 1)  # one count a lane of the one-block scan; two for the first lane
ROUND = (64 * TILE, 64 * TILE + 1)  # nt = 64: one 64-entry round of the row kernels; nt = 65: a second one of one entry
TRIP = (DIST_WAVES * ROW_GRID, DIST_WAVES * ROW_GRID + 1)  # every row wave owns one row; the first one owns two
TRIP_MORE = TRIP[0] + TILE + 1  # the second trip's rows fill a tile row and begin another: rows with listed pairs of their own
FOLD = (NJ_LANES * NJ_AHEAD, NJ_LANES * NJ_AHEAD + 1)  # one trip of nj_lane_fold; a second one for lane 0
PARTS = (NJ_MAX_PARTS + 1, NJ_MAX_PARTS + 2)  # m - 1 = NJ_MAX_PARTS rows of the triangle: a row a workgroup; one more: a second row for workgroup 0
MAX_ROWS = 1 << 18  # KP_DIST_MAX_ROWS (kp_caps.h)
WALK_NT = (ROUND[1] // TILE + 1, TRIP[1] // TILE + 1, MAX_ROWS // TILE)  # nt of 4097 rows, of 16385 rows and of the most rows: the grids tests/native_harness/dist_format_main.cpp walks tile by tile


def counts_of(codes, a, b, chunk: int = 1 << 22):
    """(compared, differences, unshared) int32 [E] of the pairs (a[e], b[e]), column by column."""
    codes, a, b = np.asarray(codes, np.uint8), np.asarray(a, np.int64), np.asarray(b, np.int64)
    out = np.zeros((3, len(a)), np.int32)
    step = max(1, chunk // max(codes.shape[1], 1))
    for e0 in range(0, len(a), step):
        x, y = codes[a[e0 : e0 + step]], codes[b[e0 : e0 + step]]
        both = (x < 4) & (y < 4)
        out[0, e0 : e0 + step] = both.sum(axis=1)
        out[1, e0 : e0 + step] = (both & (x != y)).sum(axis=1)
        out[2, e0 : e0 + step] = ((x == GAP) != (y == GAP)).sum(axis=1)
    return out[0], out[1], out[2]


class Yard:
    """The counts of all pairs of the rows of ``codes`` [R, W] in matrix form, and every report over them.  Two dense tables stay
    (compared, differences, in the narrowest unsigned type that holds W); ``unshared`` is computed for the pairs a report names."""

    def __init__(self, codes, block: int = 1024):
        codes = np.asarray(codes, np.uint8)
        self.codes, (self.R, self.W), self.block = codes, codes.shape, block
        R, W = codes.shape
        assert W < 1 << 16  # (float32 is exact below 2^24; the tables are uint16 at most)
        self.dtype = np.uint8 if W < 255 else np.uint16
        self.comp, self.diff = np.zeros((R, R), self.dtype), np.zeros((R, R), self.dtype)
        V = (codes < 4).astype(np.float32)
        X = [(codes == c).astype(np.float32) for c in range(4)]
        for a0 in range(0, R, block):
            a1 = min(a0 + block, R)
            compared = V[a0:a1] @ V.T
            same = X[0][a0:a1] @ X[0].T
            for c in range(1, 4):
                same += X[c][a0:a1] @ X[c].T
            self.comp[a0:a1] = compared
            self.diff[a0:a1] = compared - same
        self._present = (codes != GAP).astype(np.float32)
        self._n_present = self._present.sum(axis=1)
        self._edges = {}

    def _blocks(self):
        for a0 in range(0, self.R, self.block):
            yield a0, min(a0 + self.block, self.R)

    def _mc(self, min_compared) -> int:
        return min(max(int(min_compared), 0), self.W + 1)  # (within the tables' type; nothing compares W + 1 columns)

    def unshared_block(self, a0: int, a1: int) -> np.ndarray:
        """int32 [a1 - a0, R]: p_a + p_b - 2 P @ P.T of the rows a0 .. a1 - 1 against all."""
        P, p = self._present, self._n_present
        return (p[a0:a1, None] + p[None, :] - 2.0 * (P[a0:a1] @ P.T)).astype(np.int32)

    # ---- listing -----------------------------------------------------------------------------------------------------------------------
    def _listed(self, a0, a1, max_diff, min_compared):
        md = self.W if max_diff is None else min(int(max_diff), self.W)
        m = (self.diff[a0:a1] <= md) & (self.comp[a0:a1] >= self._mc(min_compared))
        return m & (np.arange(self.R)[None, :] > np.arange(a0, a1)[:, None])  # the upper triangle

    def count(self, max_diff=None, min_compared=0) -> int:
        return int(sum(int(self._listed(a0, a1, max_diff, min_compared).sum()) for a0, a1 in self._blocks()))

    def tile_counts(self, max_diff=None, min_compared=0) -> np.ndarray:
        """int64 [R, nt]: the listed pairs (a, b) of row a with b in tile column tj -- the entries of the device's count table."""
        nt = -(-self.R // TILE)
        out = np.zeros((self.R, nt), np.int64)
        for a0, a1 in self._blocks():
            m = self._listed(a0, a1, max_diff, min_compared)
            padded = np.zeros((a1 - a0, nt * TILE), bool)
            padded[:, : self.R] = m
            out[a0:a1] = padded.reshape(a1 - a0, nt, TILE).sum(axis=2)
        return out

    def pairs(self, max_diff=None, min_compared=0) -> np.ndarray:
        """PAIR_DTYPE records of the listed pairs, ascending (a, b)."""
        parts = []
        for a0, a1 in self._blocks():
            ra, rb = np.nonzero(self._listed(a0, a1, max_diff, min_compared))  # row-major: ascending (a, b)
            rec = np.zeros(len(ra), PAIR_DTYPE)
            rec["a"], rec["b"] = ra + a0, rb
            rec["compared"], rec["differences"] = self.comp[a0:a1][ra, rb], self.diff[a0:a1][ra, rb]
            if 8 * len(ra) > (a1 - a0) * self.R:
                rec["unshared"] = self.unshared_block(a0, a1)[ra, rb]
            elif len(ra):  # few pairs of the block are listed: theirs alone, column by column
                rec["unshared"] = counts_of(self.codes, rec["a"], rec["b"])[2]
            parts.append(rec)
        return np.concatenate(parts) if parts else np.zeros(0, PAIR_DTYPE)

    # ---- nearest partner ---------------------------------------------------------------------------------------------------------------
    def nearest(self, min_compared: int) -> np.ndarray:
        """NEAREST_DTYPE [R]: the row-wise argmin of (differences, partner) among compared >= min_compared; row -1 for none."""
        R, none = self.R, np.iinfo(np.int64).max
        out = np.zeros(R, NEAREST_DTYPE)
        out["row"] = -1
        cols = np.arange(R, dtype=np.int64)
        for a0, a1 in self._blocks():
            key = self.diff[a0:a1].astype(np.int64) * R + cols[None, :]
            key[self.comp[a0:a1] < self._mc(min_compared)] = none
            key[np.arange(a1 - a0), np.arange(a0, a1)] = none  # no row is its own partner
            at = key.argmin(axis=1)
            out["row"][a0:a1] = np.where(key[np.arange(a1 - a0), at] == none, -1, at)
        has = np.flatnonzero(out["row"] >= 0)
        c, d, u = counts_of(self.codes, has, out["row"][has])
        out["compared"][has], out["differences"][has], out["unshared"][has] = c, d, u
        return out

    # ---- labels --------------------------------------------------------------------------------------------------------------------------
    def _adjacency(self, limit: int, min_compared: int):
        """(src, dst, differences) of the thresholded adjacency in both directions, src ascending."""
        key = (int(limit), self._mc(min_compared))
        if key not in self._edges:
            src, dst, dif = [], [], []
            for a0, a1 in self._blocks():
                m = (self.diff[a0:a1] <= min(key[0], self.W)) & (self.comp[a0:a1] >= key[1])
                m[np.arange(a1 - a0), np.arange(a0, a1)] = False
                ra, rb = np.nonzero(m)
                src.append((ra + a0).astype(np.int32))
                dst.append(rb.astype(np.int32))
                dif.append(self.diff[a0:a1][ra, rb])
            self._edges = {key: (np.concatenate(src), np.concatenate(dst), np.concatenate(dif))} if src else {key: (np.zeros(0, np.int32),) * 3}
        return self._edges[key]

    def labels(self, levels, min_compared: int) -> np.ndarray:
        """int32 [K, R]: every row's label, the smallest row of its component under the edges of each level."""
        R = self.R
        out = np.zeros((len(levels), R), np.int32)
        if not len(levels) or R == 0:
            return out
        src, dst, dif = self._adjacency(max(levels), min_compared)
        for k, t in enumerate(levels):
            sel = dif <= t
            s, d = (src, dst) if sel.all() else (src[sel], dst[sel])
            lab = np.arange(R, dtype=np.int32)
            if len(s):
                first = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])  # the runs of one src
                rows = s[first]
                while True:
                    new = lab.copy()
                    new[rows] = np.minimum(new[rows], np.minimum.reduceat(lab[d], first))  # the smallest label among the neighbours
                    while True:  # pointer jumping: a label's own label
                        jump = new[new]
                        if (jump == new).all():
                            break
                        new = jump
                    if (new == lab).all():
                        break
                    lab = new
            out[k] = lab
        return out

    def clusters(self, levels, min_compared: int):
        return self.labels(levels, min_compared), self.nearest(min_compared)

    # ---- forest --------------------------------------------------------------------------------------------------------------------------
    def forest(self, min_compared: int):
        """(edges PAIR_DTYPE [E] ascending by (differences, a, b), component int32 [R]): Prim under the full key, a component after
        another, each begun at its smallest row."""
        R, none = self.R, np.iinfo(np.int64).max
        mc = self._mc(min_compared)
        rows = np.arange(R, dtype=np.int64)
        key = np.full(R, none, np.int64)  # of a row outside the tree: its lightest edge into the tree, differences * R^2 + a * R + b
        outside = np.ones(R, bool)
        component = np.zeros(R, np.int32)
        chosen, root = [], 0
        for _ in range(R):
            v = int(key.argmin())
            if key[v] == none:  # no edge leaves the tree: the next component begins at the smallest row left
                v = root = int(outside.argmax())
            else:
                chosen.append(int(key[v]))
            outside[v] = False
            key[v] = none
            component[v] = root
            offer = (self.diff[v].astype(np.int64) * R + np.minimum(rows, v)) * R + np.maximum(rows, v)
            better = outside & (self.comp[v] >= mc) & (offer < key)
            key[better] = offer[better]
        k = np.sort(np.array(chosen, np.int64))  # ascending by key
        edges = np.zeros(len(k), PAIR_DTYPE)
        edges["a"], edges["b"] = (k // R) % R, k % R
        edges["compared"], edges["differences"], edges["unshared"] = counts_of(self.codes, edges["a"], edges["b"])
        assert (edges["differences"] == k // (R * R)).all()
        return edges, component


# ---- populations -------------------------------------------------------------------------------------------------------------------------
def plant(codes, founders) -> None:
    """The planted rows of ``distances_util.population``, into ``codes`` in place: two identical rows, an all-GAP row, an all-N row,
    rows one column away from row 10 (column 0, either side of a plane-word edge and of a chunk edge, the last column; clipped to the
    last column of a short matrix) and a pair of complements."""
    cols = codes.shape[1]
    codes[1] = codes[0]
    codes[2] = GAP
    codes[3] = N
    codes[10] = founders[0]
    for r, c in zip(range(4, 10), (0, 63, 64, 64 * 8 - 1, 64 * 8, cols - 1)):
        c = min(c, cols - 1)
        codes[r] = codes[10]
        codes[r, c] = (codes[10, c] + 1) % 4
    codes[11] = founders[1]
    codes[12] = 3 - founders[1]


def many_founders(rng, R: int, nb: int = 1, n_founders: int = 256) -> np.ndarray:
    """Codes [R, 16 nb]: every row one of ``n_founders`` founders with 0..3 substitutions, one row in eight with an N and one in eight
    with a GAP column, the planted rows of ``plant``, and the last four rows identical.  A filter at or below 6 lists the relatives and a thin slice of the
    strangers, not all R (R - 1) / 2 pairs."""
    cols = 16 * nb
    founders = rng.integers(0, 4, (n_founders, cols)).astype(np.uint8)
    codes = founders[rng.integers(0, n_founders, R)].copy()
    k = rng.integers(0, 4, R)
    for j in range(3):
        hit = np.flatnonzero(k > j)
        at = rng.integers(0, cols, len(hit))
        codes[hit, at] = (codes[hit, at] + rng.integers(1, 4, len(hit))) % 4
    for code in (N, GAP):
        hit = np.flatnonzero(rng.random(R) < 0.125)
        codes[hit, rng.integers(0, cols, len(hit))] = code
    plant(codes, founders)
    codes[R - 3 :] = codes[R - 4]  # the last rows have listed pairs among themselves under every filter that keeps identical rows
    return codes


def last_column(rng, R: int, nb: int = 5) -> np.ndarray:
    """Codes [R, 16 nb] for R = 64 TILE + 1: rows 0..63 and the last row, the only one of the last tile column, are copies of one
    founder and every other row a stranger -- but for three: row 200 is the founder one column away (its only listed pair lies in
    the last tile column, and only under a max_diff of 1 or more), rows 300 and 310 are copies of a second founder (their pair lies
    in the first 64 tile columns, and row 300 has none in the last)."""
    cols = 16 * nb
    codes = rng.integers(0, 4, (R, cols)).astype(np.uint8)
    codes[:TILE] = codes[R - 1]
    codes[200] = codes[R - 1]
    codes[200, cols // 2] = (codes[200, cols // 2] + 1) % 4
    codes[310] = codes[300]
    return codes


def copies(rng, R: int, nb: int = 1) -> np.ndarray:
    """R copies of one row: every pair is an edge at every level, every union collides."""
    return np.tile(rng.integers(0, 4, 16 * nb).astype(np.uint8), (R, 1))


def classes(rng, R: int, nb: int = 5, n_classes: int = TILE) -> np.ndarray:
    """Row r is a copy of founder r % n_classes: every tile holds every class."""
    return rng.integers(0, 4, (n_classes, 16 * nb)).astype(np.uint8)[np.arange(R) % n_classes]


def taxa_only(rng, R: int, nb: int) -> np.ndarray:
    """Codes without N or GAP: mutated copies of three founders, every row a taxon of the neighbour-joining tree.  The last two rows
    are identical and strangers to all others, so the first join is the one pair of the last row of the triangle -- at
    NJ_MAX_PARTS + 2 taxa the row a workgroup of the pick reaches only by its stride."""
    cols = 16 * nb
    founders = rng.integers(0, 4, (3, cols)).astype(np.uint8)
    codes = founders[rng.integers(0, 3, R)].copy()
    for r in range(R):
        at = rng.integers(0, cols, int(rng.integers(0, 13)))
        codes[r, at] = (codes[r, at] + rng.integers(1, 4, len(at))) % 4
    codes[R - 2 :] = rng.integers(0, 4, cols).astype(np.uint8)  # two copies of a fourth founder: the first join, in the triangle's last row
    return codes


def ruler_chain(R: int):
    """(codes [R, W], weights [R - 1]): the chain of tests/test_gpu_tree.py at any length -- the edge between positions p and p + 1
    owns 1 + (trailing zeros of p + 1) columns of its own, in which every position beyond p differs from the founder.  W is the sum
    of the weights, up to a multiple of 16."""
    weights = [((p + 1) & -(p + 1)).bit_length() for p in range(R - 1)]
    W = -(-sum(weights) // 16) * 16
    founder = np.random.default_rng(31).integers(0, 4, W).astype(np.uint8)
    codes = np.tile(founder, (R, 1))
    at = 0
    for p, w in enumerate(weights):
        codes[p + 1 :, at : at + w] = (founder[at : at + w] + 1) % 4
        at += w
    return codes, weights


# ---- the cases both modules name -----------------------------------------------------------------------------------------------------------
BLOCKS_SCAN, BLOCKS_ROUND, BLOCKS_NJ = (1, 5), (1, 4 * 8 + 1), 4 * 8 + 1  # 4 CH + 1 blocks: a short last chunk, a short last plane word
FILTERS = ((None, 0), (6, 0), (0, 0))  # no limit; distances_util's SPLIT; identical in the compared columns
TRIP_FILTERS = ((0, 0), (3, 0), (6, 16))
TRIP_LEVELS = (0, 3, 6)
_made = {}


def codes_of(kind: str, R: int, nb: int) -> np.ndarray:
    """The population of a case, made once a process and left unchanged: ``mixed`` is ``distances_util.population``."""
    key = (kind, R, nb)
    if key not in _made:
        rng = np.random.default_rng([R, nb, sum(kind.encode())])
        if kind == "mixed":
            from tests.distances_util import population

            codes = population(rng, R, nb)
        else:
            codes = {"founders": many_founders, "last_column": last_column, "copies": copies, "classes": classes, "taxa": taxa_only}[kind](rng, R, nb)
        codes.setflags(write=False)
        _made[key] = codes
    return _made[key]


_yards = {}


def yard_of(kind: str, R: int, nb: int) -> Yard:
    """The yardstick of a case; the last two stay (both modules ask for a case's reports one after another)."""
    key = (kind, R, nb)
    if key not in _yards:
        while len(_yards) >= 2:
            _yards.pop(next(iter(_yards)))
        _yards[key] = Yard(codes_of(kind, R, nb))
    return _yards[key]
