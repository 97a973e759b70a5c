"""The scale cases of the pair reports, the parts that need no GPU (tests/test_gpu_pair_scale.py runs them on the device): the
scalable yardsticks of tests/pair_scale_util.py equal the plain restatements in bytes wherever those can follow; the constants the
sizes are derived from are the ones in the sources; and every case is what its label says, proved with the yardstick alone -- the
tile rows, the entries of the count table either side of the row kernels' second round, the taxa of the neighbour-joining cases, the
clusters every level set makes, the components of the forest.  tests/native_harness/dist_format_main.cpp, built and run here, walks
every tile of the grids of 4097, 16385 and 2^18 rows."""

from __future__ import annotations

import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import clusters_util as CU
from tests import distances_util as D
from tests import nj_util as NJ
from tests import pair_scale_util as P
from tests import tree_util as TU

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "kaptive_amd" / "csrc"
BLOCKS = (1, 5, 4 * D.CHUNK + 1)


def _int(pattern: str, text: str) -> int:
    m = re.search(pattern, text)
    assert m, pattern
    return int(eval(m.group(1), {"__builtins__": {}}))  # ("1 << 16" and the like)


# ---- 1. the constants and the sizes derived from them ------------------------------------------------------------------------------------
def test_the_sizes_come_from_the_constants_in_the_sources():
    handle, dist, cigar = (CSRC / "kp_dist_handle.h").read_text(), (CSRC / "kp_dist.hip").read_text(), (CSRC / "kp_cigar.hip").read_text()
    nj, nj_h, caps, dist_h = (CSRC / "kp_dist_nj.hip").read_text(), (CSRC / "kp_nj.h").read_text(), (CSRC / "kp_caps.h").read_text(), (CSRC / "kp_dist.h").read_text()
    threads = _int(r"constexpr int DIST_THREADS = (\d+);", handle)
    assert "constexpr int DIST_WAVES = DIST_THREADS / 64;" in dist
    waves = threads // 64
    row_grid = _int(r"dist_grid\(d->n_rows, DIST_WAVES, (\d+)\)", dist)
    cap = _int(r"inline unsigned dist_grid\(int64_t n, int per = DIST_THREADS, int64_t most = ([0-9 <]+)\)", handle)
    scan = _int(r"constexpr int SCAN_THREADS = (\d+);", cigar)
    m = re.search(r"constexpr int NJ_THREADS = (\d+), NJ_WAVES = NJ_THREADS / 64, NJ_MAX_PARTS = (\d+);", nj)
    nj_threads, parts = int(m.group(1)), int(m.group(2))
    ahead = _int(r"constexpr int AHEAD = (\d+);", nj)
    lanes = _int(r"#define KP_NJ_LANES (\d+)", nj_h)
    tile = _int(r"#define KP_DIST_TILE (\d+)", dist_h)
    max_taxa = _int(r"KP_NJ_MAX_TAXA = (\d+);", caps)
    max_rows = _int(r"KP_DIST_MAX_ROWS = ([0-9 <]+);", caps)
    assert (tile, threads, waves, row_grid, cap, scan) == (P.TILE, P.DIST_THREADS, P.DIST_WAVES, P.ROW_GRID, P.GRID_CAP, P.SCAN_THREADS)
    assert (nj_threads, parts, ahead, lanes, max_taxa, max_rows) == (P.NJ_THREADS, P.NJ_MAX_PARTS, P.NJ_AHEAD, P.NJ_LANES, P.NJ_MAX_TAXA, P.MAX_ROWS)
    assert tile == D.TILE == D.T and D.CH == D.CHUNK == 8 and max_rows == D.MAX_ROWS and max_taxa == NJ.MAX_TAXA
    # the loops the sizes straddle, as the sources write them: 64 entries a round, 64 * AHEAD entries a trip, a row a wave, a row a workgroup
    assert "for (int t = lane; t < nt; t += 64) sum += cnt[a * nt + t];" in dist and "for (int t0 = 0; t0 < nt; t0 += 64) {" in dist
    assert dist.count("a < R; a += (int64_t)gridDim.x * DIST_WAVES)") == 2
    assert "for (int32_t c0 = lane; c0 < m; c0 += 64 * AHEAD) {" in nj and "for (int32_t a = (int32_t)blockIdx.x; a < m - 1; a += (int32_t)gridDim.x) {" in nj
    assert "const int32_t parts = std::min<int32_t>(m - 1, NJ_MAX_PARTS);" in nj
    assert "const int64_t per = (n + SCAN_THREADS - 1) / SCAN_THREADS;" in cigar
    # the sizes
    assert P.SCAN == (scan, scan + 1) == (1024, 1025)  # per = 1, 2
    assert [-(-r // scan) for r in P.SCAN] == [1, 2]
    assert P.ROUND == (64 * tile, 64 * tile + 1) == (4096, 4097) and [-(-r // tile) for r in P.ROUND] == [64, 65]  # nt: one round of 64 entries, two
    assert P.TRIP == (waves * row_grid, waves * row_grid + 1) == (16384, 16385)
    assert [min(-(-r // waves), row_grid) * waves for r in P.TRIP] == [16384, 16384] and row_grid < cap  # the grid covers 16384 rows a trip
    assert P.FOLD == (lanes * ahead, lanes * ahead + 1) == (512, 513)
    assert P.PARTS == (parts + 1, parts + 2) == (1025, 1026)  # the first pick has m - 1 = 1024 and 1025 rows for at most 1024 workgroups
    assert max(P.TRIP) <= max_rows and max(P.PARTS) <= max_taxa
    assert P.WALK_NT == (65, 257, 4096) == (-(-P.ROUND[1] // tile), -(-P.TRIP[1] // tile), max_rows // tile)
    assert 4096 * 4097 // 2 == 8_390_656
    assert P.BLOCKS_ROUND == (1, 4 * D.CH + 1) and P.BLOCKS_NJ == 4 * D.CH + 1 and P.FILTERS == ((None, 0), (D.SPLIT, 0), (0, 0))
    assert P.PAIR_DTYPE == D.PAIR_DTYPE and P.NEAREST_DTYPE == CU.NEAREST_DTYPE and (P.N, P.GAP) == (D.N, D.GAP)


# ---- 2. the scalable yardsticks against the plain ones -------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", D.ROWS)
def test_yardsticks_equal_the_plain_restatements(R):
    for nb in BLOCKS:
        codes = D.population(np.random.default_rng([R, nb]), R, nb)
        every = D.all_pairs(codes)
        y = P.Yard(codes, block=50)  # (several row blocks at these sizes)
        for md, mc in (*P.FILTERS, *P.TRIP_FILTERS, (D.SPLIT, 16 * nb // 2)):
            want = every[(every["differences"] <= (10**9 if md is None else md)) & (every["compared"] >= mc)]
            got = y.pairs(md, mc)
            assert got.dtype == D.PAIR_DTYPE and got.tobytes() == want.tobytes() and y.count(md, mc) == len(want), (R, nb, md, mc)
            tiles = y.tile_counts(md, mc)
            assert tiles.shape == (R, -(-R // D.T)) and tiles.sum() == len(want)
            assert (tiles.sum(axis=1) == np.bincount(want["a"], minlength=R)).all() and (tiles.sum(axis=0) == np.bincount(want["b"] // D.T, minlength=tiles.shape[1])).all()
        for mc in (0, 1, 16 * nb // 2, 10**6):
            near = CU.nearest_of(R, every, mc)
            assert y.nearest(mc).tobytes() == near.tobytes(), (R, nb, mc)
            for levels in (CU.LEVELS, CU.EIGHT, P.TRIP_LEVELS, (D.SPLIT,), ()):
                assert y.labels(levels, mc).tobytes() == CU.labels_of(R, every, levels, mc).tobytes(), (R, nb, mc, levels)
            edges, comp = TU.forest_of(R, every, mc)
            got = y.forest(mc)
            assert got[0].tobytes() == edges.tobytes() and got[1].tobytes() == comp.tobytes(), (R, nb, mc)
        if R > 1:
            a, b = np.triu_indices(R, 1)
            c, d, u = P.counts_of(codes, a, b, chunk=1000)
            assert (c == every["compared"]).all() and (d == every["differences"]).all() and (u == every["unshared"]).all()


@pytest.mark.parametrize("make,R,nb", [(P.many_founders, 3 * D.T + 5, 1), (P.last_column, 64 * D.T + 1, 1), (P.copies, 2 * D.T + 1, 1), (P.classes, 3 * D.T + 5, 5),
                                       (P.taxa_only, D.T + 1, 5), (lambda rng, R, nb: P.ruler_chain(R)[0], 2 * D.T + 1, None)])  # fmt: skip
def test_yardsticks_on_the_populations_of_the_scale_cases(make, R, nb):
    codes = make(np.random.default_rng(9), R, nb)
    if make is P.last_column:  # (the population has its meaning at 4097 rows only: its first rows and a slice of the others)
        codes = codes[np.r_[0 : D.T, 190:320, R - 1]]
    R = codes.shape[0]
    y, every = P.Yard(codes, block=60), D.all_pairs(codes)
    assert y.pairs().tobytes() == every.tobytes()
    for mc in (0, 1, codes.shape[1]):
        assert y.labels(CU.EIGHT, mc).tobytes() == CU.labels_of(R, every, CU.EIGHT, mc).tobytes() and y.nearest(mc).tobytes() == CU.nearest_of(R, every, mc).tobytes()
        edges, comp = TU.forest_of(R, every, mc)
        got = y.forest(mc)
        assert got[0].tobytes() == edges.tobytes() and got[1].tobytes() == comp.tobytes()


def test_planted_rows_are_those_of_the_plain_population():
    """``plant`` restates what ``distances_util.population`` plants: on that population's own founders it changes nothing."""
    for nb in (1, 5, 33, 40):
        rng = np.random.default_rng(nb)
        codes = D.population(rng, 40, nb)
        again = codes.copy()
        again[[2, 3]] = 0
        again[4:10] = 1
        P.plant(again, np.stack([codes[10], codes[11]]))
        assert (again == codes).all()


# ---- 3. every case is what its label says ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", P.SCAN)
@pytest.mark.parametrize("nb", P.BLOCKS_SCAN)
def test_scan_cases(R, nb):
    codes, y = P.codes_of("mixed", R, nb), P.yard_of("mixed", R, nb)
    assert codes.shape == (R, 16 * nb) and -(-R // P.SCAN_THREADS) == (1 if R == P.SCAN[0] else 2)
    n = len(NJ.taxa_of(codes, 1))
    assert 0 < n < R  # the flag scan sees both values
    for md, mc in P.FILTERS:
        rows = y.tile_counts(md, mc).sum(axis=1)
        assert rows[0] > 0 and rows[1] > 0  # at 1025 rows the two counts of the scan's first lane
        assert (rows > 0).sum() > R // 2 and rows.sum() == y.count(md, mc)
    _levels_split(y, R)
    _forest_splits(y, R, nb)


def _levels_split(y, R, level_sets=(CU.LEVELS, CU.EIGHT)):
    for levels in level_sets:
        for k, row in enumerate(y.labels(levels, 1)):
            assert 1 < len(np.unique(row)) < R, (levels, k)


def _forest_splits(y, R, nb):
    for mc in (1, 16 * nb // 2):
        edges, comp = y.forest(mc)
        assert len(np.unique(comp)) > 1 and len(edges) == R - len(np.unique(comp))
    bases = (y.codes < 4).sum(axis=1)
    assert (bases < 16 * nb // 2).any()  # min_compared lies above some rows' coverage


@pytest.mark.parametrize("R", P.ROUND)
@pytest.mark.parametrize("nb", P.BLOCKS_ROUND)
def test_round_cases(R, nb):
    y = P.yard_of("mixed", R, nb)
    nt = -(-R // P.TILE)
    assert nt == (64 if R == P.ROUND[0] else 65) and nt * (nt + 1) // 2 == (2080 if nt == 64 else 2145)
    for md, mc in P.FILTERS:
        tiles = y.tile_counts(md, mc)
        assert tiles.shape == (R, nt)
        if nt == 65:  # some row of tile row 0 has listed pairs before and in tile column 64: the carry into the second round is not zero
            both = (tiles[: P.TILE, :64].sum(axis=1) > 0) & (tiles[: P.TILE, 64] > 0)
            assert both.any(), (md, mc)
    if nb == 1:
        assert y.count(None, 0) == R * (R - 1) // 2 == (8_386_560 if R == 4096 else 8_390_656)
    _levels_split(y, R)
    _forest_splits(y, R, nb)


def test_last_column_case():
    R, nb = P.ROUND[1], 5
    y = P.yard_of("last_column", R, nb)
    exact, near = y.tile_counts(0, 0), y.tile_counts(D.SPLIT, 0)
    # (0, 0): every pair inside tile row 0 and of tile row 0 with the last tile column is listed, and rows 300 and 310; nothing else
    want = np.zeros_like(exact)
    want[: P.TILE, 0] = np.arange(P.TILE - 1, -1, -1)
    want[: P.TILE, 64] = 1
    want[300, 310 // P.TILE] = 1
    assert (exact == want).all() and y.count(0, 0) == 64 * 63 // 2 + 64 + 1
    for a in range(P.TILE):  # the only entries of those rows that are not zero are the first and the 65th
        assert np.flatnonzero(exact[a]).tolist() == ([0, 64] if a < P.TILE - 1 else [64])
    # at the last round: the first 64 entries more than zero and entry 64 zero; and the other way round
    assert exact[300, :64].sum() > 0 and exact[300, 64] == 0
    assert near[200, :64].sum() == 0 and near[200, 64] == 1 and exact[200].sum() == 0
    assert (near - exact).sum() == P.TILE + 1 and y.count(D.SPLIT, 0) == y.count(0, 0) + P.TILE + 1  # row 200 with the founder's copies


@pytest.mark.parametrize("R", P.TRIP)
def test_trip_cases(R):
    codes, y = P.codes_of("founders", R, 1), P.yard_of("founders", R, 1)
    assert codes.shape == (R, 16) and -(-R // P.DIST_WAVES) == (P.ROW_GRID if R == P.TRIP[0] else P.ROW_GRID + 1)
    assert (codes[1] == codes[0]).all() and (codes[2] == P.GAP).all() and (codes[3] == P.N).all() and (codes[11] + codes[12] == 3).all()
    assert [int((codes[r] != codes[10]).sum()) for r in range(4, 10)] == [1] * 6
    for md, mc in P.TRIP_FILTERS:
        n = y.count(md, mc)
        assert 10_000 < n < 1_000_000, (md, mc, n)  # a listing to compare, not all 134 M pairs
        if R == P.TRIP[1] and md == 6:
            tiles = y.tile_counts(md, mc)
            assert tiles[P.TRIP[0] :].sum() == 0 and tiles[:, -1].sum() > 0  # the row of the second trip is the last: its pairs are other rows' records
    assert y.count(6, 16) < y.count(6, 0)  # min_compared drops the rows with an N or a GAP column
    _levels_split(y, R, (P.TRIP_LEVELS,))
    edges, comp = y.forest(1)
    assert 1 < len(np.unique(comp)) < 10 and len(edges) == R - len(np.unique(comp))


def test_trip_case_whose_second_trip_rows_have_pairs():
    """At 16385 rows the one row of the second trip is the last and lists nothing.  At 16449 the second trip's rows fill a tile row
    and begin another, and the last four are identical: rows of the second trip with records of their own."""
    R = P.TRIP_MORE
    y = P.yard_of("founders", R, 1)
    assert R == P.TRIP[0] + P.TILE + 1 == 16449 and -(-R // P.TILE) == 258
    for md, mc in P.TRIP_FILTERS[:2]:
        tiles = y.tile_counts(md, mc)
        assert tiles[R - 4, 256] >= 2 and tiles[R - 4, 257] == 1 and tiles[P.TRIP[0] :, :256].sum() == 0
        assert (tiles[P.TRIP[0] :, 256:].sum(axis=0) > 0).all()  # in both of their tile columns


@pytest.mark.parametrize("R", (*P.FOLD, *P.PARTS))
def test_nj_cases_have_the_taxa_of_their_labels(R):
    codes = P.codes_of("taxa", R, P.BLOCKS_NJ)
    taxa = NJ.taxa_of(codes, 1)
    assert len(taxa) == R and R in (512, 513, 1025, 1026)
    # the first pick: the smallest (Q, a, b) is the one pair of the triangle's last row -- at 1026 taxa row 1024, the second row of workgroup 0
    d = NJ.matrix_of(codes, taxa)
    s = NJ.sum64(d)
    q = ((np.float64(R - 2) * d) - s[:, None]) - s[None, :]
    q[np.tril_indices(R)] = np.inf
    assert divmod(int(np.argmin(q)), R) == (R - 2, R - 1) and (np.sort(q, axis=None)[1] > q[R - 2, R - 1])
    same = P.codes_of("copies", P.PARTS[1], P.BLOCKS_NJ)
    assert len(NJ.taxa_of(same, 1)) == P.PARTS[1] == 1026 and (same == same[0]).all()


def test_contention_cases():
    R = P.ROUND[1]
    y = P.yard_of("copies", R, 1)
    assert y.count(0, 1) == R * (R - 1) // 2 and not y.labels(CU.EIGHT, 1).any()
    near = y.nearest(1)
    assert near["row"].tolist() == [1] + [0] * (R - 1)
    edges, comp = y.forest(1)
    assert edges["a"].tolist() == [0] * (R - 1) and edges["b"].tolist() == list(range(1, R)) and not comp.any()  # the star of row 0
    y = P.yard_of("classes", R, 5)
    labels = y.labels(CU.EIGHT, 1)
    assert (labels[0] == np.arange(R) % P.TILE).all()  # level 0: the 64 classes, each under its first row
    for ti in range(R // P.TILE):  # every tile holds every class
        assert sorted(labels[0, ti * P.TILE : (ti + 1) * P.TILE].tolist()) == list(range(P.TILE))
    edges, comp = y.forest(1)
    zero = edges[edges["differences"] == 0]
    assert len(zero) == R - P.TILE and (zero["a"] == zero["b"] % P.TILE).all() and (zero["a"] < P.TILE).all()  # 64 stars
    rest = edges[edges["differences"] > 0]
    assert len(rest) == P.TILE - 1 and (rest["b"] < P.TILE).all() and not comp.any()  # the founders' tree joins them at each class's first row


def test_ruler_chain_case():
    for R in P.ROUND:
        codes, weights = P.ruler_chain(R)
        assert codes.shape[0] == R and codes.shape[1] % 16 == 0 and 16 * (codes.shape[1] // 16) < TU.MAX_COLUMNS
        c, d, u = P.counts_of(codes, np.arange(R - 1), np.arange(1, R))
        assert d.tolist() == weights and (c == codes.shape[1]).all() and not u.any()
        rng = np.random.default_rng(R)
        p, q = np.sort(rng.integers(0, R, (2, 500)), axis=0)
        cum = np.r_[0, np.cumsum(weights)]
        assert (P.counts_of(codes, p, q)[1] == cum[q] - cum[p]).all()  # positions p < q differ in the columns of the edges between them
        assert TU.harness().kpy_tree_max_rounds(R) == (13 if R == 4096 else 14) and R.bit_length() == 13


# ---- 4. the tile index at every tile of the large grids ------------------------------------------------------------------------------------
def test_stand_alone_program_walks_every_tile(tmp_path):
    exe = tmp_path / "dist_format_main"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", str(exe), str(ROOT / "tests" / "native_harness" / "dist_format_main.cpp"), str(CSRC / "kp_rows.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    for nt in P.WALK_NT:
        assert f"tiles of nt {nt}: {nt * (nt + 1) // 2} walked" in r.stdout
