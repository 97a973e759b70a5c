"""The pair reports on the device beyond three tiles of rows (kaptive_amd/csrc/kp_dist.hip, kp_dist_graph.hip, kp_dist_nj.hip) against
the scalable yardsticks of tests/pair_scale_util.py and tests/nj_util.py: bytes, no tolerance; the lengths of a neighbour-joining tree
are binary64, bit for bit.  The sizes are the last one that stays on a path and the first one that leaves it (pair_scale_util names
the constant each pair straddles; tests/test_pair_scale_cpu.py proves every label with the yardstick alone): 1024 / 1025 rows for the
one-block scan, 4096 / 4097 for the second 64-entry round of the row kernels, 16384 / 16385 / 16449 for their second grid trip,
512 / 513 taxa for the second trip of the lane fold and 1025 / 1026 for the row stride of the pick; then every union colliding, and
a ruler chain that takes every round of the tree.  Every handle runs its calls twice and a second handle runs them in reverse order:
the same bytes; ``device_allocations`` is what it was once the handles are closed."""

from __future__ import annotations

import numpy as np
import pytest

from kaptive_amd import _native
from tests import clusters_util as CU
from tests import distances_util as D
from tests import nj_util as NJ
from tests import pair_scale_util as P
from tests import tree_util as TU
from tests.distances_util import CH, SPLIT, T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _matrix(codes) -> np.ndarray:
    return D.pack(codes).reshape(codes.shape[0], -1)


def _bytes(x) -> bytes:
    return b"".join(np.ascontiguousarray(v).tobytes() for v in x) if isinstance(x, tuple) else x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes()


def _first_difference(got, want) -> str:
    for k, (g, w) in enumerate(zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,))):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape:
            return f"item {k}: shape {g.shape} on the device, {w.shape} wanted"
        if g.tobytes() != w.tobytes():
            at = np.argwhere(g != w)[0]
            return f"item {k} at {at.tolist()}: {g[tuple(at)]} on the device, {w[tuple(at)]} wanted ({int((g != w).sum())} differ)"
    return "equal"


def _run(ctx, codes, calls, handles=None):
    """``calls``: [(label, call(handle) -> arrays, wanted arrays)].  Every call twice on one handle and once, in reverse order, on a
    second: the same bytes each time, and the wanted ones."""
    before = _native.device_allocations()
    blocks = None if handles else _matrix(codes)
    one, two = handles or (_native.Distances(ctx, blocks), _native.Distances(ctx, blocks))
    try:
        first = []
        for label, call, want in calls:
            got = call(one)
            if callable(want):
                want = want()
            assert _bytes(got) == _bytes(want), f"{label}: {_first_difference(got, want)}"
            first.append(_bytes(got))
        for (label, call, _), seen in zip(calls, first):
            assert _bytes(call(one)) == seen, f"{label}: the second run on one handle"
        for (label, call, _), seen in reversed(list(zip(calls, first))):
            assert _bytes(call(two)) == seen, f"{label}: a second handle, the calls in reverse order"
    finally:
        if not handles:
            one.close()
            two.close()
    if not handles:
        assert _native.device_allocations() == before


def _listing(md, mc):
    return lambda d: d.pairs(md, mc)


def _count(md, mc):
    return lambda d: np.int64(d.count(md, mc))


def _report_calls(y, codes, nb, filters, level_sets, forest_mc, taxa=True):
    calls = []
    for md, mc in filters:
        calls.append((f"listing {md, mc}", _listing(md, mc), lambda md=md, mc=mc: y.pairs(md, mc)))
    for levels in level_sets:
        calls.append((f"clusters {levels}", lambda d, levels=levels: d.clusters(levels, 1), lambda levels=levels: y.clusters(levels, 1)))
    for mc in forest_mc:
        calls.append((f"forest {mc}", lambda d, mc=mc: d.tree(mc), lambda mc=mc: y.forest(mc)))
    if taxa:
        calls.append(("nj_taxa", lambda d: np.int64(d.nj_taxa(1)), np.int64(len(NJ.taxa_of(codes, 1)))))
    return calls


# ---- 1. the one-block scan with one and with two counts a lane ------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", P.BLOCKS_SCAN)
@pytest.mark.parametrize("R", P.SCAN)
def test_scan(ctx, R, nb):
    assert P.SCAN == (1024, 1025) and P.FILTERS == ((None, 0), (SPLIT, 0), (0, 0))
    codes, y = P.codes_of("mixed", R, nb), P.yard_of("mixed", R, nb)
    _run(ctx, codes, _report_calls(y, codes, nb, P.FILTERS, (CU.LEVELS, CU.EIGHT), (1, 16 * nb // 2)))


# ---- 2. the second 64-entry round of the row kernels: nt = 64 and 65 -------------------------------------------------------------------------
@pytest.mark.parametrize("nb", P.BLOCKS_ROUND)
@pytest.mark.parametrize("R", P.ROUND)
def test_round(ctx, R, nb):
    assert P.ROUND == (64 * T, 64 * T + 1) and P.BLOCKS_ROUND == (1, 4 * CH + 1)
    codes, y = P.codes_of("mixed", R, nb), P.yard_of("mixed", R, nb)
    filters = P.FILTERS if nb == 1 else P.FILTERS[1:]  # all R (R - 1) / 2 records once, at one block
    calls = _report_calls(y, codes, nb, filters, (CU.LEVELS, CU.EIGHT), (1, 16 * nb // 2))
    if nb != 1:
        calls.insert(0, ("count of all pairs", _count(None, 0), np.int64(R * (R - 1) // 2)))
    _run(ctx, codes, calls)


def test_round_with_pairs_in_the_last_tile_column_only(ctx):
    R, nb = P.ROUND[1], 5
    codes, y = P.codes_of("last_column", R, nb), P.yard_of("last_column", R, nb)
    calls = [(f"listing {f}", _listing(*f), lambda f=f: y.pairs(*f)) for f in ((0, 0), (SPLIT, 0), (1, 16 * nb))]
    calls.append(("count of all pairs", _count(None, 0), np.int64(R * (R - 1) // 2)))
    calls.append(("clusters", lambda d: d.clusters((0, 1, SPLIT), 1), lambda: y.clusters((0, 1, SPLIT), 1)))
    _run(ctx, codes, calls)


# ---- 3. the second grid trip of the row kernels ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=(*P.TRIP, P.TRIP_MORE))
def trip(ctx, request):
    """Two handles of a population of 16384, 16385 or 16449 rows, their planes built once for the tests below."""
    R = request.param
    assert P.TRIP == (16384, 16385) and P.TRIP_MORE == 16384 + T + 1
    before = _native.device_allocations()
    blocks = _matrix(P.codes_of("founders", R, 1))
    handles = _native.Distances(ctx, blocks), _native.Distances(ctx, blocks)
    yield R, handles
    for h in handles:
        h.close()
    assert _native.device_allocations() == before


def test_trip_counts_and_listings(ctx, trip):
    R, handles = trip
    codes, y = P.codes_of("founders", R, 1), P.yard_of("founders", R, 1)
    calls = [("count of all pairs", _count(None, 0), np.int64(R * (R - 1) // 2))]  # (their records are not asked for at this size)
    for md, mc in P.TRIP_FILTERS:
        calls.append((f"count {md, mc}", _count(md, mc), lambda md=md, mc=mc: np.int64(y.count(md, mc))))
        calls.append((f"listing {md, mc}", _listing(md, mc), lambda md=md, mc=mc: y.pairs(md, mc)))
    _run(ctx, codes, calls, handles)


def test_trip_clusters_and_nearest(ctx, trip):
    R, handles = trip
    codes, y = P.codes_of("founders", R, 1), P.yard_of("founders", R, 1)
    _run(ctx, codes, [("clusters", lambda d: d.clusters(P.TRIP_LEVELS, 1), lambda: y.clusters(P.TRIP_LEVELS, 1)),
                      ("nj_taxa", lambda d: np.int64(d.nj_taxa(1)), np.int64(len(NJ.taxa_of(codes, 1))))], handles)  # fmt: skip


def test_trip_forest_and_components(ctx, trip):
    R, handles = trip
    codes, y = P.codes_of("founders", R, 1), P.yard_of("founders", R, 1)
    _run(ctx, codes, [("forest", lambda d: d.tree(1), lambda: y.forest(1))], handles)
    assert 1 <= handles[0].tree_rounds() <= TU.harness().kpy_tree_max_rounds(R)


# ---- 4. neighbour joining: the second trip of the lane fold, the row stride of the pick ------------------------------------------------------
@pytest.mark.parametrize("n", (*P.FOLD, *P.PARTS))
def test_nj(ctx, n):
    assert P.FOLD == (512, 513) and P.PARTS == (1025, 1026) and P.BLOCKS_NJ == 4 * CH + 1
    codes = P.codes_of("taxa", n, P.BLOCKS_NJ)
    want = NJ.tree(codes, 1)
    assert len(want[0]) == n and len(want[1]) == n - 2
    assert (want[1][0]["a"], want[1][0]["b"]) == (n - 2, n - 1)  # the first join lies in the last row of the triangle: at 1026 taxa a row the pick reaches by its stride
    _run(ctx, codes, [("nj", lambda d: d.nj(1), want)])


def test_nj_of_identical_rows_ties_across_every_partial_and_both_trips(ctx):
    n = P.PARTS[1]
    codes = P.codes_of("copies", n, P.BLOCKS_NJ)
    want = NJ.tree(codes, 1)
    # the caterpillar of the tie rule (tests/test_gpu_nj.py): slots (0, 1) every time
    shape = [(0, 1, -1)] + [(n + r - 1, n - r, -1) for r in range(1, n - 3)] + [(2 * n - 4, 3, 2)]
    assert list(zip(want[1]["a"].tolist(), want[1]["b"].tolist(), want[1]["c"].tolist())) == shape and want[0].tolist() == list(range(n))
    assert not want[1]["la"].any() and not want[1]["lb"].any() and not want[1]["lc"].any() and not np.signbit(want[1]["la"]).any()
    _run(ctx, codes, [("nj", lambda d: d.nj(1), want)])


# ---- 5. contention: every union collides ------------------------------------------------------------------------------------------------------
def test_copies_of_one_row(ctx):
    R = P.ROUND[1]
    codes, y = P.codes_of("copies", R, 1), P.yard_of("copies", R, 1)
    calls = [(f"clusters {lv}", lambda d, lv=lv: d.clusters(lv, 1), lambda lv=lv: y.clusters(lv, 1)) for lv in (CU.EIGHT, (0,))]
    calls.append(("forest", lambda d: d.tree(1), lambda: y.forest(1)))
    calls.append(("count", _count(0, 1), np.int64(R * (R - 1) // 2)))
    _run(ctx, codes, calls)


def test_sixty_four_classes_in_every_tile(ctx):
    R, nb = P.ROUND[1], 5
    codes, y = P.codes_of("classes", R, nb), P.yard_of("classes", R, nb)
    calls = [(f"clusters {lv}", lambda d, lv=lv: d.clusters(lv, 1), lambda lv=lv: y.clusters(lv, 1)) for lv in (CU.EIGHT, (0, 16 * nb))]
    calls.append(("forest", lambda d: d.tree(1), lambda: y.forest(1)))
    calls.append(("listing", _listing(0, 1), lambda: y.pairs(0, 1)))
    _run(ctx, codes, calls)


# ---- 6. a ruler chain: every round of the tree, most tiles skipped after the first ones -----------------------------------------------------
@pytest.mark.parametrize("permuted", (False, True))
@pytest.mark.parametrize("R", P.ROUND)
def test_a_ruler_chain_takes_every_round(ctx, R, permuted):
    """tests/test_gpu_tree.py's chain at 4096 and 4097 rows: blocks of 2^k positions merge in pairs in round k + 1, so the run has
    floor(log2 R) = 12 rounds with edges and an empty one.  At 4096 rows that is the loop's bound; at 4097 the bound is one more."""
    chain, weights = P.ruler_chain(R)
    at = np.random.default_rng(32).permutation(R) if permuted else np.arange(R)  # chain position p lies in row at[p]
    codes = np.zeros_like(chain)
    codes[at] = chain
    a, b = np.minimum(at[:-1], at[1:]), np.maximum(at[:-1], at[1:])
    order = np.lexsort((b, a, weights))
    want = np.zeros(R - 1, P.PAIR_DTYPE)
    want["a"], want["b"] = a[order], b[order]
    want["compared"], want["differences"], want["unshared"] = P.counts_of(codes, want["a"], want["b"])
    assert want["differences"].tolist() == sorted(weights) and (want["compared"] == codes.shape[1]).all()
    bound = TU.harness().kpy_tree_max_rounds(R)
    assert R.bit_length() == 13 and bound == (13 if R == 4096 else 14)
    _run(ctx, codes, [("forest", lambda d: d.tree(1), (want, np.zeros(R, np.int32))),
                      ("rounds", lambda d: np.int64((d.tree(1), d.tree_rounds())[1]), np.int64(bound if R == 4096 else bound - 1))])  # fmt: skip
