"""The minimum spanning forest of locus rows on the device (include/kp_spec.h, TREE; kaptive_amd/csrc/kp_dist_graph.hip) against Kruskal in
tests/tree_util.py: integers, order and bytes, exactly.  Random populations at every shape at which the epilogue takes another path;
identical rows, where every key ties on differences and only (a, b) decides; a chain whose components merge in pairs, so that the
rounds run as long as rounds can; two rows, whose one edge both sides choose; the two properties that tie the forest to CLUSTERS;
the state the call must leave alone; its refusals; then the whole route on the 9-locus miniature database: ``Serotyper(db,
distances=True)`` over two batches, the command line with ``--mst``, with ``--newick``, with both beside ``--distances --clusters``
and with ``--db``, a run without the flags, and two devices."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from tests import clusters_util as CU
from tests import distances_util as D
from tests.distances_util import CH, ROWS, SPLIT, T, Run, _count_handles, _device_count, _write_inputs
from tests import tree_util as TU

pytestmark = pytest.mark.gpu

BLOCKS = (1, 4, 4 * CH, 4 * CH + 1, 8 * CH + 3)
EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _matrix(codes) -> np.ndarray:
    return D.pack(codes).reshape(codes.shape[0], -1) if codes.shape[0] else np.zeros((0, codes.shape[1] // 16), np.uint64)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _same(got, want, what):
    (ge, gc), (we, wc) = got, want
    assert ge.dtype == _native.DIST_PAIR_DTYPE and gc.dtype == np.int32 and gc.shape == wc.shape, what
    if gc.tobytes() != wc.tobytes():
        r = int(np.flatnonzero(gc != wc)[0])
        raise AssertionError(f"{what}: component of row {r}: {gc[r]} on the device, {wc[r]} wanted ({int((gc != wc).sum())} differ)")
    if ge.tobytes() != we.tobytes():
        i = next((i for i in range(min(len(ge), len(we))) if ge[i] != we[i]), min(len(ge), len(we)))
        raise AssertionError(f"{what}: {len(ge)} edges on the device, {len(we)} wanted; edge {i}: {ge[i] if i < len(ge) else None} against {we[i] if i < len(we) else None}")


# ---- 1. random populations: every shape, every min_compared ------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
def test_forest_against_kruskal(ctx, R):
    for nb in BLOCKS:
        codes = D.population(np.random.default_rng([R, nb]), R, nb)
        every = D.all_pairs(codes)  # the reference's pairs, once: every min_compared selects from them
        first = {}
        with _native.Distances(ctx, _matrix(codes)) as d:
            for mc in (0, 1, 16 * nb // 2):
                want = TU.forest_of(R, every, mc)
                got = d.tree(mc)
                _same(got, want, f"R {R}, NB {nb}, min_compared {mc}")
                assert len(got[0]) == R - len(set(got[1].tolist())) and (got[1] <= np.arange(R)).all()
                assert R < 2 or 1 <= d.tree_rounds() <= R.bit_length()  # (n components at least halve: floor(log2 n) rounds with edges and an empty one)
                first[mc] = got[0].tobytes() + got[1].tobytes()
            if R >= T - 1:
                edges, comp = d.tree(1)  # all GAP, all N: nothing compared, trees of their own
                assert comp[2] == 2 and comp[3] == 3 and not np.isin(edges["a"], (2, 3)).any() and not np.isin(edges["b"], (2, 3)).any()
                edges, comp = d.tree(0)  # ... and 0 differences from every row: hubs that carry one tree of 0-edges
                assert not comp.any() and len(edges) == R - 1 and not edges["differences"].any() and (0, 2) in set(zip(edges["a"].tolist(), edges["b"].tolist()))
        with _native.Distances(ctx, _matrix(codes)) as again:  # a second handle, the calls in another order: the same bytes
            for mc in reversed(list(first)):
                got = again.tree(mc)
                assert got[0].tobytes() + got[1].tobytes() == first[mc], mc


# ---- 2. every row identical: all keys tie on differences ---------------------------------------------------------------------------------
def test_identical_rows_give_the_star_of_row_0(ctx):
    R, nb = 3 * T + 5, 4 * CH + 1
    codes = np.tile(np.random.default_rng(21).integers(0, 4, 16 * nb).astype(np.uint8), (R, 1))
    with _native.Distances(ctx, _matrix(codes)) as d:
        edges, comp = d.tree(1)
        assert d.tree_rounds() == 2  # every row chooses (0, r), row 0 chooses (0, 1): one round of edges, one empty
    assert edges["a"].tolist() == [0] * (R - 1) and edges["b"].tolist() == list(range(1, R)) and not comp.any()  # a tie broken by tile or lane order fails here
    assert not edges["differences"].any() and (edges["compared"] == 16 * nb).all() and not edges["unshared"].any() and not edges["pad"].any()
    _same((edges, comp), TU.forest(codes, 1), "identical rows")


# ---- 3. a chain whose edges weigh as the ruler sequence --------------------------------------------------------------------------------------
def _ruler_chain(R, nb):
    """Codes [R, 16 nb] of a chain: the edge between positions p and p + 1 owns 1 + (trailing zeros of p + 1) columns of its own, in
    which every position beyond p differs from the founder -- so positions p < q differ in the columns of the edges between them."""
    founder = np.random.default_rng(31).integers(0, 4, 16 * nb).astype(np.uint8)
    codes = np.tile(founder, (R, 1))
    weights = [1 + ((p + 1) & -(p + 1)).bit_length() - 1 for p in range(R - 1)]
    assert sum(weights) <= 16 * nb
    at = 0
    for p, w in enumerate(weights):
        codes[p + 1 :, at : at + w] = (founder[at : at + w] + 1) % 4
        at += w
    return codes, weights


@pytest.mark.parametrize("permuted", (False, True))
@pytest.mark.parametrize("R", (3 * T + 5, 2 * T))
def test_a_ruler_chain_takes_every_round(ctx, R, permuted):
    """Blocks of 2^k consecutive positions merge in pairs in round k + 1 (a block's two ways out weigh k + 1 and more than k + 1), so
    the run has floor(log2 R) rounds with edges and an empty one.  At R = 2 T, a power of two, that is the loop's bound itself: a
    loop that stops a round early, or a bound one too small, fails there.  (At R = 3 T + 5 the last, short block joins its
    neighbour a round early, as the tail of any R that is no power of two does: one round fewer than the bound.)"""
    nb = 4 * CH + 1
    chain, weights = _ruler_chain(R, nb)
    at = np.random.default_rng(32).permutation(R) if permuted else np.arange(R)  # chain position p lies in row at[p]
    codes = np.zeros_like(chain)
    codes[at] = chain
    with _native.Distances(ctx, _matrix(codes)) as d:
        edges, comp = d.tree(1)
        rounds = d.tree_rounds()
    assert rounds == R.bit_length()
    if R == 2 * T:
        assert rounds == TU.harness().kpy_tree_max_rounds(R) == 8
    want = sorted((w, *sorted((int(at[p]), int(at[p + 1])))) for p, w in enumerate(weights))
    assert list(zip(edges["differences"].tolist(), edges["a"].tolist(), edges["b"].tolist())) == want and not comp.any()  # the forest is the chain
    _same((edges, comp), TU.forest(codes, 1), f"ruler chain of {R}, permuted {permuted}")


# ---- 4. two rows: the one edge is chosen from both sides ----------------------------------------------------------------------------------
def test_two_rows_record_their_edge_once(ctx):
    codes = D.population(np.random.default_rng(41), 2, 5)
    want = D.all_pairs(codes)
    with _native.Distances(ctx, _matrix(codes)) as d:
        edges, comp = d.tree(0)
        assert d.tree_rounds() == 2
    assert edges.tobytes() == want.tobytes() and len(edges) == 1 and comp.tolist() == [0, 0]


# ---- 5. the two properties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,nb", ((3 * T + 5, 4 * CH + 1), (2 * T + 1, 4)))
def test_the_forest_cut_at_a_threshold_and_the_nearest_pairs(ctx, R, nb):
    codes = D.population(np.random.default_rng([5, R, nb]), R, nb)
    with _native.Distances(ctx, _matrix(codes)) as d:
        for mc in (0, 1, 16 * nb // 2):
            edges, comp = d.tree(mc)
            for t in (0, 1, SPLIT, 40):
                labels, _ = d.clusters((t,), mc, nearest=False)
                assert TU.components_under(R, edges, t).tobytes() == labels[0].tobytes(), (mc, t)
            _, near = d.clusters((), mc)
            have = {(int(e["a"]), int(e["b"])): (int(e["compared"]), int(e["differences"]), int(e["unshared"])) for e in edges}
            for r, n in enumerate(near):
                if n["row"] >= 0:
                    pair = (min(r, int(n["row"])), max(r, int(n["row"])))
                    assert have.get(pair) == (int(n["compared"]), int(n["differences"]), int(n["unshared"])), (mc, r, n)
            assert (near["row"] >= 0).sum() > 0


# ---- 6. state --------------------------------------------------------------------------------------------------------------------------------
def test_the_state_a_tree_leaves_alone(ctx):
    lib = _native.lib()
    codes = D.population(np.random.default_rng(3), 2 * T + 1, 5)
    before = _native.device_allocations()
    with _native.Distances(ctx, _matrix(codes)) as d:
        want = d.pairs(SPLIT, 1)
        n = d.count(SPLIT, 1)
        tree = d.tree(0)
        out = np.zeros(n, _native.DIST_PAIR_DTYPE)
        assert lib.kp_dist_pairs(ctx._h, d._h, _p(out), C.c_int64(n)) == 0 and out.tobytes() == want.tobytes() and n == len(want) > 0  # count -> tree -> pairs
        clusters = d.clusters(CU.LEVELS, 1)
        again = d.tree(0)
        after = d.clusters(CU.LEVELS, 1)
        assert clusters[0].tobytes() == after[0].tobytes() and clusters[1].tobytes() == after[1].tobytes()  # clusters around a tree
        assert again[0].tobytes() == tree[0].tobytes() and again[1].tobytes() == tree[1].tobytes()  # tree twice
        _same(tree, TU.forest(codes, 0), "state")
    assert _native.device_allocations() == before


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    lib = _native.lib()
    codes = D.population(np.random.default_rng(1), 5, 3)
    blocks = _matrix(codes)
    h = C.c_void_p()
    assert lib.kp_dist_create(ctx._h, _p(blocks), C.c_int32(5), C.c_int64(3), C.byref(h)) == 0 and h.value
    edges, comp, n = np.zeros(4, _native.DIST_PAIR_DTYPE), np.full(5, -7, np.int32), C.c_int64(-7)

    def call(c=ctx._h, handle=h, e=_p(edges), cap=4, count=C.byref(n), cm=_p(comp), mc=1):
        return lib.kp_dist_tree(c, handle, C.c_int32(mc), e, C.c_int64(cap), count, cm)

    for kw, why in ((dict(c=None), None), (dict(handle=None), b"null"), (dict(count=None), b"null"), (dict(cap=3), b"n_rows - 1"), (dict(cap=0, e=None), b"n_rows - 1"),
                    (dict(cap=-1), b"n_rows - 1"), (dict(e=None), b"null edge table")):  # fmt: skip
        assert call(**kw) == EINVAL, kw
        if why is not None:
            assert why in lib.kp_last_error(ctx._h), (kw, lib.kp_last_error(ctx._h))
    assert (comp == -7).all() and not edges.view(np.uint8).any()  # a refused call stores nothing
    assert call() == 0 and n.value == len(TU.forest(codes, 1)[0]) and comp.tobytes() == TU.forest(codes, 1)[1].tobytes()
    assert edges[: n.value].tobytes() == TU.forest(codes, 1)[0].tobytes()
    assert call(cm=None, mc=0) == 0 and n.value == 4 and edges.tobytes() == TU.forest(codes, 0)[0].tobytes()  # no component table
    lib.kp_dist_destroy.restype = None
    lib.kp_dist_destroy(h)
    if _device_count() > 1:  # a handle of another device
        other = _native.Context(1)
        try:
            with _native.Distances(other, blocks) as foreign:
                assert call(handle=foreign._h) == EINVAL and b"another device" in lib.kp_last_error(ctx._h)
        finally:
            other.close()
    closed = _native.Distances(ctx, blocks)
    closed.close()
    with pytest.raises(Exception):
        closed.tree()  # a destroyed handle is a null handle to the library
    for rows, nb in ((0, 0), (0, 3), (1, 3)):  # valid: no edge, and one row is its own component
        with _native.Distances(ctx, np.zeros((rows, nb), np.uint64)) as d:
            e, c = d.tree()
            assert len(e) == 0 and c.tolist() == [0] * rows and d.tree_rounds() == 0
    # a matrix that does not fit the key: one row of 2^28 columns -- refused by the tree alone, before anything is launched
    with _native.Distances(ctx, np.zeros((1, _native.TREE_MAX_COLUMNS // 16), np.uint64)) as wide:
        assert wide.count(None, 0) == 0 and wide.clusters((0,), 0)[0].tolist() == [[0]]
        assert lib.kp_dist_tree(ctx._h, wide._h, C.c_int32(1), None, C.c_int64(0), C.byref(n), None) == EINVAL and b"KP_TREE_MAX_COLUMNS" in lib.kp_last_error(ctx._h)
        with pytest.raises(Exception):
            wide.tree()


# ---- 8. the whole route on the miniature database ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run():
    r = Run()
    yield r
    r.close()


def test_serotyper_over_two_batches(run):
    got, want = run.typer.locus_rows, run.want_rows
    assert got.ids == want.ids == run.ids and got.loci() == want.loci() == [0, 3, 6]
    ctx = run.typer.engine.ctx
    for mc in (D.MIN_COMPARED, 0, 1000, 10**6):
        rec = got.tree(ctx, mc)
        assert [tuple(int(r[f]) for f in ("locus", "a", "b", "compared", "differences", "unshared")) for r in rec] == TU.run_edges(want, mc)
        assert got.tree_tsv(ctx, mc) == TU.run_tree_tsv(want, mc) and got.newick_tsv(ctx, mc) == TU.run_newick_tsv(want, mc)
    rec = got.tree(ctx)
    assert rec["locus"].tolist() == [0] * 4 + [3] * 3 + [6] * 2  # every locus one tree
    at = {n: i for i, n in enumerate(run.ids)}
    weights = {L: sorted(int(r["differences"]) for r in rec if r["locus"] == L) for L in (0, 3, 6)}
    # the exact loci and the one that lacks a gene are 0 apart, every SNP hangs on by 1, the far one by a long edge that names it
    assert weights[0][:3] == [0, 0, 1] and weights[0][3] > D.MAX_DIFF and weights[3] == [0, 1, 1] and weights[6] == [0, 1]
    far = [r for r in rec if r["differences"] > D.MAX_DIFF]
    assert len(far) == 1 and at["L0_far_4"] in (int(far[0]["a"]), int(far[0]["b"]))
    lines = got.newick_tsv(ctx).splitlines()
    assert [ln.split(b"\t")[:3] for ln in lines] == [[run.db.loci.ids[L].encode(), b"1", str(k).encode()] for L, k in ((0, 5), (3, 4), (6, 3))]
    assert all(ln.endswith(b";") and ln.count(b"(") == ln.count(b")") for ln in lines) and got.newick_tsv(ctx, 10**6).count(b"\n") == len(run.ids)
    from tests.test_gpu_distances import _want_tsv

    assert got.tsv(ctx) == _want_tsv(want) and got.clusters_tsv(ctx) == CU.run_tsv(want)  # the other tables of the same handles
    got.close()


def test_command_line(run, tmp_path, monkeypatch):
    from kaptive_amd.cli import main
    from kaptive_amd.synth import make_db
    from tests.test_gpu_distances import _want_tsv

    db_path, paths = _write_inputs(run.db, run.genomes, tmp_path)
    made = _count_handles(monkeypatch)
    mst = _native.DISTANCES_HEADER + TU.run_tree_tsv(run.want_rows)
    nwk = _native.newick_header() + TU.run_newick_tsv(run.want_rows)
    assert mst.count(b"\n") == 1 + len(run.ids) - 3 and nwk.count(b"\n") == 1 + 3
    # a run without the flags: no handle, and the files every other run must reproduce
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "plain.tsv"), "--distances", str(tmp_path / "d0.tsv"), "--clusters", str(tmp_path / "c0.tsv")]) == 0
    plain, d0, c0 = ((tmp_path / f).read_bytes() for f in ("plain.tsv", "d0.tsv", "c0.tsv"))
    assert plain.endswith(run.tsv) and d0 == _native.DISTANCES_HEADER + _want_tsv(run.want_rows) and c0 == _native.clusters_header(CU.LEVELS) + CU.run_tsv(run.want_rows)
    del made[:]
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "bare.tsv")]) == 0
    assert made == [] and (tmp_path / "bare.tsv").read_bytes() == plain
    # either flag alone
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o1.tsv"), "--mst", str(tmp_path / "m1.tsv"), "--batch-size", "7"]) == 0
    assert (tmp_path / "m1.tsv").read_bytes() == mst and (tmp_path / "o1.tsv").read_bytes() == plain
    assert len(made) == 3 and not list(tmp_path.glob("*aligned*")) and not list(tmp_path.glob("*newick*"))  # a handle per locus; no other table
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o2.tsv"), "--newick", str(tmp_path / "n2.tsv")]) == 0
    assert (tmp_path / "n2.tsv").read_bytes() == nwk and (tmp_path / "o2.tsv").read_bytes() == plain
    # all four tables: each is what it is alone, and each matrix is uploaded once
    del made[:]
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o3.tsv"), "--mst", str(tmp_path / "m3.tsv"), "--newick", str(tmp_path / "n3.tsv"),
                 "--distances", str(tmp_path / "d3.tsv"), "--clusters", str(tmp_path / "c3.tsv"), "--batch-size", "5"]) == 0  # fmt: skip
    assert [(tmp_path / f).read_bytes() for f in ("o3.tsv", "m3.tsv", "n3.tsv", "d3.tsv", "c3.tsv")] == [plain, mst, nwk, d0, c0]
    assert len(made) == 3
    # --min-compared applies to both
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o4.tsv"), "--mst", str(tmp_path / "m4.tsv"), "--newick", str(tmp_path / "n4.tsv"),
                 "--min-compared", "1000000"]) == 0  # fmt: skip
    assert (tmp_path / "m4.tsv").read_bytes() == _native.DISTANCES_HEADER  # nothing compares a million columns: no edge,
    assert (tmp_path / "n4.tsv").read_bytes() == _native.newick_header() + TU.run_newick_tsv(run.want_rows, 10**6)  # every assembly a tree
    # a second database: a table per database
    o_path = str(make_db("kpsc_o", seed=8).save(tmp_path / "o.npz"))
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "both.tsv"), "--mst", str(tmp_path / "both.m.tsv"), "--newick",
                 str(tmp_path / "both.n.tsv")]) == 0  # fmt: skip
    assert (tmp_path / "both.m.kpsc_k.tsv").read_bytes() == mst and (tmp_path / "both.n.kpsc_k.tsv").read_bytes() == nwk
    assert (tmp_path / "both.m.kpsc_o.tsv").read_bytes().startswith(_native.DISTANCES_HEADER)
    assert (tmp_path / "both.n.kpsc_o.tsv").read_bytes().startswith(_native.newick_header())
    assert (tmp_path / "both.kpsc_k.tsv").read_bytes() == plain
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "x.tsv"), "--newick", "-"]) == 1  # stdout is refused
    assert not (tmp_path / "x.tsv").exists()


@pytest.mark.skipif("_device_count() < 2")
def test_command_line_on_two_devices(run, tmp_path):
    import subprocess
    import sys

    db_path, paths = _write_inputs(run.db, run.genomes, tmp_path)
    from tests.conftest import ROOT

    r = subprocess.run([sys.executable, "-m", "kaptive_amd", "assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--mst", str(tmp_path / "m.tsv"),
                        "--newick", str(tmp_path / "n.tsv"), "--devices", "0,1", "--batch-size", "3"], capture_output=True, timeout=600, cwd=str(ROOT))  # fmt: skip
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    assert (tmp_path / "m.tsv").read_bytes() == _native.DISTANCES_HEADER + TU.run_tree_tsv(run.want_rows)
    assert (tmp_path / "n.tsv").read_bytes() == _native.newick_header() + TU.run_newick_tsv(run.want_rows)
