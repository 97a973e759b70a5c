"""Clusters and nearest neighbours of locus rows on the device (include/kp_spec.h, CLUSTERS; kaptive_amd/csrc/kp_dist_graph.hip) against the
numpy restatement of tests/clusters_util.py: integers, order and bytes, exactly.  Random populations at every shape at which the
epilogue takes another path; a chain, in row order and permuted, which a union-find that loses a hook or a nearest pass that forgets
one side of a pair gets wrong; stars and ties across tiles; the refusals of the entry point and the state it must leave alone; then
the whole route on the 9-locus miniature database: ``Serotyper(db, distances=True)`` over two batches, the command line with
``--clusters``, with ``--distances`` beside it and with ``--db``, a run without the flag, and two devices."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from tests import clusters_util as CU
from tests import distances_util as D
from tests.distances_util import CH, ROWS, SPLIT, T, Run, _count_handles, _device_count, _write_inputs
from tests.test_gpu_distances import BLOCKS as DIST_BLOCKS

pytestmark = pytest.mark.gpu

BLOCKS = (1, 4, 4 * CH, 4 * CH + 1, 8 * CH + 3)
EINVAL = -1
LEVEL_SETS = ((0,), CU.LEVELS, (SPLIT,), CU.EIGHT)


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
    (gl, gn), (wl, wn) = got, want
    assert gl.dtype == np.int32 and gl.shape == wl.shape and gn.dtype == _native.DIST_NEAREST_DTYPE and gn.shape == wn.shape, what
    if gl.tobytes() != wl.tobytes():
        k, r = np.argwhere(gl != wl)[0]
        raise AssertionError(f"{what}: label of row {r} at level {k}: {gl[k, r]} on the device, {wl[k, r]} wanted ({int((gl != wl).sum())} differ)")
    if gn.tobytes() != wn.tobytes():
        r = next(i for i in range(len(gn)) if gn[i] != wn[i])
        raise AssertionError(f"{what}: nearest of row {r}: {gn[r]} on the device, {wn[r]} wanted")


# ---- 1. random populations: every shape, every level set, every min_compared -------------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
def test_clusters_against_the_restatement(ctx, R):
    assert set(BLOCKS) <= set(DIST_BLOCKS) and CU.MAX_LEVELS == _native.CLUST_MAX_LEVELS and len(CU.EIGHT) == CU.MAX_LEVELS
    for nb in BLOCKS:
        codes = D.population(np.random.default_rng([R, nb]), R, nb)
        every = D.all_pairs(codes)  # the reference's pairs, once: every level set and min_compared selects from them
        first = {}
        with _native.Distances(ctx, _matrix(codes)) as d:
            for mc in (0, 1, 16 * nb // 2):
                near = CU.nearest_of(R, every, mc)
                for levels in LEVEL_SETS:
                    want = CU.labels_of(R, every, levels, mc), near
                    got = d.clusters(levels, mc)
                    _same(got, want, f"R {R}, NB {nb}, levels {levels}, min_compared {mc}")
                    assert (np.diff(got[0], axis=0) <= 0).all() and (got[0] <= np.arange(R)).all()  # levels nest; a label is the smallest row
                    first[(levels, mc)] = got[0].tobytes() + got[1].tobytes()
                labels, alone = d.clusters((), mc)  # K = 0: nearest alone
                assert labels.shape == (0, R) and alone.tobytes() == near.tobytes()
                labels, none = d.clusters(CU.LEVELS, mc, nearest=False)
                assert none is None and labels.tobytes() == CU.labels_of(R, every, CU.LEVELS, mc).tobytes()
            if R >= T - 1:
                labels, near = d.clusters((0, SPLIT), 1)
                if nb >= 4 * CH:  # (long enough for no planted run of N or GAP to cover a row)
                    assert labels[0, 1] == 0 and near[1]["row"] == 0 and near[0]["row"] == 1 and near[1]["differences"] == 0  # the identical rows
                assert near[2]["row"] == -1 and near[3]["row"] == -1 and labels[1, 2] == 2 and labels[1, 3] == 3  # all GAP, all N: nothing compared
                assert all(labels[1, r] == labels[1, 10] for r in range(4, 10)) and 1 < len(set(labels[1].tolist())) < R  # the levels split the population
        with _native.Distances(ctx, _matrix(codes)) as again:  # a second handle, the calls in another order: the same bytes
            for key in reversed(list(first)):
                got = again.clusters(*key)
                assert got[0].tobytes() + got[1].tobytes() == first[key], key


# ---- 2. a chain ----------------------------------------------------------------------------------------------------------------------------
def _chain(R, nb):
    rng = np.random.default_rng(11)
    founder = rng.integers(0, 4, 16 * nb).astype(np.uint8)
    codes = np.tile(founder, (R, 1))
    for r in range(R):
        codes[r, :r] = (founder[:r] + 1) % 4  # differences(r, s) = |r - s|
    return codes


@pytest.mark.parametrize("permuted", (False, True))
def test_a_chain_in_row_order_and_permuted(ctx, permuted):
    R, nb = 3 * T + 5, 4 * CH + 1
    assert 16 * nb >= R
    chain = _chain(R, nb)
    at = np.random.default_rng(12).permutation(R) if permuted else np.arange(R)  # chain position p lies in row at[p]
    codes = np.zeros_like(chain)
    codes[at] = chain
    with _native.Distances(ctx, _matrix(codes)) as d:
        labels, near = d.clusters((0, 1, 2, 3), 1)
        alone, _ = d.clusters((1,), 1, nearest=False)
    assert labels[0].tolist() == list(range(R))  # level 0: all singletons
    assert not labels[1:].any() and not alone.any()  # one cluster from level 1 on: its label is the smallest row, 0
    for p in range(R):
        nbrs = [int(at[q]) for q in (p - 1, p + 1) if 0 <= q < R]
        r = int(at[p])
        assert near[r]["row"] == min(nbrs) and (near[r]["differences"], near[r]["compared"], near[r]["unshared"]) == (1, 16 * nb, 0), (p, r, near[r])
    _same((labels, near), CU.clusters(codes, (0, 1, 2, 3), 1), f"chain, permuted {permuted}")


# ---- 3. stars and ties ---------------------------------------------------------------------------------------------------------------------
def test_stars_and_ties_across_tiles(ctx):
    R, nb = 3 * T + 5, 4 * CH + 1
    cols = 16 * nb
    rng = np.random.default_rng(13)
    codes = rng.integers(0, 4, (R, cols)).astype(np.uint8)  # strangers: three quarters of the columns apart
    centre, spokes = R - 1, (3, T - 1, T, 2 * T + 7, 3 * T + 1)  # the centre in the last tile, its relatives in every tile
    for i, r in enumerate(spokes):
        codes[r] = codes[centre]
        codes[r, 5 + 64 * i] = (codes[centre, 5 + 64 * i] + 1) % 4  # one column from the centre, two from each other
    third, early, late = T + 30, 20, 2 * T + 20  # two rows equally near to a third, in an earlier and in a later tile
    for r, c in ((early, 0), (late, cols - 1)):
        codes[r] = codes[third]
        codes[r, c] = (codes[third, c] + 2) % 4
    lonely, mc = 50, 16
    codes[lonely, 4:] = D.N  # only four columns hold a base: every partner fails min_compared
    codes[60] = codes[61] = codes[62]
    codes[61, 7] = D.GAP  # 60 and 62 identical; 61 differs in nothing that is compared
    levels = (0, 1, 2)
    with _native.Distances(ctx, _matrix(codes)) as d:
        labels, near = d.clusters(levels, mc)
        loose, loose_near = d.clusters(levels, 0)
    star = (*spokes, centre)
    assert all(labels[0, r] == r for r in star)  # nobody is identical to anybody
    assert all(labels[1, r] == 3 and labels[2, r] == 3 for r in star) and sum(labels[1] == 3) == len(star)  # joined through the centre alone
    assert all(near[r]["row"] == centre and near[r]["differences"] == 1 for r in spokes) and near[centre]["row"] == 3
    assert near[third]["row"] == early and near[third]["differences"] == 1 and near[early]["row"] == near[late]["row"] == third  # the smaller row wins
    assert labels[:, [early, third, late]].tolist() == [[early, third, late], [early] * 3, [early] * 3]
    assert near[lonely]["row"] == -1 and near[lonely].tolist() == (-1, 0, 0, 0) and labels[:, lonely].tolist() == [lonely] * 3
    assert not (near["row"] == lonely).any() and loose_near[lonely]["row"] >= 0  # ... and with min_compared 0 it has a neighbour
    assert labels[:, [60, 61, 62]].tolist() == [[60] * 3] * 3 and near[60]["row"] == 61 and near[61]["row"] == 60 and near[62]["row"] == 60
    _same((labels, near), CU.clusters(codes, levels, mc), "stars and ties")
    _same((loose, loose_near), CU.clusters(codes, levels, 0), "stars and ties, min_compared 0")


# ---- 4. refusals and state ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_listing_state(ctx):
    lib = _native.lib()
    codes = D.population(np.random.default_rng(1), 5, 3)
    blocks = _matrix(codes)
    h = C.c_void_p()
    assert lib.kp_dist_create(ctx._h, _p(blocks), C.c_int32(5), C.c_int64(3), C.byref(h)) == 0 and h.value
    labels, near = np.full((8, 5), -7, np.int32), np.zeros(5, _native.DIST_NEAREST_DTYPE)

    def call(levels=(0, 1), c=ctx._h, handle=h, lab=_p(labels), nr=_p(near), n=None, mc=1):
        lv = np.array(levels if levels is not None else (), np.int32)
        return lib.kp_dist_clusters(c, handle, _p(lv) if levels is not None else None, C.c_int32(len(lv) if n is None else n), C.c_int32(mc), lab, nr)

    for kw, why in ((dict(c=None), None), (dict(handle=None), b"null"), (dict(n=9, levels=tuple(range(9))), b"KP_CLUST_MAX_LEVELS"), (dict(n=-1), b"KP_CLUST_MAX_LEVELS"),
                    (dict(levels=(-1, 2)), b"ascending"), (dict(levels=(1, 1)), b"ascending"), (dict(levels=(2, 1)), b"ascending"), (dict(levels=None, n=2), b"null"),
                    (dict(lab=None), b"label")):  # fmt: skip
        assert call(**kw) == EINVAL, kw
        if why is not None:
            assert why in lib.kp_last_error(ctx._h), (kw, lib.kp_last_error(ctx._h))
    assert (labels == -7).all() and not near.view(np.uint8).any()  # a refused call stores nothing
    assert call(levels=(), lab=None) == 0 and near.tobytes() == CU.clusters(codes, (), 1)[1].tobytes()  # K = 0: no label table needed
    assert call(nr=None) == 0 and labels[:2].tobytes() == CU.clusters(codes, (0, 1), 1)[0].tobytes() and (labels[2:] == -7).all()  # no nearest output
    assert call(levels=tuple(range(8))) == 0 and labels.tobytes() == CU.clusters(codes, tuple(range(8)), 1)[0].tobytes()
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
        closed.clusters()  # a destroyed handle is a null handle to the library
    for rows, nb in ((0, 0), (0, 3), (1, 3)):  # valid: one row is its own cluster and has no neighbour
        with _native.Distances(ctx, np.zeros((rows, nb), np.uint64)) as d:
            lab, nr = d.clusters()
            assert lab.shape == (5, rows) and not lab.any() and nr.tolist() == [(-1, 0, 0, 0)] * rows
    # kp_dist_count -> kp_dist_clusters -> kp_dist_pairs: the listing of the count, untouched
    codes = D.population(np.random.default_rng(3), 2 * T + 1, 5)
    with _native.Distances(ctx, _matrix(codes)) as d:
        want = d.pairs(SPLIT, 1)
        n = d.count(SPLIT, 1)
        d.clusters((0, 40), 0)
        out = np.zeros(n, _native.DIST_PAIR_DTYPE)
        assert lib.kp_dist_pairs(ctx._h, d._h, _p(out), C.c_int64(n)) == 0 and out.tobytes() == want.tobytes() and n == len(want) > 0


def test_allocation_count_around_a_handle_that_clustered(ctx):
    codes = D.population(np.random.default_rng(2), 2 * T + 1, 5)
    before = _native.device_allocations()
    d = _native.Distances(ctx, _matrix(codes))
    sizes = [len(d.pairs(0, 0)), d.clusters((0,), 1)[0].shape, len(d.pairs(None, 0)), d.clusters(CU.EIGHT, 0)[0].shape, d.clusters((), 0)[0].shape]
    assert sizes[1] == (1, 2 * T + 1) and sizes[3] == (8, 2 * T + 1) and sizes[4] == (0, 2 * T + 1) and sizes[0] < sizes[2]
    d.close()
    assert _native.device_allocations() == before


# ---- 5. the whole route on the miniature database --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run():
    r = Run()
    yield r
    r.close()


def _records(rec):
    return [(int(r["locus"]), int(r["assembly"]), [int(x) for x in r["labels"]], int(r["nearest"]), int(r["compared"]), int(r["differences"]), int(r["unshared"])) for r in rec]


def test_serotyper_over_two_batches(run):
    got, want = run.typer.locus_rows, run.want_rows
    assert got.ids == want.ids == run.ids and got.loci() == want.loci() == [0, 3, 6]
    ctx = run.typer.engine.ctx
    for levels, mc in ((CU.LEVELS, D.MIN_COMPARED), ((0,), 0), ((), 1), (CU.EIGHT, 1000)):
        assert _records(got.clusters(ctx, levels, mc)) == CU.run_records(want, levels, mc)
        assert got.clusters_tsv(ctx, levels, mc) == CU.run_tsv(want, levels, mc)
    rec = got.clusters(ctx)
    assert len(rec) == len(run.ids) and rec["locus"].tolist() == [0] * 5 + [3] * 4 + [6] * 3
    at = {n: i for i, n in enumerate(run.ids)}
    of = {int(r["assembly"]): r for r in rec}
    hc = lambda name, k: int(of[at[name]]["labels"][k])  # noqa: E731
    assert hc("L0_exact_0", 0) == hc("L0_exact_1", 0) != hc("L0_snp_2", 0) and hc("L0_exact_0", 1) == hc("L0_snp_2", 1)  # identical at HC0, the SNP joins at HC1
    assert len({hc(n, 4) for n in run.ids if run.plan[n][0] == 0 and run.plan[n][1] != "far"}) == 1 and hc("L0_far_4", 4) == at["L0_far_4"]  # beyond every level
    assert hc("L3_snp_1", 0) != hc("L3_snp_2", 0) and hc("L3_snp_1", 1) == hc("L3_snp_2", 1) == hc("L3_exact_0", 1)  # two apart, joined through the exact ones
    near = of[at["L0_far_4"]]
    assert near["nearest"] >= 0 and near["differences"] > D.MAX_DIFF and run.plan[run.ids[int(near["nearest"])]][0] == 0  # nearest sees beyond the levels
    twin = of[at["L0_exact_0"]]  # (the assembly that lacks a gene is 0 differences away as well: the smaller number wins)
    assert int(twin["nearest"]) == min(at["L0_exact_1"], at["L0_lacking_3"]) and int(twin["differences"]) == 0
    from tests.test_gpu_distances import _want_tsv

    assert got.tsv(ctx) == _want_tsv(want)  # the other table of the same handles
    got.close()


def test_command_line(run, tmp_path, monkeypatch):
    from kaptive_amd.cli import main
    from kaptive_amd.synth import make_db
    from tests.test_gpu_distances import _want_tsv

    db_path, paths = _write_inputs(run.db, run.genomes, tmp_path)
    made = _count_handles(monkeypatch)
    table = _native.clusters_header(CU.LEVELS) + CU.run_tsv(run.want_rows)
    assert table.count(b"\n") == 1 + len(run.ids)
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "plain.tsv")]) == 0
    assert made == []  # a run without the flag creates no handle
    plain = (tmp_path / "plain.tsv").read_bytes()
    assert plain.endswith(run.tsv)
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--clusters", str(tmp_path / "c.tsv"), "--batch-size", "7"]) == 0
    assert (tmp_path / "c.tsv").read_bytes() == table and (tmp_path / "out.tsv").read_bytes() == plain
    assert len(made) == 3 and not list(tmp_path.glob("*aligned*"))  # a handle per locus with two rows or more; no --aligned table
    # --distances alone, then both together: each table is what it is alone, and each matrix is uploaded once
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o1.tsv"), "--distances", str(tmp_path / "d1.tsv")]) == 0
    d_alone = (tmp_path / "d1.tsv").read_bytes()
    assert d_alone == _native.DISTANCES_HEADER + _want_tsv(run.want_rows)
    del made[:]
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o2.tsv"), "--clusters", str(tmp_path / "c2.tsv"), "--distances", str(tmp_path / "d2.tsv"),
                 "--batch-size", "5"]) == 0  # fmt: skip
    assert (tmp_path / "c2.tsv").read_bytes() == table and (tmp_path / "d2.tsv").read_bytes() == d_alone and (tmp_path / "o2.tsv").read_bytes() == plain
    assert len(made) == 3
    # the levels and --min-compared, which applies to both tables
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o3.tsv"), "--clusters", str(tmp_path / "c3.tsv"), "--cluster-levels", "0,3", "--min-compared", "1000",
                 "--distances", str(tmp_path / "d3.tsv"), "--max-distance", "0"]) == 0  # fmt: skip
    assert (tmp_path / "c3.tsv").read_bytes() == _native.clusters_header((0, 3)) + CU.run_tsv(run.want_rows, (0, 3), 1000)
    assert (tmp_path / "d3.tsv").read_bytes() == _native.DISTANCES_HEADER + _want_tsv(run.want_rows, 0, 1000)
    # a second database: a table per database
    o_path = str(make_db("kpsc_o", seed=8).save(tmp_path / "o.npz"))
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "both.tsv"), "--clusters", str(tmp_path / "both.c.tsv")]) == 0
    assert (tmp_path / "both.c.kpsc_k.tsv").read_bytes() == table
    assert (tmp_path / "both.c.kpsc_o.tsv").read_bytes().startswith(_native.clusters_header(CU.LEVELS))
    assert (tmp_path / "both.kpsc_k.tsv").read_bytes() == plain
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "x.tsv"), "--clusters", "-"]) == 1  # stdout is refused
    assert not (tmp_path / "x.tsv").exists()


@pytest.mark.skipif("_device_count() < 2")
def test_command_line_on_two_devices(run, tmp_path):
    import subprocess
    import sys

    db_path, paths = _write_inputs(run.db, run.genomes, tmp_path)
    from tests.conftest import ROOT

    r = subprocess.run([sys.executable, "-m", "kaptive_amd", "assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--clusters",
                        str(tmp_path / "c.tsv"), "--devices", "0,1", "--batch-size", "3"], capture_output=True, timeout=600, cwd=str(ROOT))  # fmt: skip
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    assert (tmp_path / "c.tsv").read_bytes() == _native.clusters_header(CU.LEVELS) + CU.run_tsv(run.want_rows)
