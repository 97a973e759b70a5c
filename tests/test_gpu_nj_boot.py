"""Bootstrap support of the neighbour-joining tree on the device (include/kp_spec.h, BOOTSTRAP; kaptive_amd/csrc/kp_dist_boot.hip)
against the NumPy restatement in tests/nj_boot_util.py: the weights of a replicate, every record of every replicate's tree as bytes
and the support as exact-set counts, at every shape at which the tiles, the row sums or the pick take another path, under every
batching; trees without an inner edge; identical rows; a planted tree every replicate must recover; the state the call must leave
alone; what it allocates; its refusals; then the whole route on the 9-locus miniature database."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from tests import clusters_util as CU
from tests import distances_util as D
from tests import nj_boot_util as B
from tests import nj_util as NJ
from tests.distances_util import CH, SPLIT, T, Run, _count_handles, _device_count, _write_inputs

pytestmark = pytest.mark.gpu

EINVAL = -1
N_REP = 6


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _matrix(codes) -> np.ndarray:
    return D.pack(codes).reshape(codes.shape[0], -1) if codes.shape[0] else np.zeros((0, codes.shape[1] // 16), np.uint64)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _same_trees(got, want, what):
    assert got.dtype == _native.NJ_NODE_DTYPE and got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        r, t = next((r, t) for r in range(got.shape[0]) for t in range(got.shape[1]) if got[r, t].tobytes() != want[r, t].tobytes())
        raise AssertionError(f"{what}: replicate {r}, record {t}: {got[r, t]} on the device, {want[r, t]} wanted")


# ---- 1. the weights ------------------------------------------------------------------------------------------------------------------------
def test_numpy_weights_use_more_than_two_planes_at_one_block():
    assert B.weights(1, 1, 16).max() >= 4  # (CPU: the condition of the case below)


@pytest.mark.parametrize("nb", (1, 4, 4 * CH + 1))
def test_weights_against_numpy(ctx, nb):
    with _native.Distances(ctx, np.zeros((3, nb), np.uint64)) as d:
        for seed in (0, 1, 2**64 - 1):
            for r in (0, 1, 9999):
                got = d.boot_weights(seed, r)
                assert got.dtype == np.uint8 and got.tobytes() == B.weights(seed, r, 16 * nb).tobytes(), (nb, seed, r, got.tolist())


# ---- 2. trees and support: every shape, every batching -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", (1, 4 * CH + 1))
@pytest.mark.parametrize("R", (4, 5, T - 1, T + 1, 2 * T + 1))
def test_trees_and_support_against_numpy(ctx, R, nb):
    codes = D.population(np.random.default_rng([R, nb, 7]), R, nb)
    want = {seed: B.bootstrap(codes, 1, seed, N_REP) for seed in (1, 5)}
    taxa, nodes = want[1][0], want[1][1]
    if R >= T - 1 and nb > 1:
        assert len(taxa) >= 4  # the shapes with inner edges
    with _native.Distances(ctx, _matrix(codes)) as d:
        got_taxa, got_nodes = d.nj(1)
        assert got_taxa.tobytes() == taxa.tobytes() and got_nodes.tobytes() == nodes.tobytes()
        support, trees = d.nj_support(1, got_nodes, N_REP, seed=1, trees=True)
        _same_trees(trees, want[1][2], f"R {R}, NB {nb}")
        assert support.dtype == np.int32 and support.tolist() == want[1][3].tolist(), (R, nb)
        assert d.nj_support(1, got_nodes, N_REP, seed=1).tobytes() == support.tobytes()  # without the trees
        for most in (1, 4):  # one at a time; four, which divides nothing evenly
            s, t = d.nj_support(1, got_nodes, N_REP, seed=1, max_batch=most, trees=True)
            assert s.tobytes() == support.tobytes() and t.tobytes() == trees.tobytes(), most
    with _native.Distances(ctx, _matrix(codes)) as again:  # a second handle, a second seed: its own bytes, again equal
        s5, t5 = again.nj_support(1, nodes, N_REP, seed=5, trees=True)
        _same_trees(t5, want[5][2], f"R {R}, NB {nb}, seed 5")
        assert s5.tolist() == want[5][3].tolist()
        s5b, t5b = again.nj_support(1, nodes, N_REP, seed=5, max_batch=4, trees=True)
        assert s5b.tobytes() == s5.tobytes() and t5b.tobytes() == t5.tobytes()
        if len(nodes) > 1 and nb > 1:
            assert t5.tobytes() != want[1][2].tobytes()
        s1 = again.nj_support(1, nodes, N_REP, seed=1)
        assert s1.tolist() == want[1][3].tolist()


# ---- 3. small trees; identical rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 1, 2, 3))
def test_trees_without_an_inner_edge(ctx, n):
    rng = np.random.default_rng(n)
    codes = rng.integers(0, 4, (n + 1, 48)).astype(np.uint8)
    codes[n] = D.GAP  # a row that is no taxon
    with _native.Distances(ctx, _matrix(codes)) as d:
        taxa, nodes = d.nj(1)
        assert len(taxa) == n and len(nodes) == (0, 0, 1, 1)[n]
        support, trees = d.nj_support(1, nodes, 4, trees=True)
        assert support.tolist() == [-1] * len(nodes) and trees.shape == (4, len(nodes))
        assert d.nj_support(1, nodes, 4).tolist() == [-1] * len(nodes)
        want = B.bootstrap(codes, 1, 1, 4)
        _same_trees(trees, want[2], f"{n} taxa")  # two and three taxa still have replicate trees: their one record
    with _native.Distances(ctx, np.zeros((0, 3), np.uint64)) as d:
        assert d.nj_support(1, np.zeros(0, _native.NJ_NODE_DTYPE), 4).tolist() == []


def test_identical_rows_support_every_split_of_the_caterpillar(ctx):
    R, nb, N = T + 5, 4, 5
    codes = np.tile(np.random.default_rng(21).integers(0, 4, 16 * nb).astype(np.uint8), (R, 1))
    with _native.Distances(ctx, _matrix(codes)) as d:
        taxa, nodes = d.nj(1)
        support, trees = d.nj_support(1, nodes, N, trees=True)
    assert len(taxa) == R and support.tolist() == [N] * (R - 3) + [-1]
    assert all(trees[r].tobytes() == nodes.tobytes() for r in range(N))  # every replicate ties everywhere, as the tree itself


# ---- 4. a planted tree ------------------------------------------------------------------------------------------------------------------------
def test_every_replicate_recovers_a_planted_tree(ctx):
    """Every inner branch owns at least 40 columns of the 928: a replicate that draws none of them has probability about e^-40."""
    n, N, seed = 12, 16, 2
    codes, planted, _, W = NJ.additive(np.random.default_rng(33), n, cols_per_branch=(40, 48))
    taxa, nodes, want_trees, want = B.bootstrap(codes, 1, seed, N)
    assert NJ.splits(n, nodes) == planted and len(planted) == n - 3 and want.tolist() == [N] * (n - 3) + [-1]  # the condition, on the CPU
    with _native.Distances(ctx, _matrix(codes)) as d:
        got_taxa, got_nodes = d.nj(1)
        support, trees = d.nj_support(1, got_nodes, N, seed=seed, trees=True)
    assert got_nodes.tobytes() == nodes.tobytes()
    _same_trees(trees, want_trees, "planted tree")
    assert support.tolist() == [N] * (n - 3) + [-1]
    assert all(NJ.splits(n, trees[r]) == planted for r in range(N))


# ---- 5. state and allocation ----------------------------------------------------------------------------------------------------------------
def test_the_state_a_bootstrap_leaves_alone(ctx):
    lib = _native.lib()
    codes = D.population(np.random.default_rng(3), 2 * T + 1, 5)
    with _native.Distances(ctx, _matrix(codes)) as d:
        want = d.pairs(SPLIT, 1)
        n = d.count(SPLIT, 1)
        tree = d.nj(1)
        forest, clusters, sites = d.tree(1), d.clusters(CU.LEVELS, 1), d.sites()
        support = d.nj_support(1, tree[1], N_REP)
        out = np.zeros(n, _native.DIST_PAIR_DTYPE)
        assert lib.kp_dist_pairs(ctx._h, d._h, _p(out), C.c_int64(n)) == 0 and out.tobytes() == want.tobytes() and n == len(want) > 0  # count -> bootstrap -> pairs
        out_sites = np.zeros(len(sites), _native.SITE_DTYPE)
        assert lib.kp_dist_sites(ctx._h, d._h, _p(out_sites), C.c_int64(len(sites))) == 0 and out_sites.tobytes() == sites.tobytes() and len(sites) > 0
        forest2, clusters2, again = d.tree(1), d.clusters(CU.LEVELS, 1), d.nj(1)
        assert forest[0].tobytes() == forest2[0].tobytes() and forest[1].tobytes() == forest2[1].tobytes()
        assert clusters[0].tobytes() == clusters2[0].tobytes() and clusters[1].tobytes() == clusters2[1].tobytes()
        assert again[0].tobytes() == tree[0].tobytes() and again[1].tobytes() == tree[1].tobytes()
        assert d.nj_support(1, tree[1], N_REP).tobytes() == support.tobytes()  # the bootstrap twice
        # another min_compared between two bootstraps: the taxa of each call are its own
        few = d.nj(codes.shape[1] * 9 // 10)
        assert 4 <= len(few[0]) < len(tree[0])
        s_few = d.nj_support(codes.shape[1] * 9 // 10, few[1], N_REP)
        assert d.nj_support(1, tree[1], N_REP).tobytes() == support.tobytes()
        assert s_few.tolist() == B.bootstrap(codes, codes.shape[1] * 9 // 10, 1, N_REP)[3].tolist()
    assert support.tolist() == B.bootstrap(codes, 1, 1, N_REP)[3].tolist()


def test_nothing_of_a_batch_stays_with_the_handle(ctx):
    """``device_allocations`` counts the buffers that had to grow.  The handle's O(n) tables are made once, by the first call, and
    the matrices, the weights and every table of a batch are new buffers of every call: nothing grows, whatever the order of the
    sizes -- tables kept with the handle would have to grow for the second, larger tree and for the larger batch."""
    codes = D.population(np.random.default_rng(5), 3 * T + 5, 4 * CH + 1)
    before = _native.device_allocations()
    with _native.Distances(ctx, _matrix(codes)) as d:
        mc = codes.shape[1] * 9 // 10
        few, many = d.nj(mc), d.nj(1)
        assert 4 <= len(few[0]) < len(many[0])
        a = d.nj_support(mc, few[1], 3)
        b = d.nj_support(1, many[1], 9)
        assert _native.device_allocations() == before
        assert d.nj_support(1, many[1], 9, max_batch=2).tobytes() == b.tobytes() and d.nj_support(mc, few[1], 3).tobytes() == a.tobytes()
        assert _native.device_allocations() == before
    assert _native.device_allocations() == before


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    lib = _native.lib()
    rng = np.random.default_rng(1)
    codes = rng.integers(0, 4, (6, 48)).astype(np.uint8)
    blocks = _matrix(codes)
    taxa, nodes, want_trees, want = B.bootstrap(codes, 1, 1, 3)
    assert len(taxa) == 6 and len(nodes) == 4
    h = C.c_void_p()
    assert lib.kp_dist_create(ctx._h, _p(blocks), C.c_int32(6), C.c_int64(3), C.byref(h)) == 0 and h.value
    support, trees = np.full(4, -7, np.int32), np.zeros((3, 4), _native.NJ_NODE_DTYPE)

    def call(c=ctx._h, handle=h, reps=3, most=0, ref=_p(nodes), n_ref=4, s=_p(support), cap_s=4, t=_p(trees), cap_t=12, mc=1):
        return lib.kp_dist_nj_bootstrap(c, handle, C.c_int32(mc), C.c_uint64(1), C.c_int32(reps), C.c_int32(most), ref, C.c_int64(n_ref), s, C.c_int64(cap_s), t, C.c_int64(cap_t))

    bad_ids = nodes.copy()
    bad_ids["a"][1] = 6 + 1  # its own node
    for kw, why in ((dict(c=None), None), (dict(handle=None), b"null"), (dict(reps=0), b"replicates"), (dict(reps=-1), b"replicates"), (dict(reps=10001), b"replicates"),
                    (dict(most=-1), b"negative"), (dict(ref=None), b"null record table"), (dict(s=None), b"null support"), (dict(t=None), b"null table of replicate trees"),
                    (dict(n_ref=3), b"records of the tree"), (dict(n_ref=5), b"records of the tree"), (dict(n_ref=0, ref=None), b"records of the tree"),
                    (dict(cap_s=3), b"fewer support"), (dict(cap_s=-1), b"negative"), (dict(cap_t=11), b"fewer records"), (dict(cap_t=-1), b"negative"),
                    (dict(mc=49), b"records of the tree"), (dict(ref=_p(bad_ids)), b"node id")):  # fmt: skip
        assert call(**kw) == EINVAL, kw
        if why is not None:
            assert why in lib.kp_last_error(ctx._h), (kw, lib.kp_last_error(ctx._h))
    assert (support == -7).all() and not trees.view(np.uint8).any()  # a refused call stores nothing
    assert call(t=None, cap_t=0) == 0 and support.tolist() == want.tolist()
    support[:] = -7
    assert call() == 0 and support.tolist() == want.tolist() and trees.tobytes() == want_trees.tobytes()
    # the weights
    w = np.full(48, 7, np.uint8)
    wcall = lambda c=ctx._h, handle=h, r=0, out=_p(w), cap=48: lib.kp_dist_boot_weights(c, handle, C.c_uint64(1), C.c_int32(r), out, C.c_int64(cap))  # noqa: E731
    for kw in (dict(c=None), dict(handle=None), dict(out=None), dict(r=-1), dict(r=10000), dict(cap=47)):
        assert wcall(**kw) == EINVAL, kw
    assert (w == 7).all() and wcall() == 0 and w.tobytes() == B.weights(1, 0, 48).tobytes()
    lib.kp_dist_destroy(h)
    if _device_count() > 1:  # a handle of another device
        other = _native.Context(1)
        try:
            with _native.Distances(other, blocks) as foreign:
                assert call(handle=foreign._h) == EINVAL and b"another device" in lib.kp_last_error(ctx._h)
                assert wcall(handle=foreign._h) == EINVAL
        finally:
            other.close()
    closed = _native.Distances(ctx, blocks)
    closed.close()
    with pytest.raises(Exception):
        closed.nj_support(1, nodes, 3)


def test_more_taxa_than_the_limit_are_refused(ctx):
    R = _native.NJ_MAX_TAXA + 1
    before = _native.device_allocations()
    with _native.Distances(ctx, np.zeros((R, 1), np.uint64)) as d:
        with pytest.raises(Exception, match="KP_NJ_MAX_TAXA"):
            d.nj_support(1, np.zeros(R - 2, _native.NJ_NODE_DTYPE), 2)
    assert _native.device_allocations() == before


# ---- 7. the whole route on the miniature database ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run():
    r = Run()
    yield r
    r.close()


@pytest.fixture(scope="module")
def want_tsv(run):
    return B.run_tsv(run.want_rows, 5, 3)


def test_serotyper_over_two_batches(run, want_tsv):
    got, want = run.typer.locus_rows, run.want_rows
    ctx = run.typer.engine.ctx
    text, skipped = got.nj_tsv(ctx, bootstrap=5, seed=3)
    assert text == want_tsv and skipped == [] and text.count(b"\n") == 3
    assert [ln.split(b"\t")[:4] for ln in text.splitlines()] == [[run.db.loci.ids[L].encode(), str(k).encode(), str(k).encode(), b"5"] for L, k in ((0, 5), (3, 4), (6, 3))]
    assert got.nj_tsv(ctx) == (NJ.run_tsv(want), []) == got.nj_tsv(ctx, bootstrap=0)  # without it: what it returned before
    assert got.nj_tsv(ctx, D.MIN_COMPARED, 5, 4)[0] == B.run_tsv(want, 5, 4)
    for L in got.loci():
        idx, taxa, nodes, support = got.nj_support(ctx, L, 5, 3)
        w = B.bootstrap(D.unpack(want.locus_matrix(L)[1]), D.MIN_COMPARED, 3, 5)
        assert taxa.tobytes() == w[0].tobytes() and nodes.tobytes() == w[1].tobytes() and support.tolist() == w[3].tolist()
    got.close()


def test_command_line(run, want_tsv, tmp_path, monkeypatch):
    from kaptive_amd.cli import main
    from kaptive_amd.synth import make_db

    db_path, paths = _write_inputs(run.db, run.genomes, tmp_path)
    made = _count_handles(monkeypatch)
    labelled, plain_nj = _native.nj_support_header() + want_tsv, _native.nj_header() + NJ.run_tsv(run.want_rows)
    assert labelled.count(b"\n") == 1 + 3
    others = ("distances", "clusters", "mst", "newick", "sites", "snp-alignment")
    flags = lambda tag: [x for f in others for x in (f"--{f}", str(tmp_path / f"{f}.{tag}.tsv"))]  # noqa: E731
    # a run without the new flag: the bytes --nj wrote before, and the files every other run must reproduce
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o0.tsv"), "--nj", str(tmp_path / "t0.tsv"), *flags("0")]) == 0
    assert (tmp_path / "t0.tsv").read_bytes() == plain_nj
    plain = (tmp_path / "o0.tsv").read_bytes()
    base = [(tmp_path / f"{f}.0.tsv").read_bytes() for f in others]
    # the flag alone
    del made[:]
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o1.tsv"), "--nj", str(tmp_path / "t1.tsv"), "--nj-bootstrap", "5", "--nj-seed", "3", "--batch-size", "7"]) == 0
    assert (tmp_path / "t1.tsv").read_bytes() == labelled and (tmp_path / "o1.tsv").read_bytes() == plain and len(made) == 3  # a handle per locus
    # beside every other table
    del made[:]
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o2.tsv"), "--nj", str(tmp_path / "t2.tsv"), "--nj-bootstrap", "5", "--nj-seed", "3", *flags("2"), "--batch-size", "5"]) == 0
    assert (tmp_path / "t2.tsv").read_bytes() == labelled and (tmp_path / "o2.tsv").read_bytes() == plain
    assert [(tmp_path / f"{f}.2.tsv").read_bytes() for f in others] == base and len(made) == 3
    # the default seed is 1
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o3.tsv"), "--nj", str(tmp_path / "t3.tsv"), "--nj-bootstrap", "5"]) == 0
    assert (tmp_path / "t3.tsv").read_bytes() == _native.nj_support_header() + B.run_tsv(run.want_rows, 5, 1)
    # a second database: a table per database
    o_path = str(make_db("kpsc_o", seed=8).save(tmp_path / "o.npz"))
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "both.tsv"), "--nj", str(tmp_path / "both.t.tsv"), "--nj-bootstrap", "5", "--nj-seed", "3"]) == 0
    assert (tmp_path / "both.t.kpsc_k.tsv").read_bytes() == labelled and (tmp_path / "both.t.kpsc_o.tsv").read_bytes().startswith(_native.nj_support_header())


@pytest.mark.skipif("_device_count() < 2")
def test_command_line_on_two_devices(run, want_tsv, tmp_path):
    import subprocess
    import sys

    db_path, paths = _write_inputs(run.db, run.genomes, tmp_path)
    from tests.conftest import ROOT

    r = subprocess.run([sys.executable, "-m", "kaptive_amd", "assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--nj", str(tmp_path / "t.tsv"),
                        "--nj-bootstrap", "5", "--nj-seed", "3", "--devices", "0,1", "--batch-size", "3"], capture_output=True, timeout=600, cwd=str(ROOT))  # fmt: skip
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    assert (tmp_path / "t.tsv").read_bytes() == _native.nj_support_header() + want_tsv
