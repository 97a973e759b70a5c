"""The neighbour-joining tree of locus rows on the device (include/kp_spec.h, NJ; kaptive_amd/csrc/kp_dist_nj.hip) against the NumPy
restatement in tests/nj_util.py: taxa and records as bytes -- node ids, order and every bit of every length.  Random populations at
every shape at which the tile epilogue, the row sums or the pick take another path; identical rows, where every Q ties and only the
slot order decides; a planted additive tree; the state the call must leave alone; what it allocates; its refusals; then the whole
route on the 9-locus miniature database: ``Serotyper(db, distances=True)`` over two batches, the command line with ``--nj`` alone,
beside every other table, with ``--db``, a run without the flag, and two devices."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from tests import clusters_util as CU
from tests import distances_util as D
from tests import nj_util as NJ
from tests import tree_util as TU
from tests.distances_util import CH, SPLIT, T, Run, _count_handles, _device_count, _write_inputs

pytestmark = pytest.mark.gpu

ROWS = (0, 1, 2, 3, 4, 5, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5, 5 * T + 3)
BLOCKS = (1, 4, 4 * CH + 1)
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
    (gt, gn), (wt, wn) = got, want
    assert gt.dtype == np.int32 and gn.dtype == _native.NJ_NODE_DTYPE, what
    assert gt.tobytes() == wt.tobytes(), f"{what}: taxa {gt.tolist()} on the device, {wt.tolist()} wanted"
    if gn.tobytes() != wn.tobytes():
        i = next((i for i in range(min(len(gn), len(wn))) if gn[i].tobytes() != wn[i].tobytes()), min(len(gn), len(wn)))
        raise AssertionError(f"{what}: {len(gn)} records on the device, {len(wn)} wanted; record {i}: {gn[i] if i < len(gn) else None} against {wn[i] if i < len(wn) else None}")


# ---- 1. random populations: every shape, every min_compared ------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", BLOCKS)
@pytest.mark.parametrize("R", ROWS)
def test_tree_against_numpy(ctx, R, nb):
    codes = D.population(np.random.default_rng([R, nb]), R, nb)
    first = {}
    with _native.Distances(ctx, _matrix(codes)) as d:
        for mc in (0, 1, 16 * nb // 4):
            want = NJ.tree(codes, mc)
            got = d.nj(mc)
            _same(got, want, f"R {R}, NB {nb}, min_compared {mc}")
            n = len(got[0])
            assert d.nj_taxa(mc) == n and len(got[1]) == (0 if n < 2 else 1 if n == 2 else n - 2) and not got[1]["pad"].any()
            if R >= 16:
                assert 2 not in got[0] and 3 not in got[0]  # the all-GAP and the all-N row are no taxa
            first[mc] = got[0].tobytes() + got[1].tobytes()
    with _native.Distances(ctx, _matrix(codes)) as again:  # a second handle, the calls in another order: the same bytes
        for mc in reversed(list(first)):
            got = again.nj(mc)
            assert got[0].tobytes() + got[1].tobytes() == first[mc], mc


# ---- 2. every row identical: every Q ties ------------------------------------------------------------------------------------------------
def test_identical_rows_give_the_caterpillar_of_the_tie_rule(ctx):
    R, nb = 3 * T + 5, 4 * CH + 1
    codes = np.tile(np.random.default_rng(21).integers(0, 4, 16 * nb).astype(np.uint8), (R, 1))
    with _native.Distances(ctx, _matrix(codes)) as d:
        taxa, nodes = d.nj(1)
    n = R
    assert taxa.tolist() == list(range(n)) and len(nodes) == n - 2
    # slots (0, 1) every time: the new node against the node the last slot gave up -- a tie broken by block or lane order fails here
    want = [(0, 1, -1)] + [(n + r - 1, n - r, -1) for r in range(1, n - 3)] + [(2 * n - 4, 3, 2)]
    assert list(zip(nodes["a"].tolist(), nodes["b"].tolist(), nodes["c"].tolist())) == want
    assert not nodes["la"].any() and not nodes["lb"].any() and not nodes["lc"].any() and not np.signbit(nodes["la"]).any()
    _same((taxa, nodes), NJ.tree(codes, 1), "identical rows")


# ---- 3. a planted additive tree --------------------------------------------------------------------------------------------------------------
def test_additive_tree_on_the_device(ctx):
    n = 2 * T + 1
    codes, planted, mutations, W = NJ.additive(np.random.default_rng(33), n)
    with _native.Distances(ctx, _matrix(codes)) as d:
        taxa, nodes = d.nj(1)
    _same((taxa, nodes), NJ.tree(codes, 1), "additive tree")
    assert taxa.tolist() == list(range(n)) and NJ.splits(n, nodes) == planted and len(planted) == n - 3
    assert abs(NJ.total_length(nodes) - mutations / W) <= 1e-12


# ---- 4. state ------------------------------------------------------------------------------------------------------------------------------------
def test_the_state_a_tree_leaves_alone(ctx):
    lib = _native.lib()
    codes = D.population(np.random.default_rng(3), 2 * T + 1, 5)
    with _native.Distances(ctx, _matrix(codes)) as d:
        want = d.pairs(SPLIT, 1)
        n = d.count(SPLIT, 1)
        tree = d.nj(1)
        out = np.zeros(n, _native.DIST_PAIR_DTYPE)
        assert lib.kp_dist_pairs(ctx._h, d._h, _p(out), C.c_int64(n)) == 0 and out.tobytes() == want.tobytes() and n == len(want) > 0  # count -> nj -> pairs
        forest, clusters = d.tree(1), d.clusters(CU.LEVELS, 1)
        again = d.nj(1)
        forest2, clusters2 = d.tree(1), d.clusters(CU.LEVELS, 1)
        assert forest[0].tobytes() == forest2[0].tobytes() and forest[1].tobytes() == forest2[1].tobytes()  # tree and clusters around it
        assert clusters[0].tobytes() == clusters2[0].tobytes() and clusters[1].tobytes() == clusters2[1].tobytes()
        assert again[0].tobytes() == tree[0].tobytes() and again[1].tobytes() == tree[1].tobytes()  # nj twice
        _same(tree, NJ.tree(codes, 1), "state")
        assert forest[0].tobytes() == TU.forest(codes, 1)[0].tobytes()


# ---- 5. allocation -------------------------------------------------------------------------------------------------------------------------------
def test_the_matrix_does_not_stay_with_the_handle(ctx):
    """``device_allocations`` counts the buffers that had to grow.  The handle's O(n) tables are made once, by the first call, and
    the matrix and the partials are new buffers of every call: nothing grows, whatever the order of the sizes -- a matrix kept with
    the handle would have to grow for the second, larger tree."""
    codes = D.population(np.random.default_rng(5), 3 * T + 5, 4 * CH + 1)
    before = _native.device_allocations()
    with _native.Distances(ctx, _matrix(codes)) as d:
        few, many = d.nj(codes.shape[1] * 9 // 10), d.nj(1)  # (a taxon of the first holds a base in 95 % of the columns)
        assert 2 <= len(few[0]) < len(many[0])
        assert _native.device_allocations() == before
        assert d.nj(1)[1].tobytes() == many[1].tobytes()
    assert _native.device_allocations() == before


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    lib = _native.lib()
    rng = np.random.default_rng(1)
    codes = rng.integers(0, 4, (5, 48)).astype(np.uint8)
    blocks = _matrix(codes)
    want = NJ.tree(codes, 1)
    assert len(want[0]) == 5 and len(want[1]) == 3
    h = C.c_void_p()
    assert lib.kp_dist_create(ctx._h, _p(blocks), C.c_int32(5), C.c_int64(3), C.byref(h)) == 0 and h.value
    taxa, nodes, nt, nn = np.full(5, -7, np.int32), np.zeros(3, _native.NJ_NODE_DTYPE), C.c_int32(-7), C.c_int64(-7)

    def call(c=ctx._h, handle=h, t=_p(taxa), cap_t=5, count_t=C.byref(nt), nd=_p(nodes), cap_n=3, count_n=C.byref(nn), mc=1):
        return lib.kp_dist_nj(c, handle, C.c_int32(mc), t, C.c_int64(cap_t), count_t, nd, C.c_int64(cap_n), count_n)

    for kw, why in ((dict(c=None), None), (dict(handle=None), b"null"), (dict(count_t=None), b"null"), (dict(count_n=None), b"null record count"),
                    (dict(t=None), b"null taxon table"), (dict(nd=None), b"null record table"), (dict(cap_t=4), b"fewer taxa"), (dict(cap_t=-1), b"negative"),
                    (dict(cap_n=2), b"fewer records"), (dict(cap_n=0, nd=None), b"fewer records"), (dict(cap_t=0, t=None), b"fewer taxa")):  # fmt: skip
        assert call(**kw) == EINVAL, kw
        if why is not None:
            assert why in lib.kp_last_error(ctx._h), (kw, lib.kp_last_error(ctx._h))
    assert (taxa == -7).all() and not nodes.view(np.uint8).any()  # a refused call stores nothing
    assert call(t=None, cap_t=0, nd=None, cap_n=0, count_n=None) == 0 and nt.value == 5  # the counting form
    assert (taxa == -7).all()
    assert call() == 0 and nt.value == 5 and nn.value == 3 and taxa.tobytes() == want[0].tobytes() and nodes.tobytes() == want[1].tobytes()
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
        closed.nj()  # a destroyed handle is a null handle to the library
    for rows, nb in ((0, 0), (0, 3), (1, 3)):  # valid: no record
        with _native.Distances(ctx, np.zeros((rows, nb), np.uint64)) as d:
            t, n = d.nj()
            assert t.tolist() == list(range(rows)) and len(n) == 0


def test_more_taxa_than_the_limit_are_refused_by_this_call_alone(ctx):
    lib = _native.lib()
    R = _native.NJ_MAX_TAXA + 1
    before = _native.device_allocations()
    with _native.Distances(ctx, np.zeros((R, 1), np.uint64)) as d:  # sixteen bases a row: every row a taxon
        assert d.nj_taxa(1) == R  # the counting form counts and does not refuse
        taxa, nodes, nt, nn = np.full(R, -7, np.int32), np.zeros(R - 2, _native.NJ_NODE_DTYPE), C.c_int32(-7), C.c_int64(-7)
        assert lib.kp_dist_nj(ctx._h, d._h, C.c_int32(1), _p(taxa), C.c_int64(R), C.byref(nt), _p(nodes), C.c_int64(R - 2), C.byref(nn)) == EINVAL
        assert b"KP_NJ_MAX_TAXA" in lib.kp_last_error(ctx._h) and nt.value == R and nn.value == 0
        assert (taxa == -7).all() and not nodes.view(np.uint8).any()
        with pytest.raises(Exception, match="KP_NJ_MAX_TAXA"):
            d.nj(1)
        assert d.count(0, 1) == R * (R - 1) // 2  # the other calls keep their own limit
    assert _native.device_allocations() == before


# ---- 7. the whole route on the miniature database ---------------------------------------------------------------------------------------------
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
        text, skipped = got.nj_tsv(ctx, mc)
        assert text == NJ.run_tsv(want, mc) and skipped == []
        for L in got.loci():
            idx, taxa, nodes = got.nj(ctx, L, mc)
            _same((taxa, nodes), NJ.tree(D.unpack(want.locus_matrix(L)[1]), mc), f"locus {L}, min_compared {mc}")
            assert idx.tolist() == want.locus_matrix(L)[0].tolist()
    lines = got.nj_tsv(ctx)[0].splitlines()
    assert [ln.split(b"\t")[:3] for ln in lines] == [[run.db.loci.ids[L].encode(), str(k).encode(), str(k).encode()] for L, k in ((0, 5), (3, 4), (6, 3))]
    assert all(ln.endswith(b");") and ln.count(b"(") == ln.count(b")") for ln in lines) and got.nj_tsv(ctx, 10**6) == (b"", [])
    assert [ln.count(b"(") for ln in lines] == [3, 2, 1] and all(ln.count(n.encode()) == 1 for ln, L in zip(lines, (0, 3, 6)) for n in run.ids if n.startswith(f"L{L}_"))
    from tests.test_gpu_distances import _want_tsv

    assert got.tsv(ctx) == _want_tsv(want) and got.clusters_tsv(ctx) == CU.run_tsv(want) and got.newick_tsv(ctx) == TU.run_newick_tsv(want)  # the other tables of the same handles
    got.close()


def test_command_line(run, tmp_path, monkeypatch, capsys):
    from kaptive_amd.cli import main
    from kaptive_amd.synth import make_db
    from tests.test_gpu_distances import _want_tsv

    db_path, paths = _write_inputs(run.db, run.genomes, tmp_path)
    made = _count_handles(monkeypatch)
    nj = _native.nj_header() + NJ.run_tsv(run.want_rows)
    assert nj.count(b"\n") == 1 + 3
    # a run without the flag: the files every other run must reproduce
    others = ("distances", "clusters", "mst", "newick", "sites", "snp-alignment")
    flags = lambda tag: [x for f in others for x in (f"--{f}", str(tmp_path / f"{f}.{tag}.tsv"))]  # noqa: E731
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "plain.tsv"), *flags("0")]) == 0
    plain = (tmp_path / "plain.tsv").read_bytes()
    base = [(tmp_path / f"{f}.0.tsv").read_bytes() for f in others]
    assert plain.endswith(run.tsv) and base[0] == _native.DISTANCES_HEADER + _want_tsv(run.want_rows) and base[3] == _native.newick_header() + TU.run_newick_tsv(run.want_rows)
    assert not list(tmp_path.glob("*nj*"))
    # the flag alone
    del made[:]
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o1.tsv"), "--nj", str(tmp_path / "t1.tsv"), "--batch-size", "7"]) == 0
    assert (tmp_path / "t1.tsv").read_bytes() == nj and (tmp_path / "o1.tsv").read_bytes() == plain
    assert len(made) == 3  # a handle per locus
    # beside every other table: each is what it is alone, and each matrix is uploaded once
    del made[:]
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o2.tsv"), "--nj", str(tmp_path / "t2.tsv"), *flags("2"), "--batch-size", "5"]) == 0
    assert (tmp_path / "t2.tsv").read_bytes() == nj and (tmp_path / "o2.tsv").read_bytes() == plain
    assert [(tmp_path / f"{f}.2.tsv").read_bytes() for f in others] == base and len(made) == 3
    # --min-compared moves the bar of a taxon
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o3.tsv"), "--nj", str(tmp_path / "t3.tsv"), "--min-compared", "1000000"]) == 0
    assert (tmp_path / "t3.tsv").read_bytes() == _native.nj_header()  # nobody holds a million bases: no taxon, no line
    assert capsys.readouterr().err.count("--nj") == 0  # and nothing was skipped
    # a second database: a table per database
    o_path = str(make_db("kpsc_o", seed=8).save(tmp_path / "o.npz"))
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "both.tsv"), "--nj", str(tmp_path / "both.t.tsv")]) == 0
    assert (tmp_path / "both.t.kpsc_k.tsv").read_bytes() == nj and (tmp_path / "both.t.kpsc_o.tsv").read_bytes().startswith(_native.nj_header())
    assert (tmp_path / "both.kpsc_k.tsv").read_bytes() == plain
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "x.tsv"), "--nj", "-"]) == 1  # stdout is refused
    assert not (tmp_path / "x.tsv").exists()


def test_a_locus_beyond_the_limit_is_skipped_with_one_line(run, monkeypatch, capsys):
    """``nj_tsv`` leaves a locus of more than NJ_MAX_TAXA taxa out and names it; the command line says so on stderr and goes on."""
    from kaptive_amd.cli import _RunDistances

    rows, ctx = run.typer.locus_rows, run.typer.engine.ctx
    monkeypatch.setattr(_native, "NJ_MAX_TAXA", 4)  # locus 0 has five taxa
    text, skipped = rows.nj_tsv(ctx)
    assert skipped == [0] and text == b"".join(NJ.run_tsv(run.want_rows).splitlines(keepends=True)[1:])
    assert _RunDistances._lines(rows, (text, skipped)) == text
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "--nj" in err and run.db.loci.ids[0] in err
    rows.close()


@pytest.mark.skipif("_device_count() < 2")
def test_command_line_on_two_devices(run, tmp_path):
    import subprocess
    import sys

    db_path, paths = _write_inputs(run.db, run.genomes, tmp_path)
    from tests.conftest import ROOT

    r = subprocess.run([sys.executable, "-m", "kaptive_amd", "assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--nj", str(tmp_path / "t.tsv"),
                        "--devices", "0,1", "--batch-size", "3"], capture_output=True, timeout=600, cwd=str(ROOT))  # fmt: skip
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    assert (tmp_path / "t.tsv").read_bytes() == _native.nj_header() + NJ.run_tsv(run.want_rows)
