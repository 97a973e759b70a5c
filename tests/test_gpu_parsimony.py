"""Small parsimony on the neighbour-joining tree on the device (include/kp_spec.h, PARSIMONY; kaptive_amd/csrc/kp_dist_pars.hip) against
the set restatement in tests/parsimony_util.py: the site and the change records as bytes -- on NJ's own trees and on hand-made record
lists, at every taxa count and width at which the pass takes another shape, with the planted rows of ``D.population``, a column nobody
holds a base in and padding --; the planted additive tree and the planted homoplasy; two handles with the calls in another order; the
state the call must leave alone; what it allocates; its refusals; then the whole route on the 9-locus miniature database."""

from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from kaptive_amd import _native
from tests import clusters_util as CU
from tests import distances_util as D
from tests import nj_util as NJ
from tests import parsimony_util as P
from tests.distances_util import CH, SPLIT, T, Run, _count_handles, _device_count, _write_inputs

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4


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
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (what, len(got), len(want), got[:8].tolist(), want[:8].tolist())


@functools.lru_cache(maxsize=None)
def _codes(n, nb):
    """Rows of which exactly n are taxa.  From sixteen rows on ``D.population`` with its planted rows -- the all-GAP row, the all-N row
    and whoever else holds too little are no taxa, and relatives of row 10 make up for them --; below that, random relatives and one
    GAP row.  Column 5 holds a base in no taxon, and the last three columns are padding."""
    rng = np.random.default_rng([n, nb, 11])
    cols = 16 * nb

    def finish(c):
        c[:, 5] = np.where(np.arange(len(c)) % 2 == 0, D.N, D.GAP)
        if cols > 16:
            c[:, cols - 3 :] = D.GAP
        return c

    if n >= 16:
        codes = D.population(rng, n, nb)
        lacking = n - len(NJ.taxa_of(finish(codes.copy()), 1))
        more = np.tile(codes[10], (lacking, 1))
        for r in range(lacking):
            at = rng.integers(0, cols, 6)
            more[r, at] = (more[r, at] + rng.integers(1, 4, 6)) % 4
        codes = np.concatenate([codes[:7], more, codes[7:]])
    else:
        founder = rng.integers(0, 4, cols).astype(np.uint8)
        codes = np.tile(founder, (n + 1, 1))
        for r in range(n):
            at = rng.integers(0, cols, 5)
            codes[r, at] = (codes[r, at] + rng.integers(1, 4, 5)) % 4
            codes[r, int(rng.integers(0, cols))] = D.N
        codes[[1, n]] = codes[[n, 1]]  # the non-taxon row in the middle
        codes[1] = D.GAP
    codes = finish(codes)
    assert len(NJ.taxa_of(codes, 1)) == n < len(codes)
    return codes


@functools.lru_cache(maxsize=None)
def _own(n, nb):
    """The yardstick on NJ's own tree, made once: (taxa, nodes, sites, changes)."""
    return P.of_codes(_codes(n, nb), 1)


# ---- 1. against the yardstick: every taxa count, every width, own and hand-made trees -----------------------------------------------------------
@pytest.mark.parametrize("nb", (1, 4, 5, 4 * CH + 1))
@pytest.mark.parametrize("n", (2, 3, 4, 5, T - 1, T, T + 1, 2 * T + 1))
def test_against_the_yardstick(ctx, n, nb):
    codes = _codes(n, nb)
    taxa, nodes, sites, changes = _own(n, nb)
    assert len(sites) > 0 and len(changes) >= len(sites) and 5 not in sites["column"]
    rng = np.random.default_rng([n, nb])
    trees = [("random", P.tree_of(n, rng))] + ([("caterpillar", P.tree_of(n, None, "caterpillar"))] if n in (4, 5, T + 1) else [])
    with _native.Distances(ctx, _matrix(codes)) as d:
        got_taxa, got_nodes = d.nj(1)
        assert got_taxa.tobytes() == taxa.tobytes() and got_nodes.tobytes() == nodes.tobytes()
        s, c = d.nj_parsimony(1, got_nodes)
        _same(s, sites, f"sites, n {n}, NB {nb}"), _same(c, changes, f"changes, n {n}, NB {nb}")
        for what, ref in trees:
            ws, wc = P.parsimony(codes, taxa, ref)
            s, c = d.nj_parsimony(1, ref)
            _same(s, ws, f"sites, {what}, n {n}, NB {nb}"), _same(c, wc, f"changes, {what}, n {n}, NB {nb}")
        s, c = d.nj_parsimony(1, got_nodes)  # a shorter list behind a longer one, a longer one behind a shorter one: the same bytes again
        _same(s, sites, "sites again"), _same(c, changes, "changes again")


def test_rows_that_are_no_taxa_and_tiny_matrices(ctx):
    for R, n in ((0, 0), (1, 1), (3, 1), (3, 0)):
        codes = np.full((R, 32), D.GAP, np.uint8)
        codes[:n] = np.random.default_rng(R).integers(0, 4, (n, 32))
        with _native.Distances(ctx, _matrix(codes)) as d:
            s, c = d.nj_parsimony(1, np.zeros(0, _native.NJ_NODE_DTYPE))
            assert len(s) == 0 == len(c) and s.dtype == _native.PARS_SITE_DTYPE and c.dtype == _native.PARS_CHANGE_DTYPE
    same = np.tile(np.random.default_rng(9).integers(0, 4, 80).astype(np.uint8), (T + 3, 1))  # identical rows: a tree, no step
    with _native.Distances(ctx, _matrix(same)) as d:
        s, c = d.nj_parsimony(1, d.nj(1)[1])
        assert len(s) == 0 == len(c)


# ---- 2. planted trees ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (6, 19, T + 2))
def test_planted_trees(ctx, n):
    rng = np.random.default_rng([n, 5])
    codes, planted, at, (a, b) = P.planted_homoplasy(rng, n)
    taxa, nodes, sites, changes = P.of_codes(codes, 1)
    with _native.Distances(ctx, _matrix(codes)) as d:
        got_taxa, got_nodes = d.nj(1)
        assert len(got_taxa) == n and got_nodes.tobytes() == nodes.tobytes() and NJ.splits(n, got_nodes) == planted
        s, c = d.nj_parsimony(1, got_nodes)
    _same(s, sites, "sites"), _same(c, changes, "changes")
    under, everyone = P.below(n, got_nodes), frozenset(range(n))
    extra = s[s["column"] == at]
    assert len(extra) == 1 and extra["steps"][0] == 2 and bin(int(extra["alleles"][0])).count("1") == 2  # excess 1
    assert sorted(c["node"][c["column"] == at].tolist()) == [a, b]
    rest = s[s["column"] != at]
    assert len(rest) >= 3 * (2 * n - 3) and (rest["steps"] == 1).all() and all(bin(int(x)).count("1") == 2 for x in rest["alleles"])
    for r in c[c["column"] != at]:  # one change a column, on the branch whose split is the planted one
        assert frozenset([under[int(r["node"])], everyone - under[int(r["node"])]]) == P.bipartition(codes[:, int(r["column"])])
    assert len(c) == len(rest) + 2


# ---- 3. determinism; 4. state; 5. allocation ---------------------------------------------------------------------------------------------------------
def test_two_handles_with_the_calls_in_another_order(ctx):
    n, nb = T + 1, 5
    codes = _codes(n, nb)
    taxa, nodes, sites, changes = _own(n, nb)
    cat = P.tree_of(n, None, "caterpillar")
    with _native.Distances(ctx, _matrix(codes)) as one, _native.Distances(ctx, _matrix(codes)) as two:
        a1 = one.nj_parsimony(1, nodes)
        one.sites(), one.nj_support(1, nodes, 2)
        b1 = one.nj_parsimony(1, cat)
        b2 = two.nj_parsimony(1, cat)
        two.pairs(SPLIT, 1), two.nj(1)
        a2 = two.nj_parsimony(1, nodes)
    for x, y in ((a1, a2), (b1, b2)):
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
    _same(a1[0], sites, "sites"), _same(a1[1], changes, "changes")
    assert a1[1].tobytes() != b1[1].tobytes()


def test_the_state_a_parsimony_call_leaves_alone(ctx):
    lib = _native.lib()
    codes = D.population(np.random.default_rng(3), 2 * T + 1, 5)
    with _native.Distances(ctx, _matrix(codes)) as d:
        want = d.pairs(SPLIT, 1)
        n = d.count(SPLIT, 1)
        tree = d.nj(1)
        forest, clusters, sites = d.tree(1), d.clusters(CU.LEVELS, 1), d.sites()
        counted = d.nj_support(1, tree[1], 3)
        s, c = d.nj_parsimony(1, tree[1])
        out = np.zeros(n, _native.DIST_PAIR_DTYPE)
        assert lib.kp_dist_pairs(ctx._h, d._h, _p(out), C.c_int64(n)) == 0 and out.tobytes() == want.tobytes() and n == len(want) > 0  # count -> parsimony -> pairs
        out_sites = np.zeros(len(sites), _native.SITE_DTYPE)
        assert lib.kp_dist_sites(ctx._h, d._h, _p(out_sites), C.c_int64(len(sites))) == 0 and out_sites.tobytes() == sites.tobytes() and len(sites) > 0
        forest2, clusters2, again = d.tree(1), d.clusters(CU.LEVELS, 1), d.nj(1)
        assert forest[0].tobytes() == forest2[0].tobytes() and forest[1].tobytes() == forest2[1].tobytes()
        assert clusters[0].tobytes() == clusters2[0].tobytes() and clusters[1].tobytes() == clusters2[1].tobytes()
        assert again[0].tobytes() == tree[0].tobytes() and again[1].tobytes() == tree[1].tobytes()
        assert counted.tobytes() == d.nj_support(1, tree[1], 3).tobytes()
        # the other calls leave the last parsimony alone: the getters still hand out its records
        s2, c2 = np.zeros(len(s), _native.PARS_SITE_DTYPE), np.zeros(len(c), _native.PARS_CHANGE_DTYPE)
        assert lib.kp_dist_pars_sites(ctx._h, d._h, _p(s2), C.c_int64(len(s2))) == 0 and lib.kp_dist_pars_changes(ctx._h, d._h, _p(c2), C.c_int64(len(c2))) == 0
        assert s2.tobytes() == s.tobytes() and c2.tobytes() == c.tobytes() and len(s) > 0
    w = P.of_codes(codes, 1)
    _same(s, w[2], "sites"), _same(c, w[3], "changes")
    # every site of the parsimony is a site of SITES among the taxa, and the other way round
    held = [len({int(x) for x in codes[w[0], j] if x < 4}) for j in range(codes.shape[1])]
    assert s["column"].tolist() == [j for j, k in enumerate(held) if k >= 2]


def test_nothing_of_a_call_but_its_records_stays_with_the_handle(ctx):
    codes = D.population(np.random.default_rng(5), 3 * T + 5, 4 * CH + 1)
    before = _native.device_allocations()
    with _native.Distances(ctx, _matrix(codes)) as d:
        mc = codes.shape[1] * 9 // 10
        few, many = d.nj(mc), d.nj(1)
        assert 4 <= len(few[0]) < len(many[0])
        a = d.nj_parsimony(mc, few[1])
        b = d.nj_parsimony(1, many[1])
        assert len(b[1]) > len(a[1]) > 0 and _native.device_allocations() == before
        a2, b2 = d.nj_parsimony(mc, few[1]), d.nj_parsimony(1, many[1])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a + b, a2 + b2))
        assert _native.device_allocations() == before
    assert _native.device_allocations() == before
    _same(a[0], P.parsimony(codes, few[0], few[1])[0], "few taxa")


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    lib = _native.lib()
    codes = _codes(5, 4)
    blocks = _matrix(codes)
    taxa, nodes, sites, changes = _own(5, 4)
    assert len(taxa) == 5 and len(nodes) == 3
    h = C.c_void_p()
    assert lib.kp_dist_create(ctx._h, _p(blocks), C.c_int32(len(codes)), C.c_int64(4), C.byref(h)) == 0 and h.value
    ns, nc = C.c_int64(-7), C.c_int64(-7)
    s, c = np.zeros(len(sites), _native.PARS_SITE_DTYPE), np.zeros(len(changes), _native.PARS_CHANGE_DTYPE)
    s["column"] = -7
    longer = np.concatenate([nodes, nodes[:1]])  # (a table of four records for the count that reads four)
    last =lambda: lib.kp_last_error(ctx._h)  # noqa: E731

    def call(c_=ctx._h, handle=h, ref=_p(nodes), n_ref=3, a=C.byref(ns), b=C.byref(nc), mc=1):
        return lib.kp_dist_nj_parsimony(c_, handle, C.c_int32(mc), ref, C.c_int64(n_ref), a, b)

    # a getter before the call
    assert lib.kp_dist_pars_sites(ctx._h, h, _p(s), C.c_int64(len(s))) == ESTATE and b"must come first" in last()
    assert lib.kp_dist_pars_changes(ctx._h, h, _p(c), C.c_int64(len(c))) == ESTATE and b"must come first" in last()

    def bad(*rows):
        out = nodes.copy()
        for t, (x, y, z) in enumerate(rows):
            out[t]["a"], out[t]["b"], out[t]["c"] = x, y, z
        return out

    lists = {"a child used twice": bad((0, 1, -1), (5, 1, -1), (6, 4, 3)), "a forward reference": bad((0, 6, -1), (5, 2, -1), (1, 4, 3)),
             "a ternary record in the middle": bad((0, 1, 2), (5, 3, -1), (6, 4, -1)), "a binary last record": bad((0, 1, -1), (5, 2, -1), (6, 4, -1)),
             "an id outside": bad((0, 1, -1), (5, 2, -1), (6, 4, 9)), "a negative id": bad((-1, 1, -1), (5, 2, -1), (6, 4, 3))}  # fmt: skip
    for kw, why in ((dict(c_=None), None), (dict(handle=None), b"null"), (dict(a=None), b"null"), (dict(b=None), b"null"), (dict(ref=None), b"null record table"),
                    (dict(n_ref=-1), b"negative"), (dict(n_ref=2), b"no tree"), (dict(n_ref=4, ref=_p(longer)), b"no tree"), (dict(n_ref=0, ref=None), b"records of the tree"),
                    (dict(mc=16 * 4), b"records of the tree"), *((dict(ref=_p(v)), b"no tree") for v in lists.values())):  # fmt: skip
        assert call(**kw) == EINVAL, kw
        if why is not None:
            assert why in last(), (kw, last())
    four = P.tree_of(4)  # a tree, but of other taxa than the handle's: a wrong n_ref
    assert call(ref=_p(four), n_ref=2) == EINVAL and b"records of the tree" in last()
    assert ns.value == -7 == nc.value  # a refused call stores nothing
    assert lib.kp_dist_pars_sites(ctx._h, h, _p(s), C.c_int64(len(s))) == ESTATE  # and is no call
    # the call, then the getters' own refusals
    assert call() == 0 and ns.value == len(sites) > 1 and nc.value == len(changes)
    for getter, table, n in ((lib.kp_dist_pars_sites, s, len(sites)), (lib.kp_dist_pars_changes, c, len(changes))):
        assert getter(ctx._h, h, _p(table), C.c_int64(-1)) == EINVAL and getter(ctx._h, h, _p(table), C.c_int64(n - 1)) == EINVAL and b"fewer" in last()
        assert getter(ctx._h, h, None, C.c_int64(n)) == EINVAL and getter(None, h, _p(table), C.c_int64(n)) == EINVAL and getter(ctx._h, None, _p(table), C.c_int64(n)) == EINVAL
    assert (s["column"] == -7).all() and not c.view(np.uint8).any()  # nothing was written
    assert call(ref=_p(lists["a child used twice"])) == EINVAL  # a refused call leaves the results of the call before it
    assert lib.kp_dist_pars_sites(ctx._h, h, _p(s), C.c_int64(len(s))) == 0 and lib.kp_dist_pars_changes(ctx._h, h, _p(c), C.c_int64(len(c) + 3)) == 0
    assert s.tobytes() == sites.tobytes() and c.tobytes() == changes.tobytes()
    lib.kp_dist_destroy(h)
    if _device_count() > 1:  # a handle of another device
        other = _native.Context(1)
        try:
            with _native.Distances(other, blocks) as foreign:
                assert call(handle=foreign._h) == EINVAL and b"another device" in last()
        finally:
            other.close()
    closed = _native.Distances(ctx, blocks)
    closed.close()
    with pytest.raises(Exception):
        closed.nj_parsimony(1, nodes)


def test_more_taxa_than_the_limit_are_refused(ctx):
    R = _native.NJ_MAX_TAXA + 1
    before = _native.device_allocations()
    with _native.Distances(ctx, np.zeros((R, 1), np.uint64)) as d:  # sixteen bases a row: every row a taxon
        with pytest.raises(Exception, match="KP_NJ_MAX_TAXA"):
            d.nj_parsimony(1, P.tree_of(R, None, "caterpillar"))
        with pytest.raises(Exception, match="KP_NJ_MAX_TAXA"):
            d.nj_parsimony(1, np.zeros(R + 5, _native.NJ_NODE_DTYPE))
        assert d.nj_taxa(1) == R  # (the counting form counts and does not refuse)
    assert _native.device_allocations() == before


# ---- 7. the whole route on the miniature database ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run():
    r = Run()
    yield r
    r.close()


@pytest.fixture(scope="module")
def want_tsv(run):
    return P.run_tsv(run.want_rows)


def test_serotyper_over_two_batches(run, want_tsv):
    got, want = run.typer.locus_rows, run.want_rows
    ctx = run.typer.engine.ctx
    homoplasy, changed = want_tsv
    assert homoplasy.count(b"\n") >= 3 and changed.count(b"\n") >= homoplasy.count(b"\n")
    assert got.nj_homoplasy_tsv(ctx, D.MIN_COMPARED) == (homoplasy, []) and got.nj_changes_tsv(ctx) == (changed, [])
    assert {ln.split(b"\t")[0] for ln in changed.splitlines()} == {run.db.loci.ids[L].encode() for L in (0, 3, 6)}
    for L in got.loci():
        idx, taxa, nodes, sites, changes = got.nj_parsimony(ctx, L)
        w = P.of_codes(D.unpack(want.locus_matrix(L)[1]), D.MIN_COMPARED)
        assert taxa.tobytes() == w[0].tobytes() and nodes.tobytes() == w[1].tobytes() and idx.tolist() == want.locus_matrix(L)[0].tolist()
        _same(sites, w[2], f"locus {L}"), _same(changes, w[3], f"locus {L}")
    assert got.nj_homoplasy_tsv(ctx, 10**6) == (b"", []) == got.nj_changes_tsv(ctx, 10**6)  # nobody holds a million bases: no taxon, no tree
    assert got.nj_tsv(ctx)[0] == NJ.run_tsv(want)  # the tree of the same handles
    got.close()


def test_a_locus_beyond_the_limit_is_skipped(run, monkeypatch):
    rows, ctx = run.typer.locus_rows, run.typer.engine.ctx
    want = P.run_tsv(run.want_rows)
    monkeypatch.setattr(_native, "NJ_MAX_TAXA", 4)  # locus 0 has five taxa
    first = run.db.loci.ids[0].encode() + b"\t"
    for (text, skipped), full in ((rows.nj_homoplasy_tsv(ctx), want[0]), (rows.nj_changes_tsv(ctx), want[1])):
        assert skipped == [0] and text == b"".join(ln for ln in full.splitlines(keepends=True) if not ln.startswith(first)) and text
    rows.close()


def test_command_line(run, want_tsv, tmp_path, monkeypatch, capsys):
    from kaptive_amd.cli import main
    from kaptive_amd.synth import make_db

    db_path, paths = _write_inputs(run.db, run.genomes, tmp_path)
    made = _count_handles(monkeypatch)
    homoplasy, changed = _native.nj_homoplasy_header() + want_tsv[0], _native.nj_changes_header() + want_tsv[1]
    nj = _native.nj_header() + NJ.run_tsv(run.want_rows)
    # a run without the flags: the files every other run must reproduce
    others = ("distances", "clusters", "mst", "newick", "nj", "sites", "snp-alignment")
    flags = lambda tag: [x for f in others for x in (f"--{f}", str(tmp_path / f"{f}.{tag}.tsv"))]  # noqa: E731
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "plain.tsv"), *flags("0")]) == 0
    plain = (tmp_path / "plain.tsv").read_bytes()
    base = [(tmp_path / f"{f}.0.tsv").read_bytes() for f in others]
    assert plain.endswith(run.tsv) and base[4] == nj and not list(tmp_path.glob("*changes*")) and not list(tmp_path.glob("*homoplasy*"))
    # each flag alone beside the tree
    del made[:]
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o1.tsv"), "--nj", str(tmp_path / "t1.tsv"), "--nj-changes", str(tmp_path / "changes1.tsv"), "--batch-size", "7"]) == 0
    assert (tmp_path / "changes1.tsv").read_bytes() == changed and (tmp_path / "t1.tsv").read_bytes() == nj and (tmp_path / "o1.tsv").read_bytes() == plain
    assert len(made) == 3 and not list(tmp_path.glob("*homoplasy*"))  # a handle per locus
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o2.tsv"), "--nj", str(tmp_path / "t2.tsv"), "--nj-homoplasy", str(tmp_path / "homoplasy2.tsv")]) == 0
    assert (tmp_path / "homoplasy2.tsv").read_bytes() == homoplasy and (tmp_path / "t2.tsv").read_bytes() == nj
    # both beside every other table and the bootstrap: each is what it is alone, and each matrix is uploaded once
    del made[:]
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o3.tsv"), *flags("3"), "--nj-changes", str(tmp_path / "changes3.tsv"), "--nj-homoplasy",
                 str(tmp_path / "homoplasy3.tsv"), "--batch-size", "5"]) == 0  # fmt: skip
    assert (tmp_path / "changes3.tsv").read_bytes() == changed and (tmp_path / "homoplasy3.tsv").read_bytes() == homoplasy and (tmp_path / "o3.tsv").read_bytes() == plain
    assert [(tmp_path / f"{f}.3.tsv").read_bytes() for f in others] == base and len(made) == 3
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o4.tsv"), "--nj", str(tmp_path / "t4.tsv"), "--nj-bootstrap", "3", "--nj-transfer", "--nj-changes",
                 str(tmp_path / "changes4.tsv")]) == 0  # fmt: skip
    assert (tmp_path / "changes4.tsv").read_bytes() == changed and (tmp_path / "t4.tsv").read_bytes().startswith(_native.nj_support_header())
    assert capsys.readouterr().err.count("--nj") == 0  # nothing was skipped
    # a second database: a table per database
    o_path = str(make_db("kpsc_o", seed=8).save(tmp_path / "o.npz"))
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "both.tsv"), "--nj", str(tmp_path / "both.t.tsv"), "--nj-changes", str(tmp_path / "both.c.tsv"),
                 "--nj-homoplasy", str(tmp_path / "both.h.tsv")]) == 0  # fmt: skip
    assert (tmp_path / "both.c.kpsc_k.tsv").read_bytes() == changed and (tmp_path / "both.h.kpsc_k.tsv").read_bytes() == homoplasy
    assert (tmp_path / "both.c.kpsc_o.tsv").read_bytes().startswith(_native.nj_changes_header()) and (tmp_path / "both.h.kpsc_o.tsv").read_bytes().startswith(_native.nj_homoplasy_header())
    assert (tmp_path / "both.kpsc_k.tsv").read_bytes() == plain
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "x.tsv"), "--nj", str(tmp_path / "x.t.tsv"), "--nj-changes", "-"]) == 1  # stdout is refused
    # the flag without the tree: the parser's error
    with pytest.raises(SystemExit):
        main(["assembly", db_path, *paths, "-o", str(tmp_path / "o5.tsv"), "--nj-changes", str(tmp_path / "changes5.tsv")])
    assert "--nj-changes requires --nj FILE" in capsys.readouterr().err and not (tmp_path / "changes5.tsv").exists()
