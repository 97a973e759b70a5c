"""The variable sites of locus rows on the device (include/kp_spec.h, SITES; kaptive_amd/csrc/kp_dist_sites.hip) against the restatement in
tests/sites_util.py: integers, order and bytes, exactly.  Random populations with planted columns at every number of rows at which
a lane, a wave, a workgroup or a slab fills up and at every row width at which a plane word is short; matrices without a site; the
property that ties the site matrix to DISTANCES; the state the calls must leave alone and their refusals; then the whole route on
the 9-locus miniature database: ``Serotyper(db, distances=True)`` over two batches, the command line with ``--sites``, with
``--snp-alignment``, with ``--core-sites``, beside the four pair tables and with ``--db``, a run without the flags, and two devices."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from tests import clusters_util as CU
from tests import distances_util as D
from tests import sites_util as SU
from tests import tree_util as TU
from tests.distances_util import CH, ROWS, SPLIT, T, Run, _count_handles, _device_count, _write_inputs

pytestmark = pytest.mark.gpu

THREADS, LANE_ROWS, SLAB = _native.SITES_THREADS, _native.SITES_LANE_ROWS, _native.SITES_SLAB
SITE_ROWS = tuple(sorted({0, 1, 2, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, THREADS * LANE_ROWS - 1, THREADS * LANE_ROWS + 1, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 3}))
BLOCKS = (1, 4, 5, 4 * CH + 1, 8 * CH + 3)
LARGE = THREADS * LANE_ROWS - 1  # from here on: the two smallest and one large NB only
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


def planted(rng, R: int, nb: int) -> np.ndarray:
    """``D.population`` with the columns of the issue planted on top.  A column with a single dissenting row at each of the matrix
    columns 0, 15, 16, 63, 64, the last one and the one before a gene's padding (columns 40 .. 47 are GAP in every row where the rows
    are wide enough: a gene of 40 bases) -- the dissenter being row 0, row R - 1, the last row of the first slab and the first row
    of the second in turn; then, where they are free, a column in which every row holds the same base, one with base + base + N and
    the rest GAP, and a pair of columns that differ in one GAP: a core site and one that is none."""
    codes = D.population(rng, R, nb)
    cols = 16 * nb
    if R == 0:
        return codes
    if nb >= 4:
        codes[:, 40:48] = D.GAP
    at = [c for c in dict.fromkeys((0, 15, 16, 63, 64, cols - 1, 39 if nb >= 4 else 0)) if c < cols]
    dissenters = [0, R - 1, min(SLAB - 1, R - 1), min(SLAB, R - 1)]
    for i, c in enumerate(at):
        base = int(rng.integers(0, 4))
        codes[:, c] = base
        codes[dissenters[(i + R) % 4], c] = (base + 1) % 4
    free = [c for c in (1, 2, 3, 4) if c not in at]
    codes[:, free[0]] = 2  # every row the same base: the count is R, and every plane of a full lane's counter carries
    if R >= 3:
        codes[:, free[1]] = D.GAP
        codes[[0, R // 2, R - 1], free[1]] = (1, D.N, 3)  # a site through the two bases beside the N
        codes[:, free[2]] = codes[:, free[3]] = 0
        codes[R // 2, free[2]] = codes[R // 2, free[3]] = 3  # a core site ...
        codes[R - 1, free[3]] = D.GAP  # ... and its twin with one GAP
    return codes


def _want(codes):
    R = codes.shape[0]
    out = {"profile": SU.profile(codes) if R else np.zeros(0, SU.SITE_DTYPE)}
    for core in (False, True):
        s = SU.sites(codes, core) if R > 1 else np.zeros(0, SU.SITE_DTYPE)
        out[core] = (s, SU.site_blocks(codes, s["column"]))
    return out


def _check(d, want, what, order=("profile", False, True)):
    got = {}
    for key in order:
        if key == "profile":
            got[key] = d.profile().tobytes()
            assert d.profile().dtype == _native.SITE_DTYPE and len(d.profile()) == len(want[key]), what  # 16 NB records, not 64 NW
            assert got[key] == want[key].tobytes(), f"{what}: profile; first column {int(np.flatnonzero(d.profile() != want[key])[0])}"
        else:
            s = d.sites(core=key)
            rows = d.site_rows()
            ws, wr = want[key]
            assert s["column"].tolist() == ws["column"].tolist() and s.tobytes() == ws.tobytes(), f"{what}: sites, core {key}"
            assert rows.shape == wr.shape and rows.tobytes() == wr.tobytes(), f"{what}: site rows, core {key}"
            got[key] = s.tobytes() + rows.tobytes()
    return got


# ---- 1. random populations with planted columns: every number of rows, every width ---------------------------------------------------------
@pytest.mark.parametrize("R", SITE_ROWS)
def test_profile_sites_and_site_rows_against_the_restatement(ctx, R):
    for nb in BLOCKS if R < LARGE else (BLOCKS[0], BLOCKS[1], BLOCKS[-1]):
        codes = planted(np.random.default_rng([R, nb]), R, nb)
        want = _want(codes)
        what = f"R {R}, NB {nb}"
        with _native.Distances(ctx, _matrix(codes)) as d:
            first = _check(d, want, what)
        if R >= 3:
            s, core = want[False][0], want[True][0]
            assert {0, 15}.issubset(s["column"].tolist()) and (s["n"].sum(axis=1) + s["n_n"] <= R).all()
            assert 0 < len(core) < len(s) and (want["profile"]["n"].max() == R)
        with _native.Distances(ctx, _matrix(codes)) as again:  # a second handle, the calls in another order: the same bytes
            assert _check(again, want, what, order=(True, False, "profile")) == first


# ---- 2. matrices without a site -----------------------------------------------------------------------------------------------------------
def test_identical_all_gap_and_all_n_rows_have_no_site(ctx):
    R, nb = 3 * T + 5, 4 * CH + 1
    same = np.tile(np.random.default_rng(21).integers(0, 4, 16 * nb).astype(np.uint8), (R, 1))
    for codes in (same, np.full((R, 16 * nb), D.GAP, np.uint8), np.full((R, 16 * nb), D.N, np.uint8)):
        with _native.Distances(ctx, _matrix(codes)) as d:
            for core in (False, True):
                assert len(d.sites(core)) == 0 and d.sites_count(core) == 0 and d.site_rows().shape == (R, 0)
            assert d.profile().tobytes() == SU.profile(codes).tobytes()
    with _native.Distances(ctx, _matrix(same)) as d:
        p = d.profile()
        assert (p["n"].sum(axis=1) == R).all() and (p["n"].max(axis=1) == R).all() and not p["n_n"].any()


# ---- 3. the property ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
def test_the_site_matrix_keeps_every_pairs_differences(ctx, R):
    nb = 4 * CH + 1
    codes = D.population(np.random.default_rng([3, R, nb]), R, nb)
    with _native.Distances(ctx, _matrix(codes)) as d:
        full = d.pairs(None, 0)
        s = d.sites()
        rows = d.site_rows()
    assert rows.shape == (R, (len(s) + 15) // 16)
    if R < 2:
        assert len(s) == 0 and len(full) == 0
        return
    assert 0 < len(s) <= 16 * nb
    with _native.Distances(ctx, rows) as cut:  # a site matrix is itself a matrix of locus rows
        few = cut.pairs(None, 0)
    assert few["a"].tolist() == full["a"].tolist() and few["b"].tolist() == full["b"].tolist() and len(few) == R * (R - 1) // 2
    assert few["differences"].tobytes() == full["differences"].tobytes() and (few["compared"] <= full["compared"]).all()


# ---- 4. state and refusals -----------------------------------------------------------------------------------------------------------------
def test_the_state_the_calls_leave_alone_and_their_refusals(ctx):
    lib = _native.lib()
    codes = planted(np.random.default_rng(4), 2 * T + 1, 5)
    want = _want(codes)
    before = _native.device_allocations()
    with _native.Distances(ctx, _matrix(codes)) as d:
        n_sites, none = C.c_int64(-7), np.zeros(0, _native.SITE_DTYPE)
        # without a count
        assert lib.kp_dist_sites(ctx._h, d._h, None, C.c_int64(0)) == ESTATE and b"kp_dist_sites_count" in lib.kp_last_error(ctx._h)
        assert lib.kp_dist_site_rows(ctx._h, d._h, None, C.c_int64(0)) == ESTATE and b"kp_dist_sites_count" in lib.kp_last_error(ctx._h)
        with pytest.raises(Exception):
            d.site_rows()
        # unknown flags, null pointers
        for flags in (2, 4, 3, -1, 1 << 30):
            assert lib.kp_dist_sites_count(ctx._h, d._h, C.c_int32(flags), C.byref(n_sites)) == EINVAL and b"flags" in lib.kp_last_error(ctx._h)
        assert lib.kp_dist_sites_count(ctx._h, d._h, C.c_int32(0), None) == EINVAL and lib.kp_dist_sites_count(None, d._h, C.c_int32(0), C.byref(n_sites)) == EINVAL
        assert lib.kp_dist_sites_count(ctx._h, None, C.c_int32(0), C.byref(n_sites)) == EINVAL and n_sites.value == -7
        assert lib.kp_dist_sites(ctx._h, d._h, None, C.c_int64(0)) == ESTATE  # a refused count is no count
        # sites between count and pairs, and around clusters and tree
        pairs = d.pairs(SPLIT, 1)
        n = d.count(SPLIT, 1)
        s = d.sites()
        out = np.zeros(n, _native.DIST_PAIR_DTYPE)
        assert lib.kp_dist_pairs(ctx._h, d._h, _p(out), C.c_int64(n)) == 0 and out.tobytes() == pairs.tobytes() and n == len(pairs) > 0  # count -> sites -> pairs
        clusters, tree = d.clusters(CU.LEVELS, 1), d.tree(0)
        assert d.site_rows().tobytes() == want[False][1].tobytes()  # count -> pairs, clusters, tree -> site rows
        again = d.sites()
        after, tree_after = d.clusters(CU.LEVELS, 1), d.tree(0)
        assert s.tobytes() == again.tobytes() == want[False][0].tobytes()
        assert clusters[0].tobytes() == after[0].tobytes() and clusters[1].tobytes() == after[1].tobytes()
        assert tree[0].tobytes() == tree_after[0].tobytes() and tree[1].tobytes() == tree_after[1].tobytes() == TU.forest(codes, 0)[1].tobytes()
        # short caps
        S, cols = len(s), codes.shape[1]
        room, blocks = np.zeros(S, _native.SITE_DTYPE), np.zeros((len(codes), (S + 15) // 16), np.uint64)
        assert S > 16 and lib.kp_dist_sites(ctx._h, d._h, _p(room), C.c_int64(S - 1)) == EINVAL and lib.kp_dist_sites(ctx._h, d._h, None, C.c_int64(S)) == EINVAL
        assert lib.kp_dist_site_rows(ctx._h, d._h, _p(blocks), C.c_int64(blocks.size - 1)) == EINVAL and lib.kp_dist_site_rows(ctx._h, d._h, None, C.c_int64(blocks.size)) == EINVAL
        prof = np.zeros(cols, _native.SITE_DTYPE)
        assert lib.kp_dist_profile(ctx._h, d._h, _p(prof), C.c_int64(cols - 1)) == EINVAL and lib.kp_dist_profile(ctx._h, d._h, None, C.c_int64(cols)) == EINVAL
        assert not room.view(np.uint8).any() and not blocks.any() and not prof.view(np.uint8).any()  # a refused call stores nothing
        assert lib.kp_dist_sites(ctx._h, d._h, _p(room), C.c_int64(S)) == 0 and room.tobytes() == s.tobytes()  # ... and leaves the count standing
        assert lib.kp_dist_profile(ctx._h, d._h, _p(prof), C.c_int64(cols)) == 0 and prof.tobytes() == want["profile"].tobytes()
        # the core count replaces the other one
        assert d.sites_count(True) == len(want[True][0]) and d.site_rows().tobytes() == want[True][1].tobytes()
        assert len(none) == 0
    assert _native.device_allocations() == before
    for rows, nb in ((0, 0), (0, 3), (1, 3)):  # valid: no site
        with _native.Distances(ctx, np.full((rows, nb), D.pack(np.arange(16) % 4)[0], np.uint64)) as d:
            assert len(d.sites()) == 0 and len(d.sites(True)) == 0 and d.site_rows().shape == (rows, 0) and len(d.profile()) == 16 * nb * rows
            if rows:
                assert d.profile()["n"].sum() == 16 * nb
    if _device_count() > 1:  # a handle of another device
        other = _native.Context(1)
        try:
            with _native.Distances(other, _matrix(codes)) as foreign:
                assert lib.kp_dist_sites_count(ctx._h, foreign._h, C.c_int32(0), C.byref(n_sites)) == EINVAL and b"another device" in lib.kp_last_error(ctx._h)
        finally:
            other.close()


# ---- 5. the whole route on the miniature database ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run():
    r = Run()
    yield r
    r.close()


def _tuples(rec):
    return [(int(r["locus"]), int(r["gene"]), int(r["position"]), int(r["column"]), tuple(int(x) for x in r["n"]), int(r["n_n"])) for r in rec]


def test_serotyper_over_two_batches(run):
    got, want = run.typer.locus_rows, run.want_rows
    assert got.ids == want.ids == run.ids and got.loci() == want.loci() == [0, 3, 6]
    ctx = run.typer.engine.ctx
    for core in (False, True):
        assert _tuples(got.sites(ctx, core)) == SU.run_sites(want, core)
        assert got.sites_tsv(ctx, core) == SU.run_sites_tsv(want, core) and got.snp_alignment_tsv(ctx, core) == SU.run_alignment_tsv(want, core)
    rec = got.sites(ctx)
    three = rec[rec["locus"] == 3]  # exact, snp, snp, exact: the two planted bases and nothing else
    genes = sorted(g for name, (L, kind, g) in run.plan.items() if L == 3 and kind == "snp")
    assert len(three) == 2 and sorted(three["gene"].tolist()) == genes and all(sorted(r["n"].tolist())[2:] == [1, 3] and r["n_n"] == 0 for r in three)
    lines = [ln.split(b"\t") for ln in got.snp_alignment_tsv(ctx).splitlines() if ln.startswith(run.db.loci.ids[3].encode() + b"\t")]
    assert len(lines) == 4 and all(ln[2] == b"2" and len(ln[3]) == 2 for ln in lines) and len({ln[3] for ln in lines}) == 3
    for L in (0, 3, 6):
        idx, s, blocks = got.site_rows(ctx, L)
        codes = D.unpack(want.locus_matrix(L)[1])
        assert blocks.tobytes() == SU.site_blocks(codes, SU.sites(codes)["column"]).tobytes() and got.profile(ctx, L).tobytes() == SU.profile(codes).tobytes()
    from tests.test_gpu_distances import _want_tsv

    assert got.tsv(ctx) == _want_tsv(want) and got.clusters_tsv(ctx) == CU.run_tsv(want) and got.tree_tsv(ctx) == TU.run_tree_tsv(want)  # the other tables of the same handles
    got.close()


def _count_site_calls(monkeypatch):
    calls = []
    for name in ("profile", "sites_count", "site_rows"):
        real = getattr(_native.Distances, name)

        def counting(self, *a, _real=real, _name=name, **kw):
            calls.append(_name)
            return _real(self, *a, **kw)

        monkeypatch.setattr(_native.Distances, name, counting)
    return calls


def test_command_line(run, tmp_path, monkeypatch):
    from kaptive_amd.cli import main
    from kaptive_amd.synth import make_db
    from tests.test_gpu_distances import _want_tsv

    db_path, paths = _write_inputs(run.db, run.genomes, tmp_path)
    made = _count_handles(monkeypatch)
    calls = _count_site_calls(monkeypatch)
    sites = {core: _native.SITES_HEADER + SU.run_sites_tsv(run.want_rows, core) for core in (False, True)}
    aln = {core: _native.SNP_ALIGNMENT_HEADER + SU.run_alignment_tsv(run.want_rows, core) for core in (False, True)}
    assert sites[False].count(b"\n") > 1 + 4 and aln[False].count(b"\n") == 1 + len(run.ids) and sites[True] != sites[False]
    # 7. a run with --distances alone: no sites call, and the files every other run must reproduce
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "plain.tsv"), "--distances", str(tmp_path / "d0.tsv")]) == 0
    plain, d0 = (tmp_path / "plain.tsv").read_bytes(), (tmp_path / "d0.tsv").read_bytes()
    assert calls == [] and len(made) == 3 and plain.endswith(run.tsv) and d0 == _native.DISTANCES_HEADER + _want_tsv(run.want_rows)
    assert sorted(p.name for p in tmp_path.glob("*.tsv")) == ["d0.tsv", "plain.tsv"]
    # either flag alone, then with --core-sites
    del made[:]
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o1.tsv"), "--sites", str(tmp_path / "s1.tsv"), "--batch-size", "7"]) == 0
    assert (tmp_path / "s1.tsv").read_bytes() == sites[False] and (tmp_path / "o1.tsv").read_bytes() == plain
    assert len(made) == 3 and "site_rows" not in calls and not list(tmp_path.glob("*aligned*"))  # a handle per locus; no other table
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o2.tsv"), "--snp-alignment", str(tmp_path / "a2.tsv")]) == 0
    assert (tmp_path / "a2.tsv").read_bytes() == aln[False] and (tmp_path / "o2.tsv").read_bytes() == plain
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o3.tsv"), "--sites", str(tmp_path / "s3.tsv"), "--snp-alignment", str(tmp_path / "a3.tsv"),
                 "--core-sites", "--batch-size", "5"]) == 0  # fmt: skip
    assert [(tmp_path / f).read_bytes() for f in ("o3.tsv", "s3.tsv", "a3.tsv")] == [plain, sites[True], aln[True]]
    # beside the four pair tables: each is what it is alone, and each matrix is uploaded once
    del made[:]
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o4.tsv"), "--sites", str(tmp_path / "s4.tsv"), "--snp-alignment", str(tmp_path / "a4.tsv"),
                 "--distances", str(tmp_path / "d4.tsv"), "--clusters", str(tmp_path / "c4.tsv"), "--mst", str(tmp_path / "m4.tsv"), "--newick", str(tmp_path / "n4.tsv")]) == 0  # fmt: skip
    assert [(tmp_path / f).read_bytes() for f in ("o4.tsv", "s4.tsv", "a4.tsv", "d4.tsv")] == [plain, sites[False], aln[False], d0]
    assert (tmp_path / "c4.tsv").read_bytes() == _native.clusters_header(CU.LEVELS) + CU.run_tsv(run.want_rows)
    assert (tmp_path / "m4.tsv").read_bytes() == _native.DISTANCES_HEADER + TU.run_tree_tsv(run.want_rows)
    assert (tmp_path / "n4.tsv").read_bytes() == _native.newick_header() + TU.run_newick_tsv(run.want_rows)
    assert len(made) == 3
    # a second database: a table per database
    o_path = str(make_db("kpsc_o", seed=8).save(tmp_path / "o.npz"))
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "both.tsv"), "--sites", str(tmp_path / "both.s.tsv"), "--snp-alignment",
                 str(tmp_path / "both.a.tsv")]) == 0  # fmt: skip
    assert (tmp_path / "both.s.kpsc_k.tsv").read_bytes() == sites[False] and (tmp_path / "both.a.kpsc_k.tsv").read_bytes() == aln[False]
    assert (tmp_path / "both.s.kpsc_o.tsv").read_bytes().startswith(_native.SITES_HEADER)
    assert (tmp_path / "both.a.kpsc_o.tsv").read_bytes().startswith(_native.SNP_ALIGNMENT_HEADER)
    assert (tmp_path / "both.kpsc_k.tsv").read_bytes() == plain
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "x.tsv"), "--snp-alignment", "-"]) == 1  # stdout is refused
    assert not (tmp_path / "x.tsv").exists()


@pytest.mark.skipif("_device_count() < 2")
def test_command_line_on_two_devices(run, tmp_path):
    import subprocess
    import sys

    db_path, paths = _write_inputs(run.db, run.genomes, tmp_path)
    from tests.conftest import ROOT

    r = subprocess.run([sys.executable, "-m", "kaptive_amd", "assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--sites", str(tmp_path / "s.tsv"),
                        "--snp-alignment", str(tmp_path / "a.tsv"), "--devices", "0,1", "--batch-size", "3"], capture_output=True, timeout=600, cwd=str(ROOT))  # fmt: skip
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    assert (tmp_path / "s.tsv").read_bytes() == _native.SITES_HEADER + SU.run_sites_tsv(run.want_rows)
    assert (tmp_path / "a.tsv").read_bytes() == _native.SNP_ALIGNMENT_HEADER + SU.run_alignment_tsv(run.want_rows)
