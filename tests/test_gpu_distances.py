"""Pairwise locus distances on the device (include/kp_spec.h, DISTANCES; kaptive_amd/csrc/kp_dist.hip) against the numpy restatement of
tests/distances_util.py: integers and order, exactly.  Matrices of every shape at which the pair kernel takes another path -- R around
the tile (a diagonal tile, off-diagonal tiles, ragged last tiles on both axes, several tile rows), NB around the plane word and the
chunk -- with planted rows; every filter; two runs byte for byte; the refusals of the C entry points; the allocation count around a
handle; then the whole route on the 9-locus miniature database: ``Serotyper(db, distances=True)`` over two batches against
``LocusRows`` fed from the restated aligned rows, the command line with ``--distances`` and with ``--db``, the main report unchanged,
a run without the flag, and two devices."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.distances import LocusRows
from tests import distances_util as D
from tests.distances_util import CH, ROWS, SPLIT, T, Run, _device_count, _write_inputs

pytestmark = pytest.mark.gpu

BLOCKS = (1, 3, 4, 5, 4 * CH - 1, 4 * CH, 4 * CH + 1, 8 * CH + 3)
EINVAL, ESTATE = -1, -4


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _matrix(codes) -> np.ndarray:
    return D.pack(codes).reshape(codes.shape[0], -1) if codes.shape[0] else np.zeros((0, codes.shape[1] // 16), np.uint64)


def _filtered(every, max_diff, min_compared):
    md = np.iinfo(np.int32).max if max_diff is None else max_diff
    return every[(every["differences"] <= md) & (every["compared"] >= min_compared)]


# ---- 1. every shape, every filter ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
def test_pairs_against_the_restatement(ctx, R):
    assert T == D.TILE and CH == D.CHUNK
    for nb in BLOCKS:
        rng = np.random.default_rng([R, nb])
        codes = D.population(rng, R, nb)
        every = D.all_pairs(codes)  # the reference, once: the filters below select from it, in order
        assert len(every) == R * (R - 1) // 2
        with _native.Distances(ctx, _matrix(codes)) as d:
            assert (d.n_rows, d.n_blocks) == (R, nb)
            first = {}
            for max_diff, min_compared in ((None, 0), (SPLIT, 0), (0, 0), (None, 16 * nb + 1), (SPLIT, 16 * nb // 2)):
                got = d.pairs(max_diff, min_compared)
                want = _filtered(every, max_diff, min_compared)
                assert got.dtype == _native.DIST_PAIR_DTYPE and d.count(max_diff, min_compared) == len(want)
                if got.tobytes() != want.tobytes():
                    z = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
                    raise AssertionError(f"R {R}, NB {nb}, max_diff {max_diff}, min_compared {min_compared}: {len(got)} pairs on the device, {len(want)} wanted; "
                                         f"first difference at {z}: {got[z] if z < len(got) else None} vs {want[z] if z < len(want) else None}")
                first[(max_diff, min_compared)] = got.tobytes()
            assert len(d.pairs(None, 16 * nb + 1)) == 0  # above every pair
            if R >= T - 1:
                n_split = len(_filtered(every, SPLIT, 0))
                assert 0 < n_split < len(every), "the population must be split by max_diff"
                p = {(int(r["a"]), int(r["b"])): r for r in d.pairs(None, 0)}
                assert p[(0, 1)]["differences"] == 0 and p[(0, 1)]["unshared"] == 0  # identical rows
                assert all(p[(2, b)]["compared"] == 0 and p[(2, b)]["unshared"] == int((codes[b] != D.GAP).sum()) for b in range(3, R))  # the all-GAP row
                assert all(p[(3, b)]["compared"] == 0 and p[(3, b)]["unshared"] == int((codes[b] == D.GAP).sum()) for b in range(4, R))  # the all-N row
                assert all(p[(r, 10)]["differences"] == 1 and p[(r, 10)]["compared"] == 16 * nb for r in range(4, 10))  # one column away, at every edge
                assert p[(11, 12)]["differences"] == p[(11, 12)]["compared"] == 16 * nb  # complements
        with _native.Distances(ctx, _matrix(codes)) as again:  # a second handle, the filters in another order: the same bytes
            for key in reversed(list(first)):
                assert again.pairs(*key).tobytes() == first[key]


# ---- 2. the entry points' refusals --------------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_refusals_and_call_order(ctx):
    lib = _native.lib()
    blocks = _matrix(D.population(np.random.default_rng(1), 5, 3))
    h, n = C.c_void_p(), C.c_int64(-1)

    def create(rows, nb, ptr=_p(blocks), out=C.byref(h), c=ctx._h):
        return lib.kp_dist_create(c, ptr, C.c_int32(rows), C.c_int64(nb), out)

    for args, kw, why in (((5, 3), dict(c=None), None), ((5, 3), dict(out=None), b"null"), ((5, 3), dict(ptr=None), b"null"), ((-1, 3), {}, b"negative"),
                          ((5, 0), {}, b"at least one block"), ((5, -2), {}, b"at least one block"), ((1, 2**27), {}, b"2^31"),
                          ((_native.DIST_MAX_ROWS + 1, 1), {}, b"KP_DIST_MAX_ROWS")):  # fmt: skip
        rc = create(*args, **kw)
        assert rc == EINVAL, rc
        if why is not None:
            assert why in lib.kp_last_error(ctx._h), lib.kp_last_error(ctx._h)
        assert not h.value
    with pytest.raises(ValueError):
        _native.Distances(ctx, np.zeros(4, np.uint64))
    for rows, nb in ((0, 0), (0, 3), (1, 3)):  # valid, and no pair
        with _native.Distances(ctx, np.zeros((rows, nb), np.uint64)) as d:
            assert d.count() == 0 and len(d.pairs()) == 0 and len(d.pairs(0, 0)) == 0
    assert create(5, 3) == 0 and h.value
    out = np.zeros(16, _native.DIST_PAIR_DTYPE)
    assert lib.kp_dist_pairs(ctx._h, h, _p(out), C.c_int64(16)) == ESTATE and b"kp_dist_count" in lib.kp_last_error(ctx._h)  # before a count
    assert lib.kp_dist_count(ctx._h, None, C.c_int32(1), C.c_int32(0), C.byref(n)) == EINVAL and lib.kp_dist_count(ctx._h, h, C.c_int32(1), C.c_int32(0), None) == EINVAL
    assert lib.kp_dist_count(None, h, C.c_int32(1), C.c_int32(0), C.byref(n)) == EINVAL
    assert lib.kp_dist_count(ctx._h, h, C.c_int32(2**31 - 1), C.c_int32(0), C.byref(n)) == 0 and n.value == 10
    assert lib.kp_dist_pairs(ctx._h, h, _p(out), C.c_int64(9)) == EINVAL and b"fewer pairs" in lib.kp_last_error(ctx._h)  # a short cap
    assert lib.kp_dist_pairs(ctx._h, h, None, C.c_int64(16)) == EINVAL and lib.kp_dist_pairs(ctx._h, None, _p(out), C.c_int64(16)) == EINVAL
    assert not out.view(np.uint8).any()  # a refused call stores nothing
    assert lib.kp_dist_pairs(ctx._h, h, _p(out), C.c_int64(16)) == 0
    assert out[:10].tobytes() == D.all_pairs(D.unpack(blocks)).tobytes() and not out[10:].view(np.uint8).any()
    lib.kp_dist_destroy.restype = None
    lib.kp_dist_destroy(h)
    lib.kp_dist_destroy(None)


def test_allocation_count_around_a_handle(ctx):
    codes = D.population(np.random.default_rng(2), 2 * T + 1, 5)
    before = _native.device_allocations()
    d = _native.Distances(ctx, _matrix(codes))
    sizes = [len(d.pairs(0, 0)), len(d.pairs(SPLIT, 0)), len(d.pairs(None, 0)), len(d.pairs(SPLIT, 0))]  # (the record list grows, then shrinks)
    assert sizes[0] < sizes[1] < sizes[2] and sizes[3] == sizes[1]
    d.close()
    d.close()
    assert _native.device_allocations() == before


# ---- 3. the whole route on the miniature database ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run():
    r = Run()
    yield r
    r.close()


def _want_records(rows: LocusRows, max_diff=D.MAX_DIFF, min_compared=D.MIN_COMPARED):
    out = []
    for L in rows.loci():
        idx, mat = rows.locus_matrix(L)
        out += [(L, int(idx[p["a"]]), int(idx[p["b"]]), int(p["compared"]), int(p["differences"]), int(p["unshared"])) for p in D.all_pairs(D.unpack(mat), max_diff, min_compared)]
    return out


def _want_tsv(rows: LocusRows, max_diff=D.MAX_DIFF, min_compared=D.MIN_COMPARED) -> bytes:
    return b"".join(D.format_lines(rows.db.loci.ids[L], rows.columns(L), [rows.ids[i] for i in rows.locus_matrix(L)[0]],
                                   D.all_pairs(D.unpack(rows.locus_matrix(L)[1]), max_diff, min_compared)) for L in rows.loci())  # fmt: skip


def test_serotyper_over_two_batches(run):
    got, want, db = run.typer.locus_rows, run.want_rows, run.db
    assert got.ids == want.ids == run.ids and got.best.tolist() == want.best.tolist() == [run.plan[n][0] for n in run.ids]
    assert got.loci() == want.loci() == [0, 3, 6]
    for L in got.loci():
        (i1, m1), (i2, m2) = got.locus_matrix(L), want.locus_matrix(L)
        assert i1.tolist() == i2.tolist() and m1.tobytes() == m2.tobytes(), f"locus {L}: the device's rows and the restated ones"
    bt, (rows, blocks) = run.bts[0]  # ... and gene by gene, in plain loops, for the first batch
    for a in range(len(bt.ids)):
        L = int(bt.best_locus[a])
        idx, mat = got.locus_matrix(L)
        assert D.unpack(mat[idx.tolist().index(a)]).tolist() == D.locus_row(db, L, bt.sums["n_kept"][a], bt.kept[a], rows[a], blocks).tolist()
    ctx = run.typer.engine.ctx
    for max_diff, min_compared in ((D.MAX_DIFF, D.MIN_COMPARED), (None, 0), (0, 1)):
        rec = got.distances(ctx, max_diff, min_compared)
        assert [tuple(int(x) for x in r) for r in rec] == _want_records(want, max_diff, min_compared)
    every = {(int(r["a"]), int(r["b"])): r for r in got.distances(ctx, None, 0)}
    assert len(every) == 10 + 6 + 3
    at = {n: i for i, n in enumerate(run.ids)}
    pair = lambda x, y: every[tuple(sorted((at[x], at[y])))]  # noqa: E731
    cols = got.columns(0)
    r = pair("L0_exact_0", "L0_exact_1")  # two identical loci
    assert (r["compared"], r["differences"], r["unshared"]) == (cols, 0, 0)
    r = pair("L0_exact_0", "L0_snp_2")  # one planted SNP in a gene
    assert (r["compared"], r["differences"], r["unshared"]) == (cols, 1, 0)
    r, lost = pair("L0_exact_0", "L0_lacking_3"), int(db.genes.lengths[run.plan["L0_lacking_3"][2]])  # one gene lacking
    assert r["differences"] == 0 and r["unshared"] >= lost and r["compared"] <= cols - lost
    r = pair("L0_exact_0", "L0_far_4")
    assert r["differences"] > D.MAX_DIFF
    assert pair("L3_snp_1", "L3_snp_2")["differences"] == 2 and pair("L3_exact_0", "L3_exact_3")["differences"] == 0
    listed = got.distances(ctx)
    assert 0 < len(listed) < len(every) and not any(at["L0_far_4"] in (int(r["a"]), int(r["b"])) for r in listed)
    assert got.tsv(ctx) == _want_tsv(want) and got.tsv(ctx).count(b"\n") == len(listed)
    idx, diff, comp = got.matrix(ctx, 3)
    assert idx.tolist() == sorted(at[n] for n in run.ids if run.plan[n][0] == 3) and (diff == diff.T).all() and (comp == comp.T).all() and not diff.diagonal().any()
    assert diff[idx.tolist().index(at["L3_snp_1"]), idx.tolist().index(at["L3_snp_2"])] == 2


def test_command_line(run, tmp_path):
    from kaptive_amd.cli import main
    from kaptive_amd.synth import make_db

    db_path, paths = _write_inputs(run.db, run.genomes, tmp_path)
    table = _native.DISTANCES_HEADER + _want_tsv(run.want_rows)
    assert table.count(b"\n") > 5
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "plain.tsv")]) == 0
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--distances", str(tmp_path / "d.tsv"), "--batch-size", "7"]) == 0
    assert (tmp_path / "d.tsv").read_bytes() == table
    plain = (tmp_path / "plain.tsv").read_bytes()
    assert (tmp_path / "out.tsv").read_bytes() == plain and plain.endswith(run.tsv)  # the main report: the bytes of a run without the flag
    assert not list(tmp_path.glob("*aligned*"))  # the rows are made, no --aligned table is written
    # the thresholds, and --aligned beside it: each table is what it is alone
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o2.tsv"), "--aligned", str(tmp_path / "rows.tsv")]) == 0
    rows_alone = (tmp_path / "rows.tsv").read_bytes()
    assert main(["assembly", db_path, *paths, "-o", str(tmp_path / "o2.tsv"), "--aligned", str(tmp_path / "rows.tsv"), "--distances", str(tmp_path / "d2.tsv"),
                 "--max-distance", "0", "--min-compared", "1000", "--batch-size", "5"]) == 0  # fmt: skip
    assert (tmp_path / "rows.tsv").read_bytes() == rows_alone and (tmp_path / "o2.tsv").read_bytes() == plain
    assert (tmp_path / "d2.tsv").read_bytes() == _native.DISTANCES_HEADER + _want_tsv(run.want_rows, 0, 1000)
    # a second database: a table per database
    o_path = str(make_db("kpsc_o", seed=8).save(tmp_path / "o.npz"))
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "both.tsv"), "--distances", str(tmp_path / "both.d.tsv")]) == 0
    assert (tmp_path / "both.d.kpsc_k.tsv").read_bytes() == table
    assert (tmp_path / "both.d.kpsc_o.tsv").read_bytes().startswith(_native.DISTANCES_HEADER)
    assert (tmp_path / "both.kpsc_k.tsv").read_bytes() == plain
    assert main(["assembly", db_path, *paths, "--db", o_path, "-o", str(tmp_path / "x.tsv"), "--distances", "-"]) == 1  # stdout is refused
    assert not (tmp_path / "x.tsv").exists()


def test_without_the_flag_nothing_is_allocated_or_kept(run):
    from kaptive_amd.serotyping.core import Serotyper

    typer = Serotyper(run.db)
    try:
        part = run.genomes[:7]
        typer.type_many(part)
        before = _native.device_allocations()
        results = typer.type_many(part)  # a settled context, a repeated batch: nothing grows
        assert _native.device_allocations() == before
        assert typer.locus_rows is None and not typer.engine.aligned and not typer.engine.cigar
        from kaptive_amd.serotyping.io import KaptiveRow

        assert b"".join(bytes(KaptiveRow.from_result(r)) for r in results) == run.bts[0][0].tsv()  # the typing does not depend on the option
    finally:
        typer.engine.close()


@pytest.mark.skipif("_device_count() < 2")
def test_command_line_on_two_devices(run, tmp_path):
    import subprocess
    import sys

    db_path, paths = _write_inputs(run.db, run.genomes, tmp_path)
    from tests.conftest import ROOT

    r = subprocess.run([sys.executable, "-m", "kaptive_amd", "assembly", db_path, *paths, "-o", str(tmp_path / "out.tsv"), "--distances",
                        str(tmp_path / "d.tsv"), "--devices", "0,1", "--batch-size", "3"], capture_output=True, timeout=600, cwd=str(ROOT))  # fmt: skip
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    assert (tmp_path / "d.tsv").read_bytes() == _native.DISTANCES_HEADER + _want_tsv(run.want_rows)
