"""The occurrence cut on every path and on both sides of its thresholds, with the inputs of tests/occ_cut_util.py
(tests/test_occ_cut_oracle.py pins what those inputs are): kp_occ_cut_kernel's rounds, wave slices, certificate, counting
windows and compaction, kp_occ_sketch_kernel's chunks and kp_occ_quantile_kernel's histogram and index.  For every assembly
the anchors after the cut, the band tasks and the hits equal the oracle's, the state word and the mid_occ the pass left
(Batch.occ) equal the oracle's, and where the assembly claimed a counting table its (value, count) entries are the histogram
of the oracle's minimizers, exactly.  Integers throughout: no tolerance, no case left out of a comparison."""

import numpy as np
import pytest

from kaptive_amd import _native
from tests import occ_cut_util as U
from tests.test_gpu_parity import _same_records

pytestmark = pytest.mark.gpu
TASK_ORDER = list(_native.TASK_DTYPE.names)


@pytest.fixture(scope="module")
def built(oracle):
    return U.built(oracle)


@pytest.fixture(scope="module")
def ctx(built):
    c = _native.Context(0)
    c.load_genes(built["codes"], built["off"])
    yield c
    c.close()


_WANT: dict = {}


def _want(oracle, odb, asm):
    """The oracle's side of one assembly, computed once: a batch may hold an assembly twice, and two passes compare with it."""
    key = (id(odb), asm.id)
    if key not in _WANT:
        pa = asm.packed()
        n_over_max, mid_occ, asks = odb.occ(pa)
        hist = U.minimizer_histogram(oracle, pa) if asks else None
        _WANT[key] = dict(pa=pa, anchors=odb.anchors(pa), tasks=np.sort(odb.tasks(pa), order=TASK_ORDER), hits=odb.align(pa),
                             state=int(n_over_max > 0) | 2 * int(asks), mid_occ=mid_occ, hist=hist)  # fmt: skip
    return _WANT[key]


def _run_and_compare(oracle, built, ctx, asms, what):
    want = [_want(oracle, built["odb"], a) for a in asms]
    batch = ctx.batch([w["pa"] for w in want])
    hits, off = batch.align()
    for i, (asm, w) in enumerate(zip(asms, want)):
        where = f"{what}, {asm.id} (entry {i})"
        got = batch.anchors(i)
        assert np.array_equal(got, w["anchors"]), f"{where}: {len(got)} anchors after the cut, the oracle has {len(w['anchors'])}"
        _same_records(np.sort(batch.tasks(i), order=TASK_ORDER), w["tasks"], f"{where}: tasks")
        _same_records(hits[off[i] : off[i + 1]], w["hits"], f"{where}: hits")
        state, mid_occ, table = batch.occ(i)
        assert (state, mid_occ) == (w["state"], w["mid_occ"]), f"{where}: state {state} and mid_occ {mid_occ}, the oracle has {w['state']} and {w['mid_occ']}"
        if w["hist"] is None:
            assert len(table) == 0, f"{where}: a counting table without a demand"
            continue
        x, cnt = w["hist"]
        order = np.argsort(table[:, 0], kind="stable")
        assert len(table) == len(x), f"{where}: the table holds {len(table)} values, the assembly has {len(x)} distinct minimizers"
        assert np.array_equal(table[order, 0], x), f"{where}: the table's values are not the assembly's minimizers"
        wrong = np.flatnonzero(table[order, 1] != cnt)
        assert len(wrong) == 0, f"{where}: {len(wrong)} counts differ, the first: value {x[wrong[0]]} counted {table[order, 1][wrong[0]]} times, occurs {cnt[wrong[0]]} times"
    return batch, hits, off


def _mixed(cases):
    """The cases' assemblies between repeat-free neighbours."""
    plain = U.plain_neighbours()
    asms = [plain[0]]
    for i, c in enumerate(cases):
        asms.append(c.asm)
        if i % 7 == 3:
            asms.append(plain[i % 2])
    return asms + [plain[1]]


def test_list_positions_rounds_slices_and_compaction(oracle, built, ctx):
    """Group A: gene R's stretch at every place of the sorted list that the round, slice and compaction logic tells apart --
    which kp_chain_kernel's identical round and slice logic meets as well (tasks and hits) --, the case whose drops straddle
    the compaction chunk first and last in the batch, and a second pass on the same context."""
    cases = built["groups"]["A"]
    straddle = next(c.asm for c in cases if c.label.startswith("chunk_511_512"))
    asms = [straddle, *_mixed(cases), straddle]
    first, hits, off = _run_and_compare(oracle, built, ctx, asms, "list positions")
    last = len(asms) - 1
    assert first.anchors(0).tobytes() == first.anchors(last).tobytes() and hits[off[0] : off[1]].tobytes() == hits[off[last] : off[last + 1]].tobytes()
    empty = next(i for i, a in enumerate(asms) if a.id == "all_dropped")
    assert len(first.anchors(empty)) == 0 and len(first.tasks(empty)) == 0 and off[empty] == off[empty + 1]
    again, hits2, off2 = _run_and_compare(oracle, built, ctx, asms, "list positions, second pass")
    assert np.array_equal(off, off2) and hits.tobytes() == hits2.tobytes()
    first.close()
    again.close()


def test_counts_on_both_sides_of_the_floor_the_certificate_and_the_window(oracle, built, ctx):
    """Group B: ten and eleven anchors of a seed on one and on both strands, ten and eleven pairs without a seed beyond ten,
    seeds on either side of a counting window's edge and on a gene's last position on either strand, tombstones of an earlier
    window under a later one."""
    batch, _, _ = _run_and_compare(oracle, built, ctx, _mixed(built["groups"]["B"]), "counting")
    batch.close()


def test_floor_or_quantile(oracle, built, ctx):
    """Group C: two seeds beyond the floor are cut at the floor; a third -- in the same or in another window of the gene, not in
    another gene -- hands the decision to the assembly's quantile, which keeps them, cuts exactly above itself, or lies
    below the floor."""
    batch, _, _ = _run_and_compare(oracle, built, ctx, _mixed(built["groups"]["C"]), "floor or quantile")
    batch.close()


def test_sketch_tables_at_chunk_contig_and_n_run_edges(oracle, built, ctx):
    """Group D: the counting table itself -- short contigs, several contigs in a chunk, contig ends just behind a chunk edge,
    a start inside a chunk's warm-up, N runs at chunk edges and in the warm-up, low-complexity runs across chunk edges."""
    batch, _, _ = _run_and_compare(oracle, built, ctx, _mixed(built["groups"]["D"]), "sketch tables")
    batch.close()


def test_sketch_second_chunk_per_thread(oracle, built, ctx):
    """Group D: more padded positions than a table's threads have first chunks; the repeats and the gene under test lie
    beyond them."""
    batch, _, _ = _run_and_compare(oracle, built, ctx, _mixed(built["groups"]["D2"]), "second chunk")
    batch.close()


def test_quantile_index_and_histogram_cap(oracle, built, ctx):
    """Group E: mid_occ on both sides of every step of kth (5000 / 5001 and 10 000 / 10 001 distinct minimizers), and a
    count at the quantile in the histogram's last bins and beyond its cap."""
    batch, _, _ = _run_and_compare(oracle, built, ctx, _mixed(built["groups"]["E"]), "quantile")
    batch.close()


def test_quantile_of_a_single_distinct_minimizer(oracle):
    """Group E, a database of its own (a gene with a homopolymer run): poly-A assemblies claim a table that holds one value --
    n = 1, kth = 0, the quantile read off a single bin."""
    from kaptive_amd.pack import pack_sequences_flat

    codes, off = pack_sequences_flat(U.single_value_gene_sequences())
    single = dict(odb=oracle.OracleDB(codes, off))
    c = _native.Context(0)
    c.load_genes(codes, off)
    cases = U.single_value_cases()
    batch, _, _ = _run_and_compare(oracle, single, c, [U.plain_neighbours()[1], *[x.asm for x in cases], U.plain_neighbours()[1]], "single value")
    for i, x in enumerate(cases, start=1):
        state, _, table = batch.occ(i)
        assert state == 3 and len(table) == 1, x.label
    batch.close()
    c.close()


def test_occ_of_a_displaced_batch_is_refused(oracle, built, ctx):
    """Batch.occ follows the other stage accessors: a batch whose work set went to later passes has no resident results, and
    an assembly index outside the batch is a bad argument."""
    pa = U.plain_neighbours()[0].packed()
    batches = [ctx.batch([pa]) for _ in range(_native.WORK_SLOTS + 1)]
    for b in batches:
        b.align()
    state, mid_occ, table = batches[-1].occ(0)
    assert (state, mid_occ, len(table)) == (0, U.MID, 0)
    with pytest.raises(_native.NativeError, match="no resident alignment results"):
        batches[0].occ(0)
    with pytest.raises(ValueError):
        batches[-1].occ(1)
    for b in batches:
        b.close()
