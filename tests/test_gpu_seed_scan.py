"""The seed scan on every lane, unit, list and flank edge, with the inputs of tests/seed_scan_util.py (tests/test_seed_scan_oracle.py
pins what those inputs are): kp_scan_dense_kernel's units, iterations, neighbour values, word offsets, list and stage,
kp_edge_kernel's flanks and thread split, kp_expand_kernel's rejections, strand lists and load-balanced copy.  Every batch runs
twice on one context and once with its assemblies in reverse order; each time the candidate list the scan left
(Batch.candidates) equals the numpy model's front and back sets exactly -- as counts, as sorted arrays, and without a duplicate
--, and every assembly's anchors and hits equal the oracle's.  Integers throughout: no tolerance, no case left out."""

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from tests import seed_scan_util as U
from tests.test_gpu_parity import _same_records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built(oracle):
    return U.built(oracle)


@pytest.fixture(scope="module")
def ctx(built):
    c = _native.Context(0)
    c.load_genes(built["world"].codes, built["world"].off)
    yield c
    c.close()


_WANT: dict = {}


def _want(odb, asm):
    """The oracle's side of one assembly, computed once per content: a batch may hold an assembly many times, and three passes compare with it."""
    pa = asm.packed()
    key = (np.asarray(pa.words).tobytes(), np.asarray(pa.ctg_start).tobytes(), np.asarray(pa.ctg_len).tobytes(), np.asarray(pa.n_runs).tobytes())
    if key not in _WANT:
        _WANT[key] = dict(anchors=odb.anchors(pa), hits=odb.align(pa))
    return _WANT[key]


def _run_and_compare(world, ctx, asms, what):
    model = world.model(asms)
    batch = ctx.batch([a.packed() for a in asms])
    hits, off = batch.align()
    front, back = batch.candidates()
    assert (len(front), len(back)) == (len(model.front), len(model.back)), f"{what}: {len(front)} front and {len(back)} back candidates, the model has {len(model.front)} and {len(model.back)}"
    front, back = np.sort(front), np.sort(back)
    assert len(np.unique(front)) == len(front), f"{what}: the front list holds a candidate twice"
    for got, want, part in ((front, model.front, "front"), (back, model.back, "back")):
        wrong = np.flatnonzero(got != want)
        assert len(wrong) == 0, f"{what}: {len(wrong)} {part} candidates differ; the first: device {U.unpack_cand(got[wrong[:1]])}, model {U.unpack_cand(want[wrong[:1]])}"
    for i, asm in enumerate(asms):
        w = _want(world.odb, asm)
        got = batch.anchors(i)
        assert np.array_equal(got, w["anchors"]), f"{what}, {asm.id} (entry {i}): {len(got)} anchors, the oracle has {len(w['anchors'])}"
        _same_records(hits[off[i] : off[i + 1]], w["hits"], f"{what}, {asm.id} (entry {i}): hits")
    batch.close()
    return hits, off


def _three_passes(built, ctx, name):
    world, asms = built["world"], built["cases"][name].asms
    hits, off = _run_and_compare(world, ctx, asms, name)
    hits2, off2 = _run_and_compare(world, ctx, asms, f"{name}, second pass")
    assert np.array_equal(off, off2) and hits.tobytes() == hits2.tobytes()
    _run_and_compare(world, ctx, asms[::-1], f"{name}, reversed")


def test_phase_sweep_every_unit_on_every_lane(built, ctx):
    """a: 62 copies of one probe assembly of 64 P bases, gcd(P, 62) = 1: every unit of the probe -- gene pieces, contigs of 1, 14, 15
    and 16 bases, N runs of 1 and 40 bases, a periodic stretch, abutting contigs, a contig that ends the assembly -- is owned once
    by every lane, once on either side of every iteration boundary, in the batch's first unit and in its last."""
    _three_passes(built, ctx, "a_phase_sweep")


@pytest.mark.parametrize("name", ["b_unit_offsets", "b_near_palindromes"])
def test_word_and_unit_offsets(built, ctx, name):
    """b: one gene 15-mer at each of the 64 offsets of a unit (every word offset of every word, the o == 0 path, positions 50..63
    that read the next lane's word); 15-mers that differ from their reverse complement in the middle base only, between every
    pair of flanking bases."""
    _three_passes(built, ctx, name)


def test_neighbour_reach(built, ctx):
    """c: strict window minima at positions 0, 8, 9 and 63, 55, 54 of the units on either side of a unit boundary and of the
    boundary between lane 62 of one iteration and lane 1 of the next; ties 9 and 10 positions apart across both."""
    _three_passes(built, ctx, "c_neighbour_reach")


@pytest.mark.parametrize("name", ["d_every_lane", "d_list_peak", "d_stage_full", "d_stage_flush", "d_walk_window", "d_nothing_passes", "d_final_walk_only", "d_periods"])
def test_list_and_stage(built, ctx, name):
    """d: every lane listing every position (992 entries before each walk, full rounds), the fullest list the model constructs
    (DENSE_LIST - 16), the stage filled to its last entry and the flush one candidate earlier, a walk at an occupancy between the trigger
    and the list's end, an iteration that stages nothing
    between two that do, an iteration whose only walk is the last, tie-dense units of every period."""
    _three_passes(built, ctx, name)


@pytest.mark.parametrize("name", ["e_rejects", "e_strands", "e_family", "e_survivors"])
def test_expansion(built, ctx, name):
    """e: candidates in padding, in N runs and across abutting contigs and assemblies are listed and rejected; both strand
    lists; one candidate with a family's postings among candidates with one; waves with one and with 64 survivors; a wave that
    holds front and back candidates."""
    _three_passes(built, ctx, name)


def test_empty_assemblies(built, ctx):
    """e: an assembly without a contig between two others and as the batch's last entry."""
    case = built["cases"]["e_empty"]
    assert [a.packed().padded_len for a in case.asms][1::2] == [0, 0]
    _three_passes(built, ctx, "e_empty")


@pytest.mark.parametrize("name", ["f_flank_lengths", "f_flank_shapes"])
def test_flanks(built, ctx, name):
    """f: a clean stretch of every length 1..90 between contig ends and N runs, at padded offsets 0 and 32 mod 64 (the edge
    kernel's one-thread and two-thread paths split at 73 / 74); N runs on a contig's first and last base, one base apart, shorter
    than KP_W behind a stretch and into the contig's end; ties inside the flanks and across the hand-over positions."""
    _three_passes(built, ctx, name)


def test_candidates_of_a_displaced_or_unfinished_batch_are_refused(built, ctx):
    """Batch.candidates follows the other stage accessors: it reads the finalised work set of the batch's last pass."""
    pa = built["cases"]["e_family"].asms[0].packed()
    fresh = ctx.batch([pa])
    with pytest.raises(_native.NativeError):
        fresh.candidates()
    batches = [fresh] + [ctx.batch([pa]) for _ in range(_native.WORK_SLOTS)]
    for b in batches:
        b.align()
    front, back = batches[-1].candidates()
    assert len(front) > 0 and len(back) > 0
    with pytest.raises(_native.NativeError, match="no resident alignment results"):
        batches[0].candidates()
    n = _native.lib().kp_batch_candidates(ctx._h, batches[-1]._h, None, C.c_int64(0))
    assert n == 2 + len(front) + len(back)
    small = np.zeros(n - 1, np.uint64)
    assert _native.lib().kp_batch_candidates(ctx._h, batches[-1]._h, _native._p(small), C.c_int64(n - 1)) == -1 and not small.any()  # refused, nothing written
    for b in batches:
        b.close()


def test_candidates_after_a_rerun_are_those_of_the_last_pass(built):
    """A candidate list of one entry overflows: the pass is run again with a grown list, and the accessor returns that pass's
    whole list -- never the first pass's truncated one."""
    world = built["world"]
    c = _native.Context(0)
    c.load_genes(world.codes, world.off)
    c.set_option("cand_cap", 1)
    asms = built["cases"]["e_family"].asms
    model = world.model(asms)
    batch = c.batch([a.packed() for a in asms])
    batch.align()
    assert batch.stats()["retries"] >= 1
    front, back = batch.candidates()
    assert np.array_equal(np.sort(front), model.front) and np.array_equal(np.sort(back), model.back)
    batch.close()
    _run_and_compare(world, c, asms, "e_family after a grown candidate list")
    c.close()
