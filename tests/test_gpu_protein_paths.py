"""Every path of the protein DP (kaptive_amd/csrc/kp_prot.hip) in both modes against the oracle, bit for bit, on the case
tables of tests/protein_paths_util.py (run with -m gpu on an MI355X).

tests/test_protein_paths_cpu.py shows without a GPU that those tables reach every path and both sides of every
threshold and that the oracle's seeded mode equals the reference at bands other than the comparator's; here the device
equals the oracle on them, the reference-recorded seeded fixture included, and on batches large enough that a block of
kp_protein_kernel goes round its pair loop twice."""

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.core.seq import Sequences
from tests import protein_paths_util as U

pytestmark = pytest.mark.gpu

KP_EINVAL = -1  # include/kaptive_amd.h


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _run(aligner, q, t, offsets=None, k=None):
    if offsets is None:
        return aligner.protein_align(q.seqs, q.offsets, q.lengths, t.seqs, t.offsets, t.lengths)
    return aligner.protein_align_seeded(q.seqs, q.offsets, q.lengths, t.seqs, t.offsets, t.lengths, np.asarray(offsets, np.int32), k)


def _differences(cases, paths, want, got) -> list[str]:
    return [
        f"{name}: path {path}, {len(q)} x {len(t)} residues, offset {off}, k {k}: oracle {want[i].tolist()} device {got[i].tolist()}"
        for i, ((name, q, t, off, k), path) in enumerate(zip(cases, paths)) if (want[i] != got[i]).any()
    ]  # fmt: skip


def test_seeded_kernel_equals_the_reference_recorded_fixture(ctx, golden_dir):
    z = np.load(golden_dir / "protein_dp_seeded.npz")
    want = np.stack([z[c] for c in U.COLS], axis=1)
    for k in U.GOLDEN_KS:
        sel = np.flatnonzero(z["k"] == k)
        assert len(sel) > 40
        got = ctx.protein_align_seeded(z["q_seqs"], z["q_offsets"][sel], z["q_lengths"][sel], z["t_seqs"], z["t_offsets"][sel],
                                       z["t_lengths"][sel], z["offsets"][sel], k)  # fmt: skip
        bad = np.flatnonzero((got != want[sel]).any(axis=1))
        assert len(bad) == 0, (k, z["names"][sel[bad[:3]]], z["offsets"][sel[bad[:3]]], want[sel[bad[:3]]], got[bad[:3]])


def test_unseeded_table_equals_oracle(ctx, oracle):
    cases = U.unseeded_table()
    paths = U.classify(cases)
    q, t = U.pack(cases)
    want, got = _run(oracle, q, t), _run(ctx, q, t)
    bad = _differences(cases, paths, want, got)
    assert not bad, f"{len(bad)} of {len(cases)} differ:\n" + "\n".join(bad[:8])
    # the same pair beside three narrow neighbours (`narrow` true) and beside a 51-diagonal one (false)
    pairs = U.company_pairs(cases)
    assert len(pairs) == 3
    for a, b in pairs:
        assert (paths[a], paths[b]) == ("quad3", "quad4") and np.array_equal(got[a], got[b]) and got[a, 0] > 0, (cases[a][0], got[a], got[b])


def test_seeded_table_equals_oracle(ctx, oracle):
    groups = U.by_k(U.seeded_table())
    assert tuple(groups) == U.SEEDED_KS
    bad, n = [], 0
    for k, cases in groups.items():  # one call per k
        q, t = U.pack(cases)
        offs = [c[3] for c in cases]
        bad += _differences(cases, U.classify(cases), _run(oracle, q, t, offs, k), _run(ctx, q, t, offs, k))
        n += len(cases)
    assert not bad, f"{len(bad)} of {n} differ:\n" + "\n".join(bad[:8])


@pytest.fixture(scope="module")
def big(oracle):
    """The two big batches with the oracle's rows in both modes, computed once."""
    out = {}
    for wide in (False, True):
        qs, ts, offs = U.big_batch(wide=wide)
        q, t = Sequences.from_bytes(qs), Sequences.from_bytes(ts)
        out[wide] = (qs, ts, offs, q, t, _run(oracle, q, t), _run(oracle, q, t, offs, U.BIG_K))
    return out


@pytest.mark.parametrize("wide", (False, True), ids=("small_pairs", "with_wide_pairs"))
@pytest.mark.parametrize("seeded", (False, True), ids=("unseeded", "seeded"))
def test_big_batch_equals_oracle_in_any_order(ctx, big, wide, seeded):
    """20 003 pairs on 4096 blocks: 905 blocks stage a second quad in the LDS their first one used, and the last quad
    holds three pairs.  A pair's row must depend neither on its neighbours nor on its block: the batch permuted gives
    every pair the same row."""
    qs, ts, offs, q, t, want_plain, want_seeded = big[wide]
    want = want_seeded if seeded else want_plain
    assert len(qs) == U.BIG_N > 4 * U.BIG_BLOCKS and (want[:, 0] > 0).sum() > 15000
    got = _run(ctx, q, t, offs if seeded else None, U.BIG_K if seeded else None)
    bad = np.flatnonzero((want != got).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], bad[:5] // 4 >= U.BIG_BLOCKS, want[bad[:3]], got[bad[:3]], q.lengths[bad[:3]], t.lengths[bad[:3]])
    perm = np.random.default_rng(77).permutation(U.BIG_N)
    qp, tp = Sequences.from_bytes([qs[i] for i in perm]), Sequences.from_bytes([ts[i] for i in perm])
    got_p = _run(ctx, qp, tp, offs[perm] if seeded else None, U.BIG_K if seeded else None)
    bad = np.flatnonzero((got_p != got[perm]).any(axis=1))
    assert len(bad) == 0, (len(bad), perm[bad[:5]], got[perm[bad[:3]]], got_p[bad[:3]])


def test_seeded_entry_refuses_bad_arguments_and_goes_on(ctx, oracle):
    lib = _native.lib()
    k = 8
    cases = [c for c in U.golden_seeded_table() if c[4] == k][:8]
    q, t = U.pack(cases)
    offs = np.array([c[3] for c in cases], np.int32)
    n = len(cases)
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)  # noqa: E731
    q_off, q_len, t_off, t_len = (np.ascontiguousarray(a, np.int32) for a in (q.offsets, q.lengths, t.offsets, t.lengths))

    def call(q_len_=q_len, offs_=offs, k_=k):
        out = np.full((n, 8), -7, np.int32)
        rc = lib.kp_protein_align_seeded(ctx._h, p(q.seqs), p(q_off), p(q_len_), p(t.seqs), p(t_off), p(t_len), C.c_int32(n),
                                         None if offs_ is None else p(offs_), C.c_int32(k_), p(out))  # fmt: skip
        return rc, out

    too_long = q_len.copy()
    too_long[3] = 65536
    for what, kw in (("k = -1", dict(k_=-1)), ("null offsets", dict(offs_=None)), ("a length of 65536", dict(q_len_=too_long))):
        rc, out = call(**kw)
        assert rc == KP_EINVAL and (out == -7).all(), (what, rc)
        assert lib.kp_last_error(ctx._h), what
        with pytest.raises(ValueError):
            ctx._check(rc, what)
    want = _run(oracle, q, t, offs, k)
    rc, out = call()
    assert rc == 0 and np.array_equal(out, want) and (want[:, 0] > 0).any()
    assert np.array_equal(_run(ctx, q, t, offs, k), want)  # the context still answers
    none = np.zeros(0, np.int32)
    empty = ctx.protein_align_seeded(np.zeros(0, np.uint8), none, none, np.zeros(0, np.uint8), none, none, none, 20)
    assert empty.shape == (0, 8) and ctx.protein_align(np.zeros(0, np.uint8), none, none, np.zeros(0, np.uint8), none, none).shape == (0, 8)
    assert lib.kp_protein_align_seeded(ctx._h, None, None, None, None, None, None, C.c_int32(0), None, C.c_int32(20), None) == 0
