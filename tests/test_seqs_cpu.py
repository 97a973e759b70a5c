"""kaptive_amd/csrc/kp_seqs.h on the CPU: the N-run search, the base code at a position, the mask of a window's N columns and the
substitution score -- what every fill, walk and extraction of the device asks -- against a numpy mask built from the run list, at
every position of a 200-base sequence."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests.harness_util import build_harness

N = 200
RUN_LISTS = {
    "no run": [],
    "one run of length 1": [(57, 58)],
    "a run at position 0": [(0, 9)],
    "a run ending at the last base": [(181, N)],
    "two runs one base apart": [(40, 47), (48, 60)],
    "two runs that touch": [(40, 47), (47, 60)],
    "a run longer than 32": [(70, 141)],
    "all of them": [(0, 1), (3, 4), (5, 40), (40, 90), (91, 92), (150, N)],
}


@pytest.fixture(scope="module")
def lib():
    h = build_harness("seqs_harness", "kp_seqs.h")
    h.kps_n_mask.restype = C.c_uint32
    return h


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def bases():
    codes = np.random.default_rng(31).integers(0, 4, N).astype(np.uint32)
    words = np.zeros((N + 15) // 16, np.uint32)
    for i, c in enumerate(codes):
        words[i >> 4] |= c << np.uint32(2 * (i & 15))
    return codes.astype(np.int64), words


@pytest.mark.parametrize("name", list(RUN_LISTS))
def test_run_lookups_agree_with_a_mask_at_every_position(lib, bases, name):
    codes, words = bases
    pairs = RUN_LISTS[name]
    runs = np.asarray(pairs, np.int32).reshape(-1)
    runs = np.concatenate([runs, np.zeros(2, np.int32)])  # (never read: a non-empty buffer for the empty list)
    n = len(pairs)
    mask = np.zeros(N, bool)
    for s, e in pairs:
        mask[s:e] = True
    ends = np.asarray([e for _, e in pairs], np.int64)
    for t in range(N):
        assert lib.kps_first_run_after(_p(runs), n, t) == int((ends <= t).sum()), (name, t)
        assert lib.kps_in_n_run(_p(runs), n, t) == int(mask[t]), (name, t)
        assert lib.kps_code_at(_p(words), _p(runs), n, t) == (4 if mask[t] else codes[t]), (name, t)
        # the view of a contig [20, 190): outside it every position reads 5, whatever the runs say
        want = 5 if t < 20 or t >= 190 else (4 if mask[t] else codes[t])
        assert lib.kps_target_code(_p(words), len(words), _p(runs), n, 20, 190, t) == want, (name, t)
    assert lib.kps_first_run_after(_p(runs), n, -1) == 0 and lib.kps_first_run_after(_p(runs), n, N) == n
    # windows of 1, 11 and 32 columns from before position 0 to past the last run
    padded = np.zeros(N + 80, bool)
    padded[40 : 40 + N] = mask
    for width in (1, 11, 32):
        for t0 in range(-40, N + 8):
            want = sum(1 << j for j in range(width) if padded[40 + t0 + j])
            assert lib.kps_n_mask(_p(runs), n, t0, width) == want, (name, width, t0)


def test_query_codes_and_substitution_scores(lib):
    q = np.random.default_rng(32).integers(0, 5, 37).astype(np.uint32)
    nib = np.zeros((len(q) + 7) // 8, np.uint32)
    for i, c in enumerate(q):
        nib[i >> 3] |= c << np.uint32(4 * (i & 7))
    assert [lib.kps_query_code(_p(nib), len(q), r) for r in range(len(q))] == q.tolist()
    for qc in range(6):
        for tc in range(6):  # kp_spec.h: match 2, mismatch -4, anything ambiguous or outside -1
            assert lib.kps_sub_score(qc, tc) == (-1 if qc > 3 or tc > 3 else 2 if qc == tc else -4)
