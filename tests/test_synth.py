"""The synthetic generators that tests and bench.py share draw exactly what they drew before they were made faster."""

import numpy as np
import pytest

from kaptive_amd.synth import _ACGT, _base_probs, random_dna


@pytest.mark.parametrize("gc", [0.0, 0.39, 0.5, 0.57, 1.0])
@pytest.mark.parametrize("n", [0, 1, 3, 1000, (1 << 15) - 1, 1 << 15, (1 << 15) + 1, 200_003])
def test_random_dna_equals_weighted_choice(n, gc):
    a, b = np.random.default_rng(n + 7), np.random.default_rng(n + 7)
    want = _ACGT[a.choice(4, size=n, p=_base_probs(gc))]
    got = random_dna(b, n, gc)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert a.bit_generator.state == b.bit_generator.state  # the draws that follow are the same too
