"""The register-copy claim re-sort (csrc/ks_sort_regs.h, KS_SORT_REGS) proven on the host: ks_claim_sort_probe's
device -2 runs the algorithm the kernel runs, its wave operations (ballot, readlane, per-lane select, bpermute /
permute) emulated over 64 lanes held in plain arrays, and device -1 runs Go's pdqsort_func (csrc/ks_gosort.h).  Keys
and order must be equal entry for entry: the replay is swap for swap, so ties land where Go leaves them.

Every length 0 .. 128 goes through the copy; 129 and 300 are more than it holds (path 3) and must still agree.  Device
-3 is the copy's 64-entry form (KS_SORT_REGS_N64, the shipped one), which holds 64.  Path 2, an invariant that failed
inside the copy, must never show."""
import random

import numpy as np
import pytest

from karpenter_amd import claim_sort_probe
from sort_regs_cases import lifted, shuffled_order, small_first, tables, unbalanced

LENGTHS = list(range(0, 129)) + [129, 300]


def both(keys, mode=0, pos=-1, seed=0, device=-2):
    n = len(keys)
    order = shuffled_order(n, seed)
    ct, ch = tables(n)
    want = claim_sort_probe(keys, order, ct, ch, mode=mode, pos=pos, device=-1)
    got = claim_sort_probe(keys, order, ct, ch, mode=mode, pos=pos, device=device, path=True)
    what = "n %d mode %d pos %d device %d keys %s" % (n, mode, pos, device, list(keys)[:130])
    assert list(want[0]) == sorted(keys), what
    assert list(got[0]) == list(want[0]), "keys: " + what
    assert list(got[1]) == list(want[1]), "order: got %s want %s: %s" % (list(got[1]), list(want[1]), what)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), "position arrays: " + what
    cap = 128 if device == -2 else 64
    assert got[5] & 0xff == (1 if n <= cap else 3), "path %d: %s" % (got[5], what)
    return got[5] >> 8 & 0xfff  # breakPatterns calls


def inputs(n):
    yield [5] * n
    yield list(range(n))
    yield list(range(n, 0, -1))
    rng = random.Random(n)
    for vals in (2, max(n // 2, 1)):
        for _ in range(3):
            yield [rng.randint(1, vals) for _ in range(n)]


@pytest.mark.parametrize("n", LENGTHS)
def test_lane_model_equals_go(n):
    for device in (-2, -3):
        for seed, keys in enumerate(inputs(n)):
            both(keys, seed=seed, device=device)
        if n >= 2:
            for keys, pos in lifted(n):
                both(keys, mode=0, device=device)
                both(keys, mode=1, pos=pos, device=device)


def test_break_patterns_and_the_reversal_run_on_the_copy():
    """The regimes tests/test_sort_regs_gpu.py relies on: an unbalanced first partition reaches breakPatterns, and
    a decreasing array of 50 entries or more is reversed, both without leaving the register copy."""
    for n in (14, 50, 64, 65, 128):
        assert both(unbalanced(n)) >= 1, n
        both(small_first(n))
        both(list(range(n, 0, -1)))
    for n in (14, 50, 64):
        assert both(unbalanced(n), device=-3) >= 1, n
    assert both(unbalanced(13)) == 0  # 13 entries cannot reach it: a first partition leaves 12, a leaf
