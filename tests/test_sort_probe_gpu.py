"""The claim re-sort of the Solve kernel run on arrays of the test's choosing (ks_claim_sort_probe: one wave loads
keys / order into LDS, fills the two other position arrays from claim tables and runs Solver::sort_claims' logic;
no Solve), compared by exact equality with the same entry's host mode, Go's pdqsort_func of csrc/ks_gosort.h.

  mode 0   the general path: the wave-parallel leaves (<= 12 entries, KS_SORT_LEAF), partialInsertionSort, the
           exact pdqsort with its partitions, the reversal of a decreasing array;
  mode 1   the path after a count increment at `pos`: the closed form (KS_CLOSED_SHIFT) over tie blocks that end
           on and around the 64-entry chunks and the 256-entry batches, with the crossing at the array's start,
           on a chunk edge and ending at the last position.

Every case also compares the position arrays the kernel kept (ptpl / phead) with a regather computed here."""
import random

import numpy as np
import pytest

from karpenter_amd import claim_sort_probe, inspect, synth
from test_sort_single_descent import closed_applies

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 11, 12, 13, 24, 25, 49, 50, 51, 63, 64, 65, 127, 128, 129, 300)
R = 3


@pytest.fixture(scope="module")
def build():
    return inspect(synth.config2(10))


def tables(n, r=R):
    """Per-claim template and headroom values no two claims share, the headroom beyond 32 bits."""
    ct = np.array([(c * 7 + 3) % 64 for c in range(n)], dtype=np.int32)
    ch = np.array([[(c << 33) + c * 1000003 + 17 * k - 5 for k in range(r)] for c in range(n)], dtype=np.int64).reshape(n, r)
    return ct, ch


def run(keys, mode=0, pos=-1, seed=0, r=R):
    n = len(keys)
    order = list(range(n))
    random.Random(seed * 7919 + n).shuffle(order)  # claim ids are not positions
    ct, ch = tables(n, r)
    want = claim_sort_probe(keys, order, ct, ch, mode=mode, pos=pos, device=-1)
    got = claim_sort_probe(keys, order, ct, ch, mode=mode, pos=pos, device=0)
    what = "n %d mode %d pos %d keys %s" % (n, mode, pos, list(keys)[:80])
    assert list(want[0]) == sorted(keys), what
    assert sorted(want[1]) == list(range(n)), what
    assert list(got[0]) == list(want[0]), "keys: " + what
    assert list(got[1]) == list(want[1]), "order: got %s want %s: %s" % (list(got[1])[:80], list(want[1])[:80], what)
    o = np.array(got[1], dtype=np.int64)
    assert np.array_equal(got[2], ct[o]) and np.array_equal(got[2], want[2]), "ptpl: " + what
    assert np.array_equal(got[3], ch[o].reshape(n, r)) and np.array_equal(got[3], want[3]), "phead: " + what
    return got[4]


def incremented(n, at):
    """Non-decreasing with ties of three, the entry at `at` lifted by one (a descent when its right neighbour tied)."""
    k = [i // 3 for i in range(n)]
    k[at] += 1
    return k


@pytest.mark.parametrize("n", LENGTHS)
def test_general_path_against_go(n):
    run([5] * n)
    run(list(range(n)))
    run(list(range(n, 0, -1)))  # choosePivot's decreasing hint from 50 entries on
    rng = random.Random(n)
    for vals in (2, max(n // 2, 1)):
        for rep in range(3):
            run([rng.randint(1, vals) for _ in range(n)], seed=rep)
    if n >= 2:
        for at in sorted({0, n // 2, n - 2}):
            k = incremented(n, at)
            run(k)
            run(k, mode=1, pos=at)


@pytest.mark.parametrize("r", (3, 4))
def test_both_resource_counts(r):
    k = incremented(131, 66)
    assert run(k, mode=1, pos=66, r=r) in (0, 2)
    assert run(list(range(70, 0, -1)), r=r) == 1


def crossing(pre, t, suf):
    """`pre` entries of keys <= 5, the claim with key 6 at pos = pre, a tie block of t entries with key 5, `suf`
    entries of keys >= 6 (the first five tie with the claim: it stops before them)."""
    return [min(5, 1 + i // 16) for i in range(pre)] + [6] + [5] * t + [6 + i // 5 for i in range(suf)], pre


@pytest.mark.parametrize("t", (0, 1, 63, 64, 65, 255, 256, 257))
def test_closed_form_tie_blocks(t, build):
    closed = 0
    for pre, suf in ((0, 60), (63, 60), (64, 60), (max(10, 60 - t), 0)):
        keys, pos = crossing(pre, t, suf)
        n = len(keys)
        assert n >= 50 and (suf or pos + t == n - 1)
        how = run(keys, mode=1, pos=pos)
        applies = closed_applies([(k, i) for i, k in enumerate(keys)], pos)
        assert applies == (t > 0)  # the case is the closed form's: choosePivot's samples miss the descent
        if build["closedShift"]:
            assert (how == 2) == applies, (pre, t, suf, how)
        else:
            assert how in (0, 2) and (how != 2 or applies), (pre, t, suf, how)
        closed += how == 2
        assert run(keys, mode=0) != 2  # the same array as an appended claim's: never the closed form
    if t > 0 and build["closedShift"]:
        assert closed == 4, "the tie block of %d must go through the closed form: %d of 4" % (t, closed)
