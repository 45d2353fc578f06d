"""choosePivot's hint by arithmetic (KS_PIVOT_ARITH) and the appended claim's closed form (KS_APPEND_CLOSED) in the Solve
kernel's claim re-sort, through the probe (ks_claim_sort_probe mode 1: Solver::sort_claims' top frame after
a count crossing at `pos`; ks_claim_sort_probe_append: after an appended claim) and through the Solve.

Probe: device against the entry's host mode (Go's pdqsort_func), exact equality of all four arrays (test_sort_probe_gpu's
`run`), and which path ran: with the arithmetic form compiled in, a confirmed descent takes the closed form exactly off
the six positions l-1, l, 2l-1, 2l, 3l-1, 3l (tests/test_pivot_arith_model.py); on them the sampled hint is not
"increasing" and the general re-sort runs.  Without it (-DKS_PIVOT_ARITH=0) the sampled hint gives the same split.

The append entry: device against Go's sort in the same way, the new claim landing behind the last count not above its
own, and whether the closed form ran (it must, from 50 entries on, when it is compiled in).

Solve: parity with the oracle on four recorded shapes, and the counters -- every closed-form re-sort was decided without
samples, some crossing of cross_151 sits on a sample position, the self-check build counts no disagreement, every
appended claim's re-sort at 50 claims and more took its closed form."""
import random

import numpy as np
import pytest

import run_front_cases
from karpenter_amd import claim_sort_probe_append, inspect, synth
from test_lean_step_gpu import _assert_parity, _lean, _solve_both
from test_pivot_arith_model import cells, crossed, sample_positions
from test_sort_probe_gpu import crossing, run, tables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def build():
    return inspect(synth.config2(10))


def _check(keys, pos, r=3):
    n = len(keys)
    assert n >= 50 and keys[pos] > keys[pos + 1]
    how = run(keys, mode=1, pos=pos, r=r)
    if pos in sample_positions(n):
        assert how in (0, 1), "a crossing on a sample position is the general re-sort's: n %d pos %d how %d" % (n, pos, how)
    else:
        assert how == 2, "a crossing off the sample positions is the closed form's: n %d pos %d how %d" % (n, pos, how)
    return how


@pytest.mark.parametrize("n", (50, 51, 52, 53, 64, 65, 122, 129))
def test_every_position(n):
    ties = [i // 3 for i in range(n)]
    closed = sum(_check(crossed(ties, pos), pos) == 2 for pos in range(n - 1))
    assert closed == n - 1 - 6
    for pos in cells(n):  # one tie block to the end of the array: the longest move
        _check(crossed([5] * n, pos), pos)


@pytest.mark.parametrize("n", (257, 321, 1024))
def test_cells_around_the_samples(n):
    for base in ([i // 3 for i in range(n)], [5] * n, [2 * i for i in range(n)]):
        hows = [_check(crossed(base, pos), pos, r=3 + (n & 1)) for pos in cells(n)]
        assert sum(h == 2 for h in hows) == len(hows) - 6


@pytest.mark.parametrize("t", (63, 64, 65, 255, 256, 257))
def test_tie_blocks_at_the_chunk_and_batch_edges(t):
    """The block the claim is lifted over ends 63 / 64 / 65 and 255 / 256 / 257 entries past pos: closed_move's and
    closed_crossing's 64-entry chunks and 256-entry batches."""
    closed = 0
    for pre, suf in ((0, 60), (5, 60), (63, 60), (64, 60), (70, 0)):
        keys, pos = crossing(pre, t, suf)
        assert suf or pos + t == len(keys) - 1
        closed += _check(keys, pos) == 2
    assert closed == 5  # none of these positions is a sample's


def _append(keys, r, seed=0):
    n = len(keys)
    order = list(range(n - 1))
    random.Random(seed * 7919 + n).shuffle(order)  # claim ids are not positions; the new claim has the last id
    order.append(n - 1)
    ct, ch = tables(n, r)
    want = claim_sort_probe_append(keys, order, ct, ch, device=-1)
    got = claim_sort_probe_append(keys, order, ct, ch, device=0)
    what = "n %d r %d keys %s" % (n, r, list(keys)[:80])
    assert list(want[0]) == sorted(keys) and sorted(want[1]) == list(range(n)), what
    assert list(got[0]) == list(want[0]), "keys: " + what
    assert list(got[1]) == list(want[1]), "order: got %s want %s: %s" % (list(got[1])[:80], list(want[1])[:80], what)
    o = np.array(got[1], dtype=np.int64)
    assert np.array_equal(got[2], ct[o]) and np.array_equal(got[2], want[2]), "ptpl: " + what
    assert np.array_equal(got[3], ch[o].reshape(n, r)) and np.array_equal(got[3], want[3]), "phead: " + what
    return got[4], got[5], list(got[1]).index(n - 1)


@pytest.mark.parametrize("r", (3, 4))
@pytest.mark.parametrize("n", (50, 64, 65, 129, 130, 257, 1024))
def test_appended_claim(n, r, build):
    """The new claim (count 1, the last id) behind p claims of count 1 and n - 1 - p greater ones: p = 0, around the
    64-entry chunk of the count and at n - 2, the moved block of n - 1 - p entries across the shift's chunks."""
    for p in sorted({0, 1, 63, 64, 65, n - 2}):
        if p > n - 2:
            continue
        keys = [1] * p + [3 + (i * 5) // n for i in range(n - 1 - p)] + [1]
        how, taken, at = _append(keys, r, seed=p)
        assert at == p and how == 0, (n, p, how, at)
        assert taken == build["appendClosed"], (n, p, taken)
    how, taken, at = _append([0] * 7 + [2] * (n - 8) + [1], r)  # no count equal to the new one
    assert (how, taken, at) == (0, build["appendClosed"], 7)


def test_appended_claim_refusals(build):
    """Below 50 entries and with a last entry not below its neighbour the kernel sorts as before."""
    how, taken, at = _append([1] * 5 + [3] * 43 + [1], 3)  # n = 49: the general pdqsort (the tie order is Go's)
    assert taken == 0 and how == 1 and at <= 5
    how, taken, at = _append([1] * 30 + [3] * 33 + [3], 3)  # sorted already: partialInsertionSort finds no descent
    assert (how, taken, at) == (0, 0, 63)
    how, taken, at = _append([1] * 30 + [3] * 33 + [4], 4)
    assert (how, taken, at) == (0, 0, 63)


SOLVES = ("cross_151", "small_only_111", "front3_115", "chain_64")


@pytest.mark.parametrize("name", SOLVES)
def test_solve_counters(name, build):
    mk, claims, errors = run_front_cases.CASES[name]
    want, got = _solve_both(mk())
    _assert_parity(want, got)
    assert (len(want["newNodeClaims"]), len(want["podErrors"])) == (claims, errors)
    assert _lean(got)
    st = got.stats
    print("%s: sortsWithDescent %d sortsCross50 %d sortsClosed %d pivotArith %d sortsExact %d pivotArithDiff %d" % (
        name, st["sortsWithDescent"], st["sortsCross50"], st["sortsClosed"], st["pivotArith"], st["sortsExact"],
        st["pivotArithDiff"]))
    assert st["sortsClosed"] > 0 and st["sortsCross50"] >= st["sortsClosed"]
    assert st["pivotArithDiff"] == 0
    if build["pivotArith"]:
        assert st["pivotArith"] == st["sortsClosed"]
    else:
        assert st["pivotArith"] == 0
    print("%s: sortsAppend50 %d appendClosed %d" % (name, st["sortsAppend50"], st["appendClosed"]))
    assert st["sortsAppend50"] > 0
    assert st["appendClosed"] == (st["sortsAppend50"] if build["appendClosed"] else 0)
    if name == "cross_151":  # some crossing sits on a sample position
        assert st["sortsExact"] == 107
        assert st["sortsClosed"] < st["sortsCross50"]
