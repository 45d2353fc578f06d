"""The register-copy claim re-sort on the device (KS_SORT_REGS, csrc/ks_sort_regs.h): ks_claim_sort_probe's kernel
against Go's pdqsort_func on the host (device -1) by exact equality of all four arrays, with the path the general
re-sort took -- 1: it finished on the copy held in registers (up to 64 entries as shipped, 128 in a
-DKS_SORT_REGS_N64=0 build), 3: more entries than the copy holds, so the LDS code sorted them, 2: the copy was
abandoned on a failed invariant, which must never show -- and small LEAN Solves whose counters show the same inside
k_solve (sortsRegs, sortRegsOver, sortRegsBail).
tests/test_sort_regs_model.py proves the same algorithm on the host's lane model first.

The assertions follow ks_problem_inspect's "sortRegs" / "sortRegsN64": the shipped build holds 64 entries
(KS_SORT_REGS_N64=1: the 128-entry form measured slower), so there 65..128 entries report path 3 as 129
does; the -DKS_SORT_REGS_N64=0 build must report the copy up to 128, and a build without it (-DKS_SORT_REGS=0)
path 0 and zero counters.  scripts/variant_check.sh runs this file on those builds."""
import json
import random

import numpy as np
import pytest

import problems
import run_front_cases
from karpenter_amd import Scheduler, claim_sort_probe, inspect, synth
from oracle import bridge
from sort_regs_cases import R, lifted, shuffled_order, tables, unbalanced

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def build():
    return inspect(synth.config2(10))


def cap(build):
    """Entries the register copy takes in this build (0: compiled out)."""
    return 0 if not build["sortRegs"] else 64 if build["sortRegsN64"] else 128


def run(build, keys, mode=0, pos=-1, seed=0):
    n = len(keys)
    order = shuffled_order(n, seed)
    ct, ch = tables(n)
    want = claim_sort_probe(keys, order, ct, ch, mode=mode, pos=pos, device=-1)
    got = claim_sort_probe(keys, order, ct, ch, mode=mode, pos=pos, device=0, path=True)
    what = "n %d mode %d pos %d keys %s" % (n, mode, pos, list(keys)[:130])
    assert list(got[0]) == list(want[0]), "keys: " + what
    assert list(got[1]) == list(want[1]), "order: got %s want %s: %s" % (list(got[1]), list(want[1]), what)
    o = np.array(got[1], dtype=np.int64)
    assert np.array_equal(got[2], ct[o]) and np.array_equal(got[2], want[2]), "ptpl: " + what
    assert np.array_equal(got[3], ch[o].reshape(n, R)) and np.array_equal(got[3], want[3]), "phead: " + what
    how, path = got[4], got[5]
    if how == 2 or not cap(build):
        assert path == 0, "path %d how %d: %s" % (path, how, what)
    else:  # the general re-sort ran: on the copy up to its capacity, beyond it on LDS; never an invariant bail-out
        assert path == (1 if n <= cap(build) else 3), "path %d how %d: %s" % (path, how, what)
    return how, path


SWEEP = sorted(set(range(13, 129, 5)) | {13, 49, 50, 51, 63, 64, 65, 127, 128})


@pytest.mark.parametrize("n", SWEEP)
def test_single_increment_sweep(n, build):
    for keys, pos in lifted(n):
        run(build, keys, mode=0)
        run(build, keys, mode=1, pos=pos)


def test_129_entries_exceed_the_copy(build):
    general = 0
    for keys, pos in lifted(129):
        general += run(build, keys, mode=0)[1] == 3
        run(build, keys, mode=1, pos=pos)
    how, path = run(build, list(range(129, 0, -1)))
    assert how == 1 and path == (3 if cap(build) else 0)
    assert general > 0 or not cap(build)


@pytest.mark.parametrize("n", (13, 50, 64, 65, 128))
def test_random_decreasing_and_tied_arrays(n, build):
    how, _ = run(build, list(range(n, 0, -1)))  # choosePivot's decreasing hint, and the reversal, from 50 entries on
    assert how == 1
    rng = random.Random(n)
    for vals in (2, max(n // 2, 1), 1000):  # 2: heavy ties, partitionEqual
        for rep in range(3):
            run(build, [rng.randint(1, vals) for _ in range(n)], seed=rep)


@pytest.mark.parametrize("n", (50, 64, 65, 128))
def test_break_patterns(n, build):
    """An unbalanced first partition: the continuing frame calls breakPatterns, which runs on the copy through
    GoSortT's own code.  The host's lane model counts the calls (13 entries cannot reach one: what a first partition
    leaves is a leaf)."""
    keys = unbalanced(n)
    order = shuffled_order(n)
    ct, ch = tables(n)
    model = claim_sort_probe(keys, order, ct, ch, device=-2, path=True)
    assert model[5] & 0xff == 1 and (model[5] >> 8 & 0xfff) >= 1, "the array no longer reaches breakPatterns"
    how, _ = run(build, keys)
    assert how == 1


# (case of run_front_cases.CASES, sortsExact of the build without the register copy: tests/golden/
# lean_step_counters.json, recorded before the copy existed and reproduced by the -DKS_SORT_REGS=0 build)
SOLVES = [("chain_64", 205), ("cross_46", 318)]


@pytest.mark.parametrize("case,exact", SOLVES)
def test_lean_solve_sorts_from_registers(case, exact, build):
    builder, claims, _ = run_front_cases.CASES[case]
    s = json.dumps(builder())
    want, _ = bridge.solve(s)
    got = Scheduler(s).solve()
    assert problems.canonical(want) == got.canonical()
    assert len(want["newNodeClaims"]) == claims and claims > 12
    st = got.stats
    print("sorts %d withDescent %d exact %d closed %d sortsRegs %d sortRegsOver %d sortRegsBail %d" % (
        st["sorts"], st["sortsWithDescent"], st["sortsExact"], st["sortsClosed"], st["sortsRegs"], st["sortRegsOver"],
        st["sortRegsBail"]))
    assert st["route"]["family"] == "solve" and st["route"]["lean"] == 1
    assert st["sortsExact"] == exact
    assert st["sortRegsBail"] == 0 and st["sortRegsOver"] == 0
    if cap(build) >= claims:
        # every general re-sort, exact or finished by partialInsertionSort, ran on the copy
        assert st["sortsRegs"] == st["sortsWithDescent"] - st["sortsClosed"] and st["sortsRegs"] >= exact
    elif not cap(build):
        assert st["sortsRegs"] == 0


def test_lean_solve_past_128_claims_counts_what_exceeds_the_copy(build):
    builder, claims, _ = run_front_cases.CASES["cross_151"]
    s = json.dumps(builder())
    want, _ = bridge.solve(s)
    got = Scheduler(s).solve()
    assert problems.canonical(want) == got.canonical()
    assert len(want["newNodeClaims"]) == claims == 151
    st = got.stats
    assert st["sortsExact"] == 107  # (the recorded value, as above)
    assert st["sortRegsBail"] == 0  # no invariant failed
    assert st["sortsRegs"] + st["sortRegsOver"] == (st["sortsWithDescent"] - st["sortsClosed"] if cap(build) else 0)
    if cap(build):
        assert st["sortsRegs"] > 0 and st["sortRegsOver"] > 0
