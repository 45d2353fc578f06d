"""LEAN Solve: a run's capacity from the template's Pareto front (KS_RUN_FRONT).  claim_run_cap takes
the maximum over the front positions still among the claim's options when the claim's first options held every
front member that fitted (the validity bit of try_templates), and over every remaining option otherwise.

Every case is bit-exact parity of the canonical Results with the oracle.  A capacity that came out too small
would leave the Results intact and only split a stretch of identical pods into more steps, so every case also
holds the kernel's steps to the placement sequence (test_claim_run_cross_gpu.py: pops - runPods == stretches +
opening + runCrossLost; the formula needs a Solve without push-backs) and its counters to those the build before
the front existed recorded for the same problem (tests/golden/lean_step_counters.json).

The same cases hold the run's deferred move (KS_RUN_FUSE, off by default; scripts/variant_check.sh runs this file
against a library built with it on): `sorts`, `sortsWithDescent`, `sortsClosed`, `sortsExact`, `runCross`,
`runCrossStops`, `runCrossLost` and `algBytes` count one virtual crossing each and equal the recorded values in
either build, and so does `runCrossClosed`; `runMoves` is one per in-run re-sort without the deferred move and
bounded by the runs, stops and general re-sorts with it (ks_problem_inspect reports which loop was compiled)."""
import json
import os

import pytest

import problems
import run_front_cases as cases
import test_claim_run_cross_gpu as cross
from karpenter_amd import Scheduler
from karpenter_amd.scheduler import inspect
from oracle import bridge

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lean_step_counters.json")) as _f:
    _DOC = json.load(_f)
GOLDEN, CLOSED = _DOC["cases"], _DOC["runCrossClosed"]


def _solve(name):
    mk, claims, errors = cases.CASES[name]
    snap = mk()
    s = json.dumps(snap)
    want, _ = bridge.solve(s)
    want = problems.canonical(want)
    got = Scheduler(s).solve()
    cross._assert_parity(want, got)
    assert (len(want["newNodeClaims"]), len(want["podErrors"])) == (claims, errors), "the case no longer is what it was chosen for"
    st = got.stats
    r = st["route"]
    assert r["family"] == "solve" and r["lean"] == 1
    print("%s: steps %d runs %d runCapFront %d runCapFull %d runCross %d runCrossStops %d runCrossLost %d" % (
        name, st["pops"] - st["runPods"], st["runs"], st["runCapFront"], st["runCapFull"], st["runCross"],
        st["runCrossStops"], st["runCrossLost"]))
    for key in cases.PINNED:
        assert st[key] == GOLDEN[name][key], "%s: %s is %d, %d before the front" % (name, key, st[key], GOLDEN[name][key])
    # the in-run re-sorts are the crossings continued and refused; as many of them as before take the closed form.
    # KS_RUN_FUSE: the run's claim moves in the position arrays once per run, stop and general re-sort at most
    in_run = st["runCross"] + st["runCrossStops"]
    fused = inspect(snap)["runFuse"]
    print("%s: runFuse %d runCrossClosed %d runMoves %d in-run re-sorts %d" % (name, fused, st["runCrossClosed"], st["runMoves"], in_run))
    assert st["runCrossClosed"] == CLOSED[name]
    if fused:
        assert st["runMoves"] <= st["runs"] + st["runCrossStops"] + in_run - st["runCrossClosed"]
    else:
        assert st["runMoves"] == in_run
    if not errors:
        stretches, opening = cross._placement_stretches(snap, want)
        assert st["pops"] - st["runPods"] == stretches + opening + st["runCrossLost"]
    return st


@pytest.mark.parametrize("name", ["front3_115", "front3_31"])
def test_non_chain_front_with_a_tie(name):
    """n >= 50 and 12 < n < 50 NodeClaims, ending on cpu-big, mem-big and pods-big (run_front_cases.non_chain)."""
    st = _solve(name)
    assert st["runCapFront"] > 0
    assert st["runCapFull"] == 0
    assert st["runCross"] > 0


def test_chain_catalogue_takes_the_front_only():
    st = _solve("chain_64")
    assert st["runCapFront"] > 0
    assert st["runCapFull"] == 0


@pytest.mark.parametrize("name", ["notin_top_66", "small_only_111"])
def test_requirements_that_exclude_a_front_member_clear_the_bit(name):
    """The template's requirements keep the dominating instance type(s) out of every NodeClaim: the front no
    longer bounds the remaining options and the capacity is the full scan's."""
    st = _solve(name)
    assert st["runCapFull"] > 0


def test_nodepool_limit():
    """1870 pods fail and are pushed back (the stretch formula does not apply; the steps are the recorded ones).
    The limit is spent by whole NodeClaims of the largest type, so no claim ever lacks the front member."""
    st = _solve("pool_limit_25")
    assert st["runCapFront"] > 0
    assert st["runCapFull"] == 0


def test_nodepool_limit_that_excludes_the_front_member_clears_the_bit():
    """The limit's remainder admits only the smaller types for the last NodeClaim: its capacity is the full scan's."""
    st = _solve("pool_limit_part_25")
    assert st["runCapFront"] > 0
    assert st["runCapFull"] > 0


@pytest.mark.parametrize("name", ["cross_11", "cross_46", "cross_56", "cross_151"])
def test_re_sort_shapes_keep_their_counters(name):
    """The shapes of test_claim_run_cross_gpu.py (chain_64 above is the fifth): every path of the re-sort."""
    st = _solve(name)
    assert st["runCapFront"] > 0
    assert st["runCapFull"] == 0
    if name in ("cross_56", "cross_151") and inspect(cases.CASES[name][0]())["runFuse"]:
        assert st["runCross"] > st["runMoves"]  # heavily tied counts: some run crosses two tie blocks or more in one move
