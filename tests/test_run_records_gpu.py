"""LEAN Solve: a run of identical pods that reaches past the 64-pod queue window, while nothing was pushed back, is
logged as one record (first log entry, first queue position, pods, claim); k_log_expand writes the per-pod
commit-log entries after the Solve (KS_LOG_RUNS).  The wave's own block stores are masked so that the
two kernels write disjoint entries.  Every case is bit-exact parity of the canonical Results with the oracle --
each NodeClaim's pods in commit order among them -- with the commit count and the record count (runRecs)."""
import json

import pytest

import problems
from karpenter_amd import Scheduler, inspect, synth
from oracle import bridge

pytestmark = pytest.mark.gpu

RUN_LENGTHS = [63, 64, 65, 127, 128, 129, 200]
# single placements before the run (pods of pairwise different requests, one step each).  The run's first log
# entry lands at 2 for 0 and 1 (the class's first pod opens the NodeClaim or lands on it, the next commit starts
# the run), at 63 -- the last lane of a block -- for 62 and on a block boundary for 63.
SINGLES = [0, 1, 62, 63]


def _records_built():
    return inspect(synth.benchmark_snapshot(1, 1, 1, diverse=False))["logRuns"] == 1


def _solve_both(snap, **kw):
    s = json.dumps(snap)
    want, _ = bridge.solve(s)
    got = Scheduler(s).solve(**kw)
    return problems.canonical(want), got


def _assert_parity(want, got):
    g = got.canonical()
    for key in ("newNodeClaims", "existingNodes", "podErrors"):
        if want[key] != g[key] and isinstance(want[key], list):
            for i, (a, b) in enumerate(zip(want[key], g[key])):
                assert a == b, "%s[%d]: want %s\n got %s" % (key, i, json.dumps(a)[:1500], json.dumps(b)[:1500])
        assert want[key] == g[key], key
    assert want == g


def _lean(got):
    r = got.stats["route"]
    return r["family"] == "solve" and r["lean"] == 1


def _snapshot(pods, pods_per_claim=1000):
    snap = synth.benchmark_snapshot(0, 1, 1, diverse=False)
    snap["instanceTypes"] = [synth.fake_instance_type("fake-it-big", 256, 512, pods=pods_per_claim)]
    snap["pods"] = pods
    return snap


def _single(i, k):
    """The k-th single placement: more cpu than the run's class (popped before it), no two alike."""
    return synth.pod(i, cpu="%dm" % (1000 + 10 * (64 - k)), mem="1Gi")


def _run_pods(first, n):
    return [synth.pod(first + i, cpu="100m", mem="100Mi") for i in range(n)]


@pytest.mark.parametrize("singles", SINGLES)
def test_one_run_past_the_window(singles):
    built = _records_built()
    for length in RUN_LENGTHS:
        n = length + (1 if singles else 2)
        snap = _snapshot([_single(i, i) for i in range(singles)] + _run_pods(singles, n))
        want, got = _solve_both(snap)
        _assert_parity(want, got)
        assert len(want["newNodeClaims"]) == 1 and not want["podErrors"]
        st = got.stats
        print("singles %d length %d runs %d runPods %d runRecs %d" % (singles, length, st["runs"], st["runPods"], st["runRecs"]))
        assert _lean(got)
        assert (st["runs"], st["runPods"]) == (1, length), (singles, length)
        assert st["ncommits"] == len(snap["pods"])
        # the run starts at window lane singles + 2 at most and has at least 63 pods: it ends past lane 64
        assert st["runRecs"] == (1 if built else 0), (singles, length)


def test_one_record_per_claim_filling_run():
    """NodeClaims of 130 pods and 410 pods of one class: each of the first three claims takes its first pod from
    the template phase, its second from a commit and 128 in one run that ends past the window (a record each, in
    blocks the singles between them share); the last claim's run of 18 lies inside the refilled window."""
    snap = _snapshot(_run_pods(0, 410), pods_per_claim=130)
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    assert sorted(len(c["pods"]) for c in want["newNodeClaims"]) == [20, 130, 130, 130] and not want["podErrors"]
    st = got.stats
    print("runs %d runPods %d runRecs %d" % (st["runs"], st["runPods"], st["runRecs"]))
    assert _lean(got)
    assert (st["runs"], st["runPods"]) == (4, 3 * 128 + 18)
    assert st["ncommits"] == 410
    assert st["runRecs"] == (3 if _records_built() else 0)


def test_replicas_expand_their_own_records():
    snap = _snapshot(_run_pods(0, 300), pods_per_claim=130)
    want, got = _solve_both(snap, replicas=3)
    _assert_parity(want, got)
    assert got.stats["ncommits"] == 300


def test_push_back_before_the_run_leaves_no_record():
    """A pod no instance type fits is popped first (the most cpu) and pushed back: the queue is no longer
    NewQueue's order, runs end at the window and are logged from it."""
    snap = _snapshot([synth.pod(0, cpu="1000", mem="1Gi")] + _run_pods(1, 202))
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    assert len(want["podErrors"]) == 1 and len(want["newNodeClaims"]) == 1
    st = got.stats
    print("runs %d runPods %d runRecs %d" % (st["runs"], st["runPods"], st["runRecs"]))
    assert _lean(got)
    assert st["runs"] > 1, "the runs must be cut at the window"
    assert st["ncommits"] == 202
    assert st["runRecs"] == 0


def test_push_back_after_the_run_reuses_its_queue_slots():
    """Four pods that fail are popped last (the least cpu; no instance type has their memory) and pushed back into
    ring slots 0-3 of the queue: slots 2 and 3 held the run's first pods.  The record's pods are NewQueue's, read
    from that order and not from the ring."""
    snap = _snapshot(_run_pods(0, 202) + [synth.pod(900 + k, cpu="50m", mem="4000Gi") for k in range(4)])
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    assert len(want["podErrors"]) == 4 and len(want["newNodeClaims"]) == 1
    st = got.stats
    print("runs %d runPods %d runRecs %d" % (st["runs"], st["runPods"], st["runRecs"]))
    assert _lean(got)
    assert (st["runs"], st["runPods"]) == (1, 200)
    assert st["ncommits"] == 202
    assert st["runRecs"] == (1 if _records_built() else 0)
