"""LEAN Solve: a run of identical pods stays on its NodeClaim across the re-sorts inside one step
(KS_RUN_CROSS).  Every case is bit-exact parity of the canonical Results with the oracle, on
shapes whose NodeClaim counts reach each path of the re-sort; the counters show the continuation ran
(runCross), was refused where an earlier position passed the quick test (runCrossStops), and that a step
is spent only where the placement sequence needs one (test_steps_follow_the_placement_stretches)."""
import json

import pytest

import problems
from karpenter_amd import Scheduler, synth
from oracle import bridge

pytestmark = pytest.mark.gpu


def _solve_both(snap):
    s = json.dumps(snap)
    want, _ = bridge.solve(s)
    got = Scheduler(s).solve()
    return problems.canonical(want), got


def _assert_parity(want, got):
    g = got.canonical()
    for key in ("newNodeClaims", "existingNodes", "podErrors"):
        if want[key] != g[key] and isinstance(want[key], list):
            for i, (a, b) in enumerate(zip(want[key], g[key])):
                assert a == b, "%s[%d]: want %s\n got %s" % (key, i, json.dumps(a)[:1500], json.dumps(b)[:1500])
        assert want[key] == g[key], key
    assert want == g


# (pods, instance types, seed) -> NodeClaims, and the re-sort path the count reaches:
#   11: n <= 12, insertionSort frame only;  46: 12 < n < 50, a descent sends pis_wave straight to the exact pdqsort;
#   64: n >= 50, wave-parallel partialInsertionSort, the exact path when choosePivot's samples straddle the descent;
#   56 and 151: the same with heavily tied counts
SHAPES = [(700, 60, 42, 11), (3000, 60, 7, 46), (1500, 20, 5, 64), (600, 8, 3, 56), (2000, 10, 8, 151)]


@pytest.mark.parametrize("pods,its,seed,claims", SHAPES)
def test_runs_cross_re_sorts(pods, its, seed, claims):
    want, got = _solve_both(synth.benchmark_snapshot(pods, its, seed, diverse=False))
    _assert_parity(want, got)
    assert len(want["newNodeClaims"]) == claims, "the shape no longer reaches the re-sort path it was chosen for"
    st = got.stats
    print("runCross %d runCrossStops %d runCrossLost %d steps %d" % (
        st["runCross"], st["runCrossStops"], st["runCrossLost"], st["pops"] - st["runPods"]))
    assert st["runCross"] > 0
    assert st["runCrossStops"] > 0


def test_cross_inside_the_window_after_push_backs():
    """Three pods too large for every instance type are pushed back: from the first on, runs are bounded by
    the 64-pod window, and the continuation runs inside it."""
    snap = synth.benchmark_snapshot(3000, 60, 7, diverse=False)
    for k in range(3):
        snap["pods"].insert(700 * (k + 1), synth.pod(900000 + k, cpu="1000", mem="1Gi"))
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    assert want["podErrors"], "the case must push pods back"


def test_cross_under_a_nodepool_limit():
    snap = synth.benchmark_snapshot(3000, 60, 7, diverse=False)
    snap["nodePools"] = [synth.node_pool("default-pool", limits={"cpu": "1500"})]
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    assert want["podErrors"], "the case must push pods back"


def test_cross_then_lean_exit_rerun():
    """Pods sharing the UID "" (the literal benchmark pods): the LEAN Solve leaves at the first push-back
    (KE_LEAN_EXIT) and the Solve is re-run non-LEAN; what the LEAN kernel did before that is discarded."""
    snap = synth.benchmark_snapshot(600, 60, 441, diverse=False, literal=True)
    big = synth.pod(900000, cpu="1000", mem="1Gi")
    big["metadata"].pop("uid", None)
    snap["pods"].insert(100, big)
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    assert want["podErrors"], "the case must push the pod back"


_SUFFIX = (("m", 1), ("Ki", 1000 << 10), ("Mi", 1000 << 20), ("Gi", 1000 << 30))


def _milli(q):
    for suf, mul in _SUFFIX:
        if q.endswith(suf):
            return int(q[:-len(suf)]) * mul
    return int(q) * 1000


def _placement_stretches(snap, res):
    """(stretches, stretches of more than one pod that open a NodeClaim) of a Solve without push-backs.
    The placement sequence is NewQueue's order -- cpu, then memory, descending, then the UID, which synth
    numbers by pod index (queue.go:83-112) -- and a stretch is a maximal part of it with one pod class
    (requests) on one NodeClaim."""
    def cls(i):
        r = snap["pods"][i]["spec"]["containers"][0]["resources"]["requests"]
        return (-_milli(r["cpu"]), -_milli(r["memory"]))
    claim, opener = {}, set()
    for ci, c in enumerate(res["newNodeClaims"]):
        opener.add(c["pods"][0])
        for p in c["pods"]:
            claim[p] = ci
    seq = sorted(range(len(snap["pods"])), key=lambda i: cls(i) + (i,))
    n = opening = 0
    i = 0
    while i < len(seq):
        j = i
        while j + 1 < len(seq) and cls(seq[j + 1]) == cls(seq[i]) and claim[seq[j + 1]] == claim[seq[i]]:
            j += 1
        n += 1
        opening += j > i and seq[i] in opener
        i = j + 1
    return n, opening


def test_steps_follow_the_placement_stretches():
    """C2's shape at 10000 pods (23 NodeClaims): the kernel's main-loop steps (pops - runPods) are the maximal
    same-class same-NodeClaim stretches of the placement sequence, derived here from the Results (157 on the
    oracle), plus what the kernel spends by construction: a NodeClaim's first pod is placed by the template
    phase, which starts no run, so a stretch that opens a NodeClaim and goes on takes a second step (23); and a
    refused continuation after which the pod lands on the run's claim all the same (runCrossLost, a subset of
    runCrossStops: any other refusal ends the stretch anyway)."""
    snap = synth.config2(10000)
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    assert not want["podErrors"]
    stretches, opening = _placement_stretches(snap, want)
    st = got.stats
    print("stretches %d opening %d steps %d runCross %d runCrossStops %d runCrossLost %d" % (
        stretches, opening, st["pops"] - st["runPods"], st["runCross"], st["runCrossStops"], st["runCrossLost"]))
    assert st["runCrossLost"] <= st["runCrossStops"]
    assert st["pops"] - st["runPods"] == stretches + opening + st["runCrossLost"]
