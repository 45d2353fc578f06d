"""LEAN Solve: the cheap single-pod steps -- the chained pop that skips the node phase behind an identical
pod a NodeClaim took (KS_RUN_CHAIN, chainPods), the capacity bound that spares a run's claim_run_cap call
(KS_CAP_BOUND, capBoundSkips) and claim_full's threshold advance with the first chunk of every resource issued
together (KS_THR_BATCH, thrBatchCalls, thrMultiChunk).

Every case is bit-exact parity of the canonical Results with the oracle.  A bound that skipped a call it should have
made would leave the Results intact and only split a run into single steps, a batched advance that dropped other
options would change algBytes before it changed a placement, and a chained pod is credited the node phase's bytes of
the pod before it, so every case also holds the kernel to the counters the build before the switches recorded for the
same problem (tests/golden/lean_chain_counters.json): algBytes, runs, claimFull, and the claim_run_cap calls, which
the calls still made and the calls skipped must add up to.

Which blocks a library holds is its build's (ks_problem_inspect's "runChain", "capBound", "thrBatch").  THE SHIPPED
BUILD HAS THE BOUND ONLY: on it this file checks the bound, parity and the recorded counters, and that
chainPods, thrBatchCalls and thrMultiChunk are 0.  The assertions about the chain (chainPods == pops - runPods - R,
chainPods == 0 where no two neighbours are identical, chainPods > 0 after push-backs) and about the batch
(thrBatchCalls > 0, thrMultiChunk > 0 at 400 instance types) run only against a library built with -DKS_RUN_CHAIN=1 /
-DKS_THR_BATCH=1: scripts/variant_check.sh "tests/test_lean_chain_gpu.py tests/test_lean_step_gpu.py" <variant>, which
is how they were run for DESIGN §7, as was the build with every switch at 0."""
import json
import os

import pytest

import lean_chain_cases as cases
import problems
from karpenter_amd import Scheduler
from karpenter_amd.scheduler import inspect
from oracle import bridge
from test_lean_step_gpu import _assert_parity

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lean_chain_counters.json")) as _f:
    GOLDEN = json.load(_f)["cases"]
_SOLVED = {}


def _solve(name):
    """(snapshot, oracle Results, GPU Results, build switches) of a case, solved once per session."""
    if name not in _SOLVED:
        snap = cases.CASES[name][0]()
        s = json.dumps(snap)
        want, _ = bridge.solve(s)
        build = inspect(snap)
        _SOLVED[name] = (snap, problems.canonical(want), Scheduler(s).solve(), build)
    return _SOLVED[name]


def _check(name):
    snap, want, got, build = _solve(name)
    _assert_parity(want, got)
    st, gold = got.stats, GOLDEN[name]
    r = st["route"]
    assert r["family"] == "solve" and r["lean"] == 1
    claims = cases.CASES[name][1]
    if claims is not None:
        assert len(want["newNodeClaims"]) == claims, "the shape no longer reaches the re-sort path it was chosen for"
    print("%s: claims %d steps %d runs %d chainPods %d runCapFront %d runCapFull %d capBoundSkips %d thrBatchCalls %d "
          "thrMultiChunk %d claimFull %d (runChain %d capBound %d thrBatch %d)" % (
              name, st["nclaims"], st["pops"] - st["runPods"], st["runs"], st["chainPods"], st["runCapFront"],
              st["runCapFull"], st["capBoundSkips"], st["thrBatchCalls"], st["thrMultiChunk"], st["claimFull"],
              build["runChain"], build["capBound"], build["thrBatch"]))
    for key in ("algBytes", "runs", "claimFull", "nclaims"):
        assert st[key] == gold[key], "%s: %s is %d, recorded %d" % (name, key, st[key], gold[key])
    assert st["runCapFront"] + st["runCapFull"] + st["capBoundSkips"] == gold["runCapCalls"]
    # a run that placed pods asked for its capacity: only calls that would have returned 0 can be skipped
    assert st["runCapFront"] + st["runCapFull"] >= st["runs"]
    if not build["capBound"]:
        assert st["capBoundSkips"] == 0
    # at most one batched advance per claim_full call -- `claimFull` counts the scan's calls, and each run adds one for
    # its k pods at once -- and only some of those drop more than a chunk
    assert st["thrMultiChunk"] <= st["thrBatchCalls"] <= st["claimFull"] + st["runs"]
    if not build["thrBatch"]:
        assert st["thrBatchCalls"] == 0 and st["thrMultiChunk"] == 0
    # a chained pod is a popped pod that is not the first of its identical-pod run
    assert 0 <= st["chainPods"] <= st["pops"] - st["runPods"]
    if not build["runChain"]:
        assert st["chainPods"] == 0
    return want, st, build


def _chain_everywhere(name, want, st, build):
    """Without existing nodes and push-backs every pod lands on a NodeClaim and the queue stays NewQueue's order: a
    main-loop step is chained unless its pod starts one of the R maximal identical-pod runs of that order."""
    assert not want["podErrors"] and not any(e["pods"] for e in want["existingNodes"])
    runs = cases.identical_runs(_solve(name)[0])
    if build["runChain"]:
        assert st["chainPods"] == st["pops"] - st["runPods"] - runs, (st["chainPods"], st["pops"], st["runPods"], runs)
    return runs


@pytest.mark.parametrize("name", sorted(cases.RESORT))
def test_re_sort_routes(name):
    """11, 46, 64, 56 and 151 NodeClaims (every route of the claim re-sort, heavy ties, more than two quick-scan
    chunks) and C2 at 10 000 pods."""
    want, st, build = _check(name)
    runs = _chain_everywhere(name, want, st, build)
    if name == "c2_10000":
        assert runs == 30 and st["pops"] - st["runPods"] == 180  # (chained: 150 of the 180 steps)
        if build["capBound"]:
            assert st["capBoundSkips"] > 0  # single-pod top-ups of a nearly full NodeClaim


def test_two_templates_by_pod_index():
    """test_memo_key_holds_the_template's construction, every other pod BY INDEX tolerating the first template's
    taint.  NewQueue's order is by requests, so 320 of the 600 pods start an identical-pod run and the other 280
    follow a pod identical to them (the oracle's order; the claim runs place 100-odd of them): the chain takes exactly
    those that are popped.  The claims of both templates stand mixed in the sorted array, and a headroom read for the
    wrong position would skip (or make) other calls than the recorded ones."""
    want, st, build = _check("two_templates")
    assert len({c["nodePoolName"] for c in want["newNodeClaims"]}) == 2, "both templates must open NodeClaims"
    assert _chain_everywhere("two_templates", want, st, build) == 320


def test_identity_boundary_no_two_neighbours_identical():
    """The same two templates with the toleration on every other pod of the queue: no two neighbours are identical
    (600 runs of one pod), so nothing is chained and no run is placed."""
    want, st, build = _check("two_templates_alt")
    assert len({c["nodePoolName"] for c in want["newNodeClaims"]}) == 2, "both templates must open NodeClaims"
    assert _chain_everywhere("two_templates_alt", want, st, build) == 600
    assert st["chainPods"] == 0
    assert st["runs"] == 0 and st["runPods"] == 0


def test_after_push_backs():
    """Three oversized pods are pushed back: from then on the identity is the window's (same template tolerations,
    tolerations and requests, not stale) and a chain ends with the window."""
    want, st, build = _check("push_backs")
    assert want["podErrors"], "the case must push pods back"
    assert st["runs"] > 0
    if build["runChain"]:
        assert st["chainPods"] > 0


@pytest.mark.parametrize("n", [3, 64, 65])
def test_existing_nodes_then_claims(n):
    """The first pods fill the existing nodes: a pod behind one that landed on a node scans the nodes itself, so fewer
    steps are chained than identical neighbours would allow, and algBytes holds the credited node phases to the
    recorded value."""
    name = "nodes_%d" % n
    want, st, build = _check(name)
    filled = [e for e in want["existingNodes"] if e["pods"]]
    assert len(filled) == n and all(len(e["pods"]) == 2 for e in filled), "the first pods must fill every existing node"
    assert want["newNodeClaims"] and not want["podErrors"]
    if build["runChain"]:
        assert 0 < st["chainPods"] < st["pops"] - st["runPods"] - cases.identical_runs(_solve(name)[0])


@pytest.mark.parametrize("its", sorted(cases.THRESHOLDS))
def test_batched_thresholds(its):
    """Threshold tables of 8, 60, 200 and 400 options.  On a build without the batch (the shipped one) this is the
    parity and counter check of _check alone; the batch's own assertions need the -DKS_THR_BATCH=1 variant."""
    snap, _, _, _ = _solve(cases.THRESHOLDS[its])
    assert len(snap["instanceTypes"]) == its
    _, st, build = _check(cases.THRESHOLDS[its])
    if build["thrBatch"]:
        assert st["thrBatchCalls"] > 0
        if its == 400:
            assert st["thrMultiChunk"] > 0  # a run's bulk commit drops more than 64 of the 400 options at once
