"""LEAN Solve: the three shortcuts inside one main-loop step -- the closed-form claim re-sort at a
single count crossing (KS_SORT_CLOSED, sortsClosed), the memo of the last NewNodeClaim (KS_TPL_MEMO,
tplMemoHits) and the log of a run past the queue window at every chunk edge (the path KS_LOG_AHEAD reorders).
Every case is bit-exact parity of the canonical Results with the oracle; the counters show which path ran."""
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


def _lean(got):
    r = got.stats["route"]
    return r["family"] == "solve" and r["lean"] == 1


# --- the re-sort -------------------------------------------------------------------------------------

# (pods, instance types, seed) -> NodeClaims.  64: n >= 50; 56 and 151: the same with heavily tied counts, the
# tie blocks of 151 claims reaching across the 64-lane chunks; 46: 12 < n < 50 never takes the closed form
CLOSED = [(1500, 20, 5, 64), (600, 8, 3, 56), (2000, 10, 8, 151)]


@pytest.mark.parametrize("pods,its,seed,claims", CLOSED)
def test_closed_form_and_exact_re_sorts(pods, its, seed, claims):
    want, got = _solve_both(synth.benchmark_snapshot(pods, its, seed, diverse=False))
    _assert_parity(want, got)
    assert len(want["newNodeClaims"]) == claims, "the shape no longer reaches the re-sort path it was chosen for"
    st = got.stats
    print("sorts %d withDescent %d exact %d closed %d tplMemoHits %d" % (
        st["sorts"], st["sortsWithDescent"], st["sortsExact"], st["sortsClosed"], st["tplMemoHits"]))
    assert _lean(got)
    assert st["sortsClosed"] > 0
    assert st["sortsExact"] > 0
    assert st["tplMemoHits"] > 0


def test_below_fifty_claims_never_takes_the_closed_form():
    want, got = _solve_both(synth.benchmark_snapshot(3000, 60, 7, diverse=False))
    _assert_parity(want, got)
    assert len(want["newNodeClaims"]) == 46
    st = got.stats
    print("sorts %d withDescent %d exact %d closed %d tplMemoHits %d" % (
        st["sorts"], st["sortsWithDescent"], st["sortsExact"], st["sortsClosed"], st["tplMemoHits"]))
    assert _lean(got)
    assert st["sortsWithDescent"] > 0
    assert st["sortsClosed"] == 0
    assert st["tplMemoHits"] > 0


def test_re_sorts_inside_the_window_after_push_backs():
    """Three pods too large for every instance type are pushed back: runs are bounded by the 64-pod window
    from then on, and descents come from claims appended behind greater counts as well."""
    snap = synth.benchmark_snapshot(3000, 60, 7, diverse=False)
    for k in range(3):
        snap["pods"].insert(700 * (k + 1), synth.pod(900000 + k, cpu="1000", mem="1Gi"))
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    assert want["podErrors"], "the case must push pods back"


# --- the memo of the last NewNodeClaim ---------------------------------------------------------------

def test_memo_bypassed_under_a_nodepool_limit():
    snap = synth.benchmark_snapshot(3000, 60, 7, diverse=False)
    snap["nodePools"] = [synth.node_pool("default-pool", limits={"cpu": "1500"})]
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    assert want["podErrors"], "the case must push pods back"
    assert _lean(got)
    assert got.stats["tplMemoHits"] == 0


TAINT = {"key": "dedicated", "value": "batch", "effect": "NoSchedule"}
TOLERATE = [{"key": "dedicated", "operator": "Equal", "value": "batch", "effect": "NoSchedule"}]


def test_memo_key_holds_the_template():
    """Two templates over different instance types, the first tainted: every other pod tolerates it and opens
    its NodeClaims there, the rest skip it and open theirs on the second -- the same requests alternate
    between the two templates, so a memo keyed without the template would hand one's options to the other."""
    snap = synth.benchmark_snapshot(600, 8, 3, diverse=False)
    snap["instanceTypes"] = synth.fake_instance_types(14)
    snap["nodeClaimTemplates"] = [synth.node_pool("tainted-pool", taints=[TAINT]), synth.node_pool("open-pool")]
    snap["instanceTypesByNodePool"] = {"tainted-pool": list(range(8)), "open-pool": list(range(4, 14))}
    for i, p in enumerate(snap["pods"]):
        if i % 2 == 0:
            p["spec"]["tolerations"] = TOLERATE
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    pools = {c["nodePoolName"] for c in want["newNodeClaims"]}
    print("claims %d pools %s tplMemoHits %d" % (len(want["newNodeClaims"]), pools, got.stats["tplMemoHits"]))
    assert len(pools) == 2, "both templates must open NodeClaims"
    assert _lean(got)
    assert got.stats["tplMemoHits"] > 0


def test_memo_across_relaxed_states():
    """The template carries a PreferNoSchedule taint.  Every other pod tolerates it from the start; the rest
    fail, are pushed back and relaxed (Preferences.Relax adds the toleration), and arrive again in their second
    state with the requests the tolerating pods opened NodeClaims with.  (Every pod has states of its own, so
    the memo's key cannot hold the state; a LEAN problem's states differ in nothing a fresh NodeClaim's options
    depend on, which is what this case and the failed first attempts -- the taint test runs on a hit too -- pin.)"""
    snap = synth.benchmark_snapshot(600, 8, 3, diverse=False)
    prefer = {"key": "spotty", "value": "", "effect": "PreferNoSchedule"}
    snap["nodeClaimTemplates"] = [synth.node_pool("default-pool", taints=[prefer])]
    # (a NodePool no template uses: its taint switches the relaxation on, and the template stays without limits)
    snap["nodePools"] = [synth.node_pool("other-pool", taints=[prefer])]
    for i, p in enumerate(snap["pods"]):
        if i % 2 == 0:
            p["spec"]["tolerations"] = [{"key": "spotty", "operator": "Exists", "effect": "PreferNoSchedule"}]
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    assert not want["podErrors"]
    st = got.stats
    print("claims %d pops %d tplMemoHits %d" % (len(want["newNodeClaims"]), st["pops"], st["tplMemoHits"]))
    assert st["pops"] > 600, "the non-tolerating pods must be pushed back and popped again"
    assert _lean(got)
    assert st["tplMemoHits"] > 0


# --- the run log -------------------------------------------------------------------------------------

RUN_LENGTHS = [63, 64, 65, 127, 128, 129, 255, 256, 257, 300]
# pods of a larger class placed first: the run's first log entry lands at 2 + prefix (the class's first pod is
# placed by the template phase or an ordinary claim commit, the second by the commit that starts the run), so
# the run starts mid-block for 0 and 5 and on a 64-entry block boundary for 62
PREFIXES = [0, 5, 62]


def _run_snapshot(length, prefix):
    """One instance type that holds everything; `prefix` pods of 2 cpu, then the class whose single run has
    `length` pods: with no prefix its first pod opens the NodeClaim and its second starts the run (length + 2
    pods); behind a prefix its first pod lands on the open NodeClaim and starts the run (length + 1)."""
    snap = synth.benchmark_snapshot(0, 1, 1, diverse=False)
    snap["instanceTypes"] = [synth.fake_instance_type("fake-it-big", 256, 512, pods=1000)]
    n = length + (1 if prefix else 2)
    snap["pods"] = [synth.pod(i, cpu="2", mem="1Gi") for i in range(prefix)] + \
                   [synth.pod(prefix + i, cpu="100m", mem="100Mi") for i in range(n)]
    return snap


@pytest.mark.parametrize("prefix", PREFIXES)
def test_run_log_past_the_window(prefix):
    for length in RUN_LENGTHS:
        snap = _run_snapshot(length, prefix)
        want, got = _solve_both(snap)
        _assert_parity(want, got)
        assert len(want["newNodeClaims"]) == 1 and not want["podErrors"]
        st = got.stats
        assert _lean(got)
        # the prefix class: template phase, then one commit and a run of prefix - 2 inside the window
        pre_runs, pre_pods = (1, prefix - 2) if prefix > 2 else (0, 0)
        assert (st["runs"], st["runPods"]) == (pre_runs + 1, pre_pods + length), (length, prefix, st["runs"], st["runPods"])
        assert st["ncommits"] == len(snap["pods"])
