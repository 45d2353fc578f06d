"""CPU preconditions of tests/test_tpl_table_gpu.py: on the oracle and the snapshot alone, every case of
tests/tpl_table_cases.py is in the cell its name says -- the NodeClaim and error counts, the route's inputs (live
resources, lean), which opens alternate in request class, that a limited pool or an unfit template is really met --
and the host side of the table (request classes, the cap) is what ks_problem_inspect reports."""
import collections
import json

import pytest

import tpl_table_cases as tc
from karpenter_amd import inspect, synth


def _openers(want):
    """The opening pod of every NodeClaim in creation order (the hostname placeholders count NewNodeClaim calls)."""
    claims = sorted(want["newNodeClaims"], key=lambda c: c["hostname"])
    return [c["pods"][0] for c in claims]


@pytest.mark.parametrize("name", tc.NAMES)
def test_case_is_in_its_cell(name):
    exp = tc.CASES[name][1]
    snap = json.loads(tc.snapshot_json(name))
    want = tc.oracle(name)
    doc = inspect(snap)
    assert doc["R"] == exp["R"] and doc["lean"] == 1
    full = doc["plans"][str(160 * 1024 - 256)]
    assert (full["talloc"] == 1 and doc["R"] in (3, 4)) == exp["lean"]
    assert len(want["podErrors"]) == exp["errors"]
    if "claims" in exp:
        assert len(want["newNodeClaims"]) == exp["claims"]
    pools = collections.Counter(c["nodePoolName"] for c in want["newNodeClaims"])
    if "pools" in exp:
        assert dict(pools) == exp["pools"]
    classes = {tc.request_class(p) for p in snap["pods"]}
    assert doc["tplClasses"] == len(classes)
    if doc["tplTableBuild"]:
        assert doc["tplTable"] == (1 if exp["lean"] else 0)
    if exp.get("alternate"):
        opens = [tc.request_class(snap["pods"][p]) for p in _openers(want)]
        assert len(opens) >= 4 and all(a != b for a, b in zip(opens, opens[1:]))
    if exp.get("limited"):
        # the limited template is first, takes some NodeClaims and then refuses: later ones open on the next templates
        assert snap["nodeClaimTemplates"][0]["metadata"]["name"] == "limited-pool" and snap["nodePools"]
        assert 0 < pools["limited-pool"] < len(want["newNodeClaims"])
        order = [c["nodePoolName"] for c in sorted(want["newNodeClaims"], key=lambda c: c["hostname"])]
        assert order.index("open-pool") > order.index("limited-pool")


def test_unfit_template_is_met():
    """no_fit: the pods asking for the extended resource find no instance type in the first template (its small types
    carry none) and open on the second; the two unfit pods fail both, with both templates' failure flags printed."""
    snap = json.loads(tc.snapshot_json("no_fit"))
    want = tc.oracle("no_fit")
    for c in want["newNodeClaims"]:
        vendor = tc.VENDOR in dict(tc.request_class(snap["pods"][c["pods"][0]]))
        assert c["nodePoolName"] == ("open-pool" if vendor else "small-pool")
    for msg in want["podErrors"].values():
        assert "small-pool" in msg and "open-pool" in msg and "no instance type" in msg


def test_taint_is_met():
    snap = json.loads(tc.snapshot_json("taint"))
    assert snap["nodeClaimTemplates"][0]["spec"]["template"]["spec"]["taints"]
    assert all("tolerations" not in p["spec"] for p in snap["pods"])
    assert {c["nodePoolName"] for c in tc.oracle("taint")["newNodeClaims"]} == {"open-pool"}


def test_daemon_overhead_is_counted():
    """req != pod: every NodeClaim's requests hold the daemon's 500m on top of its pod's 5 cpu."""
    for c in tc.oracle("daemon")["newNodeClaims"]:
        assert c["requests"]["cpu"] == "5500m"


def test_front_member_has_no_offering():
    snap = json.loads(tc.snapshot_json("front_no_offering"))
    doc = inspect(snap)
    assert doc["paretoFronts"] == [[19]]
    for c in tc.oracle("front_no_offering")["newNodeClaims"]:
        assert "fake-it-19" not in c["instanceTypeOptions"] and len(c["pods"]) > 1


def test_non_inline_shape():
    """At the reduced budget the plan keeps fewer claims in LDS than it has positions, and the case opens more than
    it keeps (one NodeClaim per big pod, replan_cases.lean_base)."""
    from oracle import bridge

    plan = inspect(tc.non_inline_shape())["plans"][str(tc.NONINLINE_BUDGET)]
    assert plan["talloc"] == 1 and plan["KL"] + 2 <= plan["KO"]
    snap = tc.non_inline(plan)
    assert inspect(snap)["plans"][str(tc.NONINLINE_BUDGET)] == plan
    n = len(bridge.solve(json.dumps(snap))[0]["newNodeClaims"])
    assert plan["KL"] < n <= plan["KO"]


def test_cap():
    """all_distinct: 40 classes; the default cap holds their table, and one record is more than 64 bytes."""
    doc = inspect(json.loads(tc.snapshot_json("all_distinct")))
    assert doc["tplClasses"] == 40
    assert 64 < doc["tplTableBytes"] // 40 and doc["tplTableBytes"] == 40 * 4 * (doc["TW"] + 6 * doc["R"] + 4)
    if doc["tplTableBuild"]:
        assert doc["tplTable"] == 1
    assert len(tc.oracle("all_distinct")["newNodeClaims"]) > 1


def test_c2_has_thirty_classes():
    """The benchmark's shape (synth.benchmark_snapshot without labels' effect): 5 cpu x 6 memory choices."""
    assert inspect(synth.benchmark_snapshot(3000, 60, 7, diverse=False))["tplClasses"] == 30
