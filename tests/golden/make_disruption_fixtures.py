#!/usr/bin/env python3
"""Known-answer Drift and Expiration scenarios hand-transcribed from the reference's Go tests.

Source: pkg/controllers/disruption/drift_test.go and expiration_test.go, with the suite setup of
suite_test.go:95-130 (fake.InstanceTypesAssorted(), the most expensive on-demand type for the nodes) and the
tests' NodePool (consolidateAfter Never; expireAfter Never for Drift, 30s for Expiration).  A NodeClaim's
condition is a snapshot stateNode's "nodeClaimConditions" entry; the Drift feature gate is the snapshot's
"featureGates".

Each scenario is {"name", "method", "source", "snapshot", "expect"}; `expect` holds the Go test's assertion on the
command the disruption controller executes:
  action       : "delete" | "replace" | "no-op"
  candidates   : node names the command removes (in the method's order)
  replacements : NodeClaims the command launches

disruption_scenarios.json keeps the expectations (data only); the tests rebuild the snapshots from this script.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_consolidation_fixtures as mcf  # noqa: E402
from make_consolidation_fixtures import synth  # noqa: E402

NOW = synth.NOW
KIND = {"drift": "Drifted", "expiration": "Expired"}
SRC = {"drift": "pkg/controllers/disruption/drift_test.go", "expiration": "pkg/controllers/disruption/expiration_test.go"}
# the lines of each case in drift_test.go / expiration_test.go (expiration_test.go has no feature-gate case)
LINES = {
    "feature-flag-off": {"drift": 76},
    "continue-to-next": {"drift": 94, "expiration": 145},
    "no-condition": {"drift": 155, "expiration": 75},
    "do-not-disrupt-node": {"drift": 170, "expiration": 89},
    "do-not-evict-pod": {"drift": 184, "expiration": 103},
    "do-not-disrupt-pod": {"drift": 205, "expiration": 124},
    "status-false": {"drift": 226, "expiration": 206},
    "can-delete": {"drift": 241, "expiration": 221},
    "all-empty-in-parallel": {"drift": 264, "expiration": 242},
    "can-replace": {"drift": 307, "expiration": 359},
    "replace-with-multiple-nodes": {"drift": 405, "expiration": 454},
    "one-non-empty-at-a-time": {"drift": 502, "expiration": 285},
}


def condition(method, ago=600, status="True"):
    return [{"type": KIND[method], "status": status, "lastTransitionTime": synth._fmt_time(NOW - ago)}]


def plain_pod(i, cpu, node, annotations=None):
    """test.Pod (no owner), bound with ExpectManualBinding."""
    p = synth.pod(i, cpu=cpu)
    if annotations:
        p["metadata"]["annotations"] = annotations
    p["spec"]["nodeName"] = node
    p["status"] = {"phase": "Running", "conditions": [{"type": "PodScheduled", "status": "True"}]}
    return p


def scenarios(method):
    its = mcf.assorted()
    most = mcf.od_sorted(its)[-1]
    disruption = {"consolidateAfter": "Never", "expireAfter": "Never" if method == "drift" else "30s"}
    S = []

    def add(name, nodes, expect, its_=None, gates=None):
        if method not in LINES[name]:
            return
        snap = mcf.snapshot(its_ or its, nodes, disruption=disruption)
        if gates is not None:
            snap["featureGates"] = gates
        S.append({"name": "%s-%s" % (method, name), "method": method, "source": "%s:%d" % (SRC[method], LINES[name][method]),
                  "snapshot": snap, "expect": expect})

    def the_node(name="node-a", cpu="32", pods=(), ago=600, status="True", annotations=None, cond=True, it=most):
        n = mcf.node(name, it, {"cpu": cpu, "pods": "100"}, list(pods), annotations=annotations)
        if cond:
            n["nodeClaimConditions"] = condition(method, ago, status)
        return n

    none = {"action": "no-op", "candidates": [], "replacements": 0}
    add("feature-flag-off", [the_node()], none, gates={"drift": False})
    # the first node's pod (150 cpu) fits no instance type; the second node's is replaced
    add("continue-to-next", [the_node("node-a", pods=[plain_pod(0, "150", "node-a")], ago=1200),
                             the_node("node-b", cpu="1", pods=[plain_pod(1, "1", "node-b")], ago=600)],
        {"action": "replace", "candidates": ["node-b"], "replacements": 1})
    add("no-condition", [the_node(cond=False)], none)
    add("do-not-disrupt-node", [the_node(annotations={"karpenter.sh/do-not-disrupt": "true"})], none)
    add("do-not-evict-pod", [the_node(pods=[plain_pod(0, "1", "node-a", {"karpenter.sh/do-not-evict": "true"})])], none)
    add("do-not-disrupt-pod", [the_node(pods=[plain_pod(0, "1", "node-a", {"karpenter.sh/do-not-disrupt": "true"})])], none)
    add("status-false", [the_node(status="False")], none)
    add("can-delete", [the_node()], {"action": "delete", "candidates": ["node-a"], "replacements": 0})
    many = [the_node("node-%03d" % i, ago=600 + i) for i in range(100)]
    add("all-empty-in-parallel", many,
        {"action": "delete", "candidates": [n["name"] for n in reversed(many)], "replacements": 0})
    add("can-replace", [the_node(pods=[mcf.rs_pod(0, cpu="1", bound_to="node-a")])],
        {"action": "replace", "candidates": ["node-a"], "replacements": 1})
    # three 2-cpu pods, the only available type holds 3 cpu: three replacements
    cur = synth.fake_instance_type("current-on-demand", 4, 4, offerings=[
        {"capacityType": "on-demand", "zone": "test-zone-1a", "price": 0.5, "available": False}])
    rep = synth.fake_instance_type("replacement-on-demand", 3, 4, offerings=[
        {"capacityType": "on-demand", "zone": "test-zone-1a", "price": 0.3, "available": True}])
    add("replace-with-multiple-nodes",
        [the_node(cpu="8", pods=[mcf.rs_pod(i, cpu="2", bound_to="node-a") for i in range(3)], it=cur)],
        {"action": "replace", "candidates": ["node-a"], "replacements": 3}, its_=[cur, rep])
    # two nodes each holding a 30-cpu pod; the one whose condition is an hour old goes first, alone
    add("one-non-empty-at-a-time", [the_node("node-a", pods=[mcf.rs_pod(0, cpu="30", bound_to="node-a")], ago=60),
                                    the_node("node-b", pods=[mcf.rs_pod(1, cpu="30", bound_to="node-b")], ago=3600)],
        {"action": "replace", "candidates": ["node-b"], "replacements": 1})
    return S


def all_scenarios():
    return scenarios("drift") + scenarios("expiration")


def main():
    out = [{"name": s["name"], "method": s["method"], "source": s["source"], "expect": s["expect"]} for s in all_scenarios()]
    with open(os.path.join(HERE, "disruption_scenarios.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("%d scenarios" % len(out))


if __name__ == "__main__":
    main()
