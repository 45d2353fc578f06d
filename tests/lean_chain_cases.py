"""Problems of the LEAN Solve's single-pod-step tests (test_lean_chain_gpu.py) and of the counters recorded for them
with the build before KS_CAP_BOUND and KS_THR_BATCH existed (tests/golden/lean_chain_counters.json, written by
scripts/record_lean_chain_counters.py)."""
import json

import queue_cases as qc
from karpenter_amd import queue_inputs, synth

TAINT = {"key": "dedicated", "value": "batch", "effect": "NoSchedule"}
TOLERATE = [{"key": "dedicated", "operator": "Equal", "value": "batch", "effect": "NoSchedule"}]


def two_templates():
    """test_lean_step_gpu.test_memo_key_holds_the_template's construction: every other pod tolerates the first
    template's taint, so no two neighbours of the queue are identical."""
    snap = synth.benchmark_snapshot(600, 8, 3, diverse=False)
    snap["instanceTypes"] = synth.fake_instance_types(14)
    snap["nodeClaimTemplates"] = [synth.node_pool("tainted-pool", taints=[TAINT]), synth.node_pool("open-pool")]
    snap["instanceTypesByNodePool"] = {"tainted-pool": list(range(8)), "open-pool": list(range(4, 14))}
    for i, p in enumerate(snap["pods"]):
        if i % 2 == 0:
            p["spec"]["tolerations"] = TOLERATE
    return snap


def two_templates_alternating():
    """The same two templates with the toleration on every other pod of the queue (NewQueue's order, which does not
    depend on tolerations): no two neighbours of the queue are identical, so every pod is a run of its own."""
    snap = two_templates()
    for p in snap["pods"]:
        p["spec"].pop("tolerations", None)
    order = qc.expected_order(queue_inputs(json.dumps(snap)))
    for rank, i in enumerate(order):
        if rank % 2 == 0:
            snap["pods"][i]["spec"]["tolerations"] = TOLERATE
    return snap


def identical_runs(snap):
    """The number of maximal runs of identical pods in NewQueue's order (the claim runs' identity: requests, first
    state words 0..3, the provisionable bit), from the host's encoding of the snapshot alone."""
    inp = queue_inputs(json.dumps(snap))
    order = qc.expected_order(inp)
    rl = qc.run_lengths(order, inp, True)
    return sum(1 for i in range(len(order)) if i == 0 or rl[i - 1] == 1)


def push_backs():
    """test_lean_step_gpu.test_re_sorts_inside_the_window_after_push_backs's construction: three pods too large for
    every instance type are pushed back, and runs are bounded by the 64-pod window from then on."""
    snap = synth.benchmark_snapshot(3000, 60, 7, diverse=False)
    for k in range(3):
        snap["pods"].insert(700 * (k + 1), synth.pod(900000 + k, cpu="1000", mem="1Gi"))
    return snap


def existing_nodes(n):
    """n existing nodes with room for two of the largest pods each (4 cpu, 8Gi, 2 pods): the queue's first pods fill
    them in first-fit order -- the register window's blocks (64 nodes each) and, at 65, the first node past a block
    edge -- and every later pod goes to NodeClaims."""
    snap = synth.benchmark_snapshot(900, 20, 5, diverse=False)
    for i in range(n):
        name = "node-%03d" % i
        snap["stateNodes"].append({
            "name": name, "hostName": name,
            "labels": {synth.ZONE: "test-zone-1", synth.ARCH: "amd64", synth.NODEPOOL: "default-pool",
                       synth.HOSTNAME: name, synth.CT: "on-demand"},
            "taints": [], "available": {"cpu": "4", "memory": "8Gi", "pods": "2"},
            "capacity": {"cpu": "4", "memory": "8Gi", "pods": "110"}, "daemonSetRequests": {}, "initialized": True})
    return snap


# name -> (builder, NodeClaims); the counts are the oracle's
RESORT = {
    "cross_11": (lambda: synth.benchmark_snapshot(700, 60, 42, diverse=False), 11),
    "cross_46": (lambda: synth.benchmark_snapshot(3000, 60, 7, diverse=False), 46),
    "chain_64": (lambda: synth.benchmark_snapshot(1500, 20, 5, diverse=False), 64),
    "cross_56": (lambda: synth.benchmark_snapshot(600, 8, 3, diverse=False), 56),
    "cross_151": (lambda: synth.benchmark_snapshot(2000, 10, 8, diverse=False), 151),
    "c2_10000": (lambda: synth.config2(10000), 23),
}
NODES = {"nodes_%d" % n: (lambda n=n: existing_nodes(n), None) for n in (3, 64, 65)}
# instance types -> case: the threshold tables of 8, 60, 200 and 400 options (1, 1, 4 and 7 chunks of 64 per resource)
THRESHOLDS = {8: "cross_56", 60: "cross_46", 200: "its_200", 400: "c2_10000"}
CASES = dict(RESORT)
CASES.update(NODES)
CASES.update({
    "two_templates": (two_templates, None),
    "two_templates_alt": (two_templates_alternating, None),
    "push_backs": (push_backs, None),
    "its_200": (lambda: synth.benchmark_snapshot(1500, 200, 5, diverse=False), None),
})
