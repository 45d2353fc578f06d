"""Snapshots for the placement tests (KS_CONS_PLACEMENTS, ks_cons_sim_results) and their references, computed once
per process from the oracle (tests/placements_reference.py).

Every cluster is small (at most about 40 nodes and 200 pods per simulation).  Node 0 is the "heavy" node: it drifted
first, so Drift picks it, and it is a consolidation candidate whose single-node simulation the pass runs.
"""
import copy
import functools

import disrupt_cases as dc
import placements_reference as pref
from karpenter_amd import synth

EDGES = (1, 63, 64, 65, 128, 129)  # commits of the heavy node's simulation: around the 64-entry log block


def heavy_first(snap, method="drift", seed=2):
    """Mark every node; the node with the most pods gets the earliest transition time."""
    dc.mark(snap, method, seed=seed)
    nodes = snap["stateNodes"]
    heavy = max(nodes, key=lambda n: len(n["pods"]))
    first = min(nodes, key=lambda n: n["nodeClaimConditions"][1]["lastTransitionTime"])
    heavy["nodeClaimConditions"], first["nodeClaimConditions"] = first["nodeClaimConditions"], heavy["nodeClaimConditions"]
    return snap


def heavy_name(snap):
    return max(snap["stateNodes"], key=lambda n: len(n["pods"]))["name"]


RUN_ROOM = (70, 10)  # identical 100m pods the two other nodes have room for


def edge_case(k, identical):
    """The heavy node holds k pods, no pending pods: its simulation commits exactly k.  One pod of 8 cpu fits no
    existing node and is committed first (so the command is a replace); the two other nodes have room for 70 and 10
    pods of 100m, what is left lands on the NodeClaim.  identical: the other k - 1 pods are 100m each -- a simulation
    places runs of identical pods on existing nodes in one step (a run of 70 on one node, past the 64-pod queue
    window); on a NodeClaim a simulation takes them pod by pod.  Otherwise they have pairwise different cpu (100m,
    101m, ...: no two pods form a run)."""
    def pods_of(j):
        if j:
            return [("250m", None, None)]
        return [("8", None, None)] + [("100m" if identical else "%dm" % (100 + i), None, None) for i in range(k - 1)]
    snap = dc.lean(3, pods_of=pods_of)
    for n, room in zip(snap["stateNodes"][1:], RUN_ROOM):
        n["available"] = {"cpu": "%dm" % (100 * room), "memory": "%dMi" % (64 * room), "pods": str(room)}
    return heavy_first(snap)


def targets_case():
    """The heavy node's pods split between existing nodes and two NodeClaims: the other nodes have room for one
    500m pod each, the two 30-cpu pods need a NodeClaim each (no type of 40 cpu holds both).  One pending pod of
    1000 cpu fits nowhere and stays unscheduled; allNonPendingScheduled stays true."""
    snap = dc.lean(4, pods_of=lambda j: [("30", None, None), ("30", None, None), ("500m", None, None), ("400m", None, None)]
                   if j == 0 else [("250m", None, None)])
    for n in snap["stateNodes"][1:]:
        n["available"] = {"cpu": "600m", "memory": "1Gi", "pods": "1"}
    snap["pendingPods"] = [synth.pod(900, cpu="1000", mem="64Mi")]
    return heavy_first(snap)


def text_case(kind):
    """Requests text that depends on the commit order, on the picked replacement (the queue is by cpu, descending:
    the first pod below is committed first)."""
    ext = None
    if kind == "mi_then_g":
        pods = [("500m", None, {"memory": "512Mi"}), ("400m", None, {"memory": "1G"})]
    elif kind == "g_then_mi":
        pods = [("500m", None, {"memory": "1G"}), ("400m", None, {"memory": "512Mi"})]
    elif kind == "mi_then_k":  # 131072k = 125Mi: the sum prints as 637Mi (BinarySI) or 667942912 (DecimalSI)
        pods = [("500m", None, {"memory": "512Mi"}), ("400m", None, {"memory": "131072k"})]
    elif kind == "k_then_mi":
        pods = [("500m", None, {"memory": "131072k"}), ("400m", None, {"memory": "512Mi"})]
    elif kind == "second_names":  # only the second pod names the resource, and its sum is zero
        ext = {"example.com/a": "64"}
        pods = [("500m", None, None), ("400m", None, {"example.com/a": "0"})]
    elif kind == "zero_first":  # the first pod names memory as 0 (DecimalSI), the second as 512Mi (BinarySI)
        pods = [("500m", None, {"memory": "0"}), ("400m", None, {"memory": "512Mi"})]
    elif kind == "negative":
        pods = [("500m", None, {"memory": "512Mi"}), ("400m", None, {"memory": "-1G"})]
    else:
        raise KeyError(kind)
    return heavy_first(dc.lean(3, pods_of=lambda j: pods if j == 0 else [("100m", None, None)], extra=ext))


TEXT_KINDS = ("mi_then_g", "g_then_mi", "mi_then_k", "k_then_mi", "second_names", "zero_first", "negative")
# the quantity texts the picked NodeClaim's pods write, in commit order, for the resource the case is about
TEXT_MIX = {"mi_then_g": ("memory", ["512Mi", "1G"]), "g_then_mi": ("memory", ["1G", "512Mi"]),
            "mi_then_k": ("memory", ["512Mi", "131072k"]), "k_then_mi": ("memory", ["131072k", "512Mi"]),
            "second_names": ("example.com/a", [None, "0"]), "zero_first": ("memory", ["0", "512Mi"]),
            "negative": ("memory", ["512Mi", "-1G"])}
# the text the Merge gives the resource: Quantity.Add adopts an addend's format while the sum is zero.  512Mi + 1G is
# no multiple of 1024 or 1000, so both formats print it alike: that pair shows only that the refusal is lifted; the
# 131072k pair (125Mi) shows the order in the text.
TEXT_WANT = {"mi_then_g": "1536870912", "g_then_mi": "1536870912", "mi_then_k": "637Mi", "k_then_mi": "667942912",
             "second_names": "0", "zero_first": "512Mi", "negative": "-463129088"}


def lds_case():
    """70 NodeClaims: with a small lds_budget most of them live in the HBM-resident claim state."""
    return dc.claims_case(70)


def mw_cluster():
    """A cluster whose pass KS_SIM_MW=1 KS_SIM_MW_MIN=1 routes to the 4-wave kernels (tests/test_cons_mw_gpu.py)."""
    return synth.cluster_snapshot(40, 4, n_its=60, seed=1, spot_frac=0.3, it_range=(4, 40))


def pass_cluster():
    """A consolidation pass with pending pods and multi-node prefixes."""
    return dc.small(seed=35, n=14, n_pending=2)


BUILDERS = {
    "r5": lambda: dc.resources_case(True),
    "selectors": lambda: filled(dc.selectors_case()),
    "topology": lambda: filled(dc.topology_case()),
    "targets": targets_case,
    "lds": lds_case,
    "delete_empty": lambda: empty_case(),
    "delete_pick": lambda: dc.claims_case(0),
    "noop": lambda: dc.count_case(3, "none"),
    "updates": lambda: updates_case(),
}
for _k in EDGES:
    BUILDERS["edge_diff_%d" % _k] = functools.partial(edge_case, _k, False)
    BUILDERS["edge_same_%d" % _k] = functools.partial(edge_case, _k, True)
for _kind in TEXT_KINDS:
    BUILDERS["text_" + _kind] = functools.partial(text_case, _kind)

ACTION = {"delete_empty": "delete", "delete_pick": "delete", "noop": "no-op"}  # every other case: replace


def filled(snap):
    """No node has room left: a picked candidate's pods need replacements."""
    for n in snap["stateNodes"]:
        dc.fill(n)
    return snap


def empty_case():
    """One drifted node has no pods: the command is that node, nothing is simulated."""
    snap = dc.lean(3, pods_of=lambda j: [("250m", None, None)] if j else [])
    return dc.mark(snap, "drift", seed=3)


def updates_case():
    snap = dc.mark(dc.small(seed=34, n=10, n_pending=2), "drift")
    for n in snap["stateNodes"]:
        dc.fill(n)
    return snap


@functools.lru_cache(maxsize=None)
def _snapshot(name):
    return BUILDERS[name]()


def snapshot(name):
    return copy.deepcopy(_snapshot(name))


@functools.lru_cache(maxsize=None)
def _reference(name, method):
    return pref.command(_snapshot(name), method)


def reference(name, method="drift"):
    """(the command document with pods per replacement, the picked simulation or None) for a case: computed once."""
    return copy.deepcopy(_reference(name, method))


def pods_by_uid(snap):
    out = {}
    for n in snap["stateNodes"]:
        for p in n["pods"]:
            out[p["metadata"]["uid"]] = p
    for p in snap.get("pendingPods", []):
        out[p["metadata"]["uid"]] = p
    return out
