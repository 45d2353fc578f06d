"""Simulation Results with pods per target, from the oracle alone: the reference of the KS_CONS_PLACEMENTS and
ks_cons_sim_results tests.

simulateScheduling (helpers.go:73-127) of a set of candidates is one Solve: pods = the pending pods, then each
candidate's reschedulable pods in candidate order, then the deleting nodes' pods; stateNodes = the active nodes
without the candidates.  tests/disrupt_reference.simulate runs that Solve for one candidate and keeps the claims'
fields; here the Solve's newNodeClaims[i]["pods"] and existingNodes[i]["pods"] are kept too, and their indices are
mapped to UIDs through that Solve's pod list.
"""
import json

import disrupt_reference as ref
from oracle import bridge

CLAIM_FIELDS = ("nodePoolName", "instanceTypeOptions", "requests", "requirements")


def simulate(snap, names):
    """The Solve of the candidates `names` (in order) as ks_cons_sim_results states it:
    {"candidates", "allNonPendingScheduled", "newNodeClaims": [{nodePoolName, instanceTypeOptions, requests,
    requirements, pods: [uid]}], "existingNodes": [{name, pods: [uid]}] (only nodes that received pods),
    "unscheduled": [uid] (in the Solve's pod order)}."""
    names = list(names)
    active = [n for n in snap["stateNodes"] if not n.get("markedForDeletion")]
    deleting = [n for n in snap["stateNodes"] if n.get("markedForDeletion")]
    by = {n["name"]: n for n in active}
    pods = list(snap.get("pendingPods", []))
    for name in names:
        pods += [p for p in by[name]["pods"] if ref.reschedulable(p)]
    pods += [p for n in deleting for p in n["pods"] if ref.reschedulable(p)]
    nodes = [n for n in active if n["name"] not in names]
    rest = {k: v for k, v in snap.items() if k not in ("stateNodes", "pods")}
    rest["pods"] = pods
    rest["stateNodes"] = nodes
    res, _ = bridge.solve(json.dumps(rest))
    uid = [p["metadata"]["uid"] for p in pods]
    assert len(set(uid)) == len(uid)
    bad = {int(k) for k in res["podErrors"]}
    placed = set()
    kept = {n["name"]: n for n in nodes}
    existing = []
    for en in res["existingNodes"]:
        if not en["pods"]:
            continue
        n = kept[en["name"]]
        if not n.get("initialized", True) or not n.get("ready", True):
            bad |= set(en["pods"])  # helpers.go:115-124
        placed |= set(en["pods"])
        existing.append({"name": en["name"], "pods": [uid[i] for i in en["pods"]]})
    claims = []
    for c in res["newNodeClaims"]:
        placed |= set(c["pods"])
        claim = {k: c[k] for k in CLAIM_FIELDS}
        claim["pods"] = [uid[i] for i in c["pods"]]
        claims.append(claim)
    assert placed.isdisjoint({int(k) for k in res["podErrors"]})
    return {"candidates": names,
            "allNonPendingScheduled": all(ref.provisionable(pods[i]) for i in bad),
            "newNodeClaims": claims, "existingNodes": existing,
            "unscheduled": [uid[i] for i in range(len(pods)) if i not in placed]}


def trim_results(got):
    """The fields of a ks_cons_sim_results document the reference states."""
    return {k: got[k] for k in ("candidates", "allNonPendingScheduled", "newNodeClaims", "existingNodes", "unscheduled")}


def command(snap, method, all_sims=False):
    """disrupt_reference.command with every replacement carrying "pods" (UIDs in commit order); also returns the
    picked candidate's whole simulation (None without a pick)."""
    want = ref.command(snap, method, all_sims=all_sims)
    cmd = want["command"]
    sim = None
    if cmd["action"] != "no-op" and want["sims"]:
        sim = simulate(snap, cmd["candidates"])
        assert [{k: c[k] for k in CLAIM_FIELDS} for c in sim["newNodeClaims"]] == cmd["replacements"]
        assert sim["allNonPendingScheduled"]
        cmd["replacements"] = sim["newNodeClaims"]
    return want, sim


def trim(got):
    return ref.trim(got)


def formats_on(claim_pods, pods_by_uid, resource):
    """The quantity texts the pods of one NodeClaim write for `resource` (None where a pod does not name it)."""
    out = []
    for u in claim_pods:
        req = {}
        for ctr in pods_by_uid[u]["spec"]["containers"]:
            req.update(ctr.get("resources", {}).get("requests", {}))
        out.append(req.get(resource))
    return out
