"""Drift / Expiration ComputeCommand (disruption/drift.go, expiration.go) replayed in Python over the oracle,
independently of the library: the reference the ks_cons_disrupt tests compare with.

- Eligibility: the oracle's consolidate(all_sims=True) candidate list applies NewCandidate and filterCandidates
  (PDBs, do-not-disrupt pods).  On snapshots whose NodePools are WhenUnderutilized with no do-not-consolidate
  annotation (and no consolidateAfter Never) consolidation's own ShouldDisrupt removes nothing, so that list,
  intersected with the nodes carrying the method's condition, is the method's candidate set.
- Order: the snapshot's "candidates" order, then Python's stable sort by the condition's lastTransitionTime
  (callers use distinct times; Go's sort.Slice is stable only up to 12 elements).
- Empty candidates: if any has no reschedulable pod the command is all of them, nothing is simulated.
- Otherwise one Solve per candidate (pending pods + the candidate's pods + the deleting nodes' pods over the
  active nodes without the candidate), the post-check of helpers.go:115-124 (a pod placed on a node that is not
  initialized or not Ready is an error), and the command of the first candidate without an error on a
  non-pending pod.

A replacement is {nodePoolName, instanceTypeOptions, requests, requirements} as the oracle's Solve renders a
NodeClaim.  (The library reports no pods per replacement: a simulation keeps no commit log.)
"""
import copy
import json
from concurrent.futures import ThreadPoolExecutor

from oracle import bridge

CONDITION = {"drift": "Drifted", "expiration": "Expired"}


def _condition(node, kind):
    for c in node.get("nodeClaimConditions") or []:
        if c.get("type") == kind:  # GetCondition: the first of its type
            return c
    return None


def _expire_is_duration(snap, pool):
    for p in snap.get("nodePools", []):
        if p["metadata"]["name"] == pool:
            v = (p.get("spec", {}).get("disruption") or {}).get("expireAfter")
            return isinstance(v, str) and v != "Never"
    return False


def reschedulable(p):
    """GetNodePods' filter (utils/node/node.go:32-53) for the pods tests build."""
    owners = [o.get("kind") for o in p["metadata"].get("ownerReferences", [])]
    if "DaemonSet" in owners or "Node" in owners:
        return False
    if p.get("status", {}).get("phase") in ("Succeeded", "Failed"):
        return False
    return not p["metadata"].get("deletionTimestamp")


def provisionable(p):
    """pod.IsProvisionable for the pods tests build: a pending pod (not bound)."""
    return not p["spec"].get("nodeName")


def without_conditions(snap):
    """The snapshot as the oracle's consolidation reads it for eligibility: consolidateAfter Never (which only
    consolidation's own ShouldDisrupt tests) taken out, so a drifted node of such a pool stays listed."""
    s = copy.copy(snap)
    s.pop("featureGates", None)
    for key in ("nodePools", "nodeClaimTemplates"):
        pools = copy.deepcopy(s.get(key, []))
        for p in pools:
            d = p.get("spec", {}).get("disruption")
            if d and d.get("consolidateAfter") == "Never":
                del d["consolidateAfter"]
        s[key] = pools
    return s


def eligible(snap):
    """Names passing NewCandidate + filterCandidates (the oracle's candidate list), as a set."""
    doc, _ = bridge.consolidate(json.dumps(without_conditions(snap)), all_sims=True, threads=8)
    return {c["name"] for c in doc["candidates"]}, doc


def candidates(snap, method, names=None):
    """The method's candidates in its order."""
    kind = CONDITION[method]
    if method == "drift" and not snap.get("featureGates", {}).get("drift", True):
        return []
    if names is None:
        names, _ = eligible(snap)
    by = {n["name"]: n for n in snap["stateNodes"]}
    out = []
    for name in snap["candidates"]:
        n = by.get(name)
        if n is None or name not in names:
            continue
        c = _condition(n, kind)
        if not c or c.get("status") != "True":
            continue
        if method == "expiration" and not _expire_is_duration(snap, n["labels"].get("karpenter.sh/nodepool")):
            continue
        out.append((c["lastTransitionTime"], name))
    out.sort(key=lambda t: t[0])  # stable; RFC 3339 UTC seconds sort as text
    return [name for _, name in out]


class _Solves:
    """One candidate's Solve input after another, over one snapshot: every node is serialised once."""

    def __init__(self, snap):
        self.snap = snap
        self.active = [n for n in snap["stateNodes"] if not n.get("markedForDeletion")]
        deleting = [n for n in snap["stateNodes"] if n.get("markedForDeletion")]
        self.tail_pods = [p for n in deleting for p in n["pods"] if reschedulable(p)]
        self.node_json = {n["name"]: json.dumps(n) for n in self.active}
        rest = {k: v for k, v in snap.items() if k not in ("stateNodes", "pods")}
        self.rest_json = json.dumps(rest)[:-1]  # the object, left open

    def input(self, name):
        cand = next(n for n in self.active if n["name"] == name)
        pods = list(self.snap.get("pendingPods", [])) + [p for p in cand["pods"] if reschedulable(p)] + self.tail_pods
        nodes = [n for n in self.active if n["name"] != name]
        text = "%s,\"pods\":%s,\"stateNodes\":[%s]}" % (self.rest_json, json.dumps(pods),
                                                       ",".join(self.node_json[n["name"]] for n in nodes))
        return pods, nodes, text


def simulate(snap, name, solves=None):
    """simulateScheduling (helpers.go:73-127) of one candidate: (allNonPendingScheduled, the Solve's NodeClaims).
    The Solve: pods = pending + the candidate's + the deleting nodes'; stateNodes = the active ones without it."""
    pods, nodes, text = (solves or _Solves(snap)).input(name)
    res, _ = bridge.solve(text)
    bad = {int(k) for k in res["podErrors"]}
    by = {n["name"]: n for n in nodes}
    for en in res["existingNodes"]:
        n = by[en["name"]]
        if not n.get("initialized", True) or not n.get("ready", True):
            bad |= set(en["pods"])
    ok = all(provisionable(pods[i]) for i in bad)
    claims = [{"nodePoolName": c["nodePoolName"], "instanceTypeOptions": c["instanceTypeOptions"],
               "requests": c["requests"], "requirements": c["requirements"]} for c in res["newNodeClaims"]]
    return ok, claims


def command(snap, method, all_sims=False):
    """{"candidates", "command": {"action", "candidates", "replacements"}, "sims"} as ks_cons_disrupt reports."""
    names, doc = eligible(snap)
    order = candidates(snap, method, names)
    by = {n["name"]: n for n in snap["stateNodes"]}
    empty = [n for n in order if not [p for p in by[n]["pods"] if reschedulable(p)]]
    if empty:
        return {"candidates": order, "command": {"action": "delete", "candidates": empty, "replacements": []}, "sims": []}
    single = {s["candidates"][0]: s for s in doc["single"]["sims"]}
    cmd = {"action": "no-op", "candidates": [], "replacements": []}
    sims, picked = [], False
    solves = _Solves(snap)
    # (the Solves are independent: a chunk at a time on a few threads, consumed in the method's order)
    with ThreadPoolExecutor(max_workers=8) as pool:
        for at in range(0, len(order), 32):
            if picked and not all_sims:
                break
            chunk = order[at:at + 32]
            for name, (ok, claims) in zip(chunk, pool.map(lambda nm: simulate(snap, nm, solves), chunk)):
                if picked and not all_sims:
                    break
                # the oracle's own single-node simulation of the candidate must agree
                want = single[name]
                assert (ok, len(claims)) == (want["allNonPendingScheduled"], want["newNodeClaims"]), \
                    (name, ok, len(claims), want)
                sims.append({"candidate": name, "allNonPendingScheduled": ok, "newNodeClaims": len(claims)})
                if ok and not picked:
                    picked = True
                    cmd = {"action": "replace" if claims else "delete", "candidates": [name], "replacements": claims}
    return {"candidates": order, "command": cmd, "sims": sims}


def trim(got):
    """The fields of a ks_cons_disrupt document the reference states."""
    return {"candidates": got["candidates"], "command": got["command"], "sims": got["sims"]}
