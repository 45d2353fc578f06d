#!/usr/bin/env python3
"""The cost of the logged re-run: ks_cons_sim_results' kernel_ms for one single-node simulation of the C5
cluster and of C5 + topology, and ks_cons_disrupt's placements_ms for a Drift command there (every node full so
that the pick needs replacements; the first 8 nodes drifted, or 64 or 512 when none of fewer can move its pods, as
on the topology cluster).  No threshold: the re-run has no parent to compare with.

    python scripts/placements_cost.py [out.json] [nodes]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "karpenter-sigs_amd"))
from karpenter_amd import Consolidator, synth  # noqa: E402

KIND = "Drifted"


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 4), "median": round(xs[len(xs) // 2], 4), "max": round(xs[-1], 4), "n": len(xs)}


def measure(snap, reps=7):
    c = Consolidator(json.dumps(snap))
    _, pass_ms = c.run(0, 1, keep=True)
    sim = c.num_sims - c.num_candidates  # the first candidate's own simulation
    res = [c.sim_results(sim) for _ in range(reps + 1)][1:]
    out = {"sims": c.num_sims, "pass_kernel_ms": round(pass_ms, 4), "sim": sim,
           "sim_pods": sum(len(t["pods"]) for t in res[0]["newNodeClaims"] + res[0]["existingNodes"]) + len(res[0]["unscheduled"]),
           "sim_results_kernel_ms": stats([r["kernel_ms"] for r in res]), "route": c.last_routes[-1]}
    # Drift over the same cluster with every node full: the picked simulation opens NodeClaims
    full = json.loads(json.dumps(snap))
    for n in full["stateNodes"]:
        n["available"] = {k: "0" for k in n["available"]}
    for drifted in (8, 64, 512):
        for i, n in enumerate(full["stateNodes"][:drifted]):
            n["nodeClaimConditions"] = [{"type": KIND, "status": "True",
                                         "lastTransitionTime": synth._fmt_time(synth.NOW - 100000 + 61 * i)}]
        d = Consolidator(json.dumps(full))
        docs = [d.disrupt("drift", placements=True) for _ in range(reps + 1)][1:]
        cmd = docs[0]["command"]
        if cmd["action"] == "replace":
            break
    out["disrupt"] = {"drifted": drifted, "simulated": len(docs[0]["sims"]), "action": cmd["action"],
                      "replacements": len(cmd["replacements"]),
                      "pods": sum(len(r["pods"]) for r in cmd["replacements"]),
                      "kernel_ms": stats([x["kernel_ms"] for x in docs]),
                      "placements_ms": stats([x["placements_ms"] for x in docs]), "route": d.last_routes[-1]}
    return out


def main():
    nodes = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
    doc = {"c5": measure(synth.config5(nodes)),
           "c5_topology": measure(synth.cluster_snapshot(nodes, 20, 400, seed=4205, topology=20))}
    text = json.dumps(doc, indent=1)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
