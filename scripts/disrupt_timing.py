#!/usr/bin/env python3
"""Measurement: ks_cons_disrupt on C5 (synth.config5) with every node drifted at a distinct time and no empty
node, beside the same handle's consolidation pass.  The method runs one single-candidate simulation
per candidate -- the pass's single-node simulations without its multi-node prefixes -- plus k_disrupt_pick and
one copy.  Prints one JSON line; needs a GPU.

  wall_ms        host clock around Consolidator.disrupt (ends in the call's device synchronisation), the plan cached
  kernel_ms      HIP events around the method's queue sort + simulations (as a pass reports its own)
  first_wall_ms  the first call: it also builds and uploads the method's plan
  pass_*         run(keep=True) + decide of the same handle, measured in the same process, alternating with the method
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "karpenter-sigs_amd"))
from karpenter_amd import Consolidator, synth  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 5000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    snap = synth.config5(n)
    for i, nd in enumerate(snap["stateNodes"]):
        assert nd["pods"]
        nd["nodeClaimConditions"] = [{"type": "Drifted", "status": "True",
                                      "lastTransitionTime": synth._fmt_time(synth.NOW - 400000 + 7 * ((i * 7919) % n))}]
    c = Consolidator(json.dumps(snap))
    t0 = time.perf_counter()
    first = c.disrupt("drift")
    first_wall = (time.perf_counter() - t0) * 1e3
    for _ in range(3):  # warm both paths
        c.run(0, 1, keep=True)
        c.decide(None, 1, candidates=False, sims=False)
        c.disrupt("drift")
    rows = []
    for _ in range(reps):  # alternate the two
        t0 = time.perf_counter()
        _, pk = c.run(0, 1, keep=True)
        t1 = time.perf_counter()
        c.decide(None, 1, candidates=False, sims=False)
        t2 = time.perf_counter()
        doc = c.disrupt("drift")
        t3 = time.perf_counter()
        rows.append(((t3 - t2) * 1e3, doc["kernel_ms"], (t1 - t0) * 1e3, pk, (t2 - t1) * 1e3))
    med = lambda i: sorted(r[i] for r in rows)[len(rows) // 2]  # noqa: E731
    lo = lambda i: min(r[i] for r in rows)  # noqa: E731
    hi = lambda i: max(r[i] for r in rows)  # noqa: E731
    assert doc["command"] == first["command"]
    print(json.dumps({
        "nodes": n, "reps": reps, "candidates": len(doc["candidates"]), "pass_candidates": c.num_candidates,
        "pass_sims": c.num_sims, "action": doc["command"]["action"], "replacements": len(doc["command"]["replacements"]),
        "sims_reported": len(doc["sims"]), "plan": doc["plan"], "routes": c.last_routes,
        "first_wall_ms": round(first_wall, 3),
        "wall_ms": {"median": round(med(0), 3), "min": round(lo(0), 3), "max": round(hi(0), 3)},
        "kernel_ms": {"median": round(med(1), 3), "min": round(lo(1), 3), "max": round(hi(1), 3)},
        "pass_run_wall_ms": {"median": round(med(2), 3), "min": round(lo(2), 3), "max": round(hi(2), 3)},
        "pass_kernel_ms": {"median": round(med(3), 3), "min": round(lo(3), 3), "max": round(hi(3), 3)},
        "pass_decide_ms": {"median": round(med(4), 3)}}))


if __name__ == "__main__":
    main()
