#!/usr/bin/env python3
"""KS_QUEUE_PACKED judged where it acts: kernel_ms - solve_kernel_ms, the HIP-event time of
everything but k_solve, and the wall time per Solve on C2, 20 timed Solves after 5 and the handle's first, one process
per measurement; two libraries in alternating pairs (KS_LIB_VARIANT names; "main" is the main build).  The chained
library is `make -C karpenter-sigs_amd variant VTU=ks_queue VDEFS=-DKS_QUEUE_PACKED=0 VNAME=chained`.
Usage: scripts/queue_setup_ab.py OUT.json PAIRS [CHAINED_VARIANT [PACKED_VARIANT]]   (defaults: chained main)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "karpenter-sigs_amd")]

if sys.argv[1] == "--child":
    import torch  # noqa: F401
    from karpenter_amd import Scheduler, synth

    sch = Scheduler(json.dumps(synth.config2(50000)))
    sch.solve(device=0, timing_only=True)
    for _ in range(5):
        sch.solve(device=0, timing_only=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    setup, ks = [], []
    for _ in range(20):
        r = sch.solve(device=0, timing_only=True)
        setup.append(r.kernel_ms - r.solve_kernel_ms)
        ks.append(r.solve_kernel_ms)
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) * 1000.0 / 20
    setup.sort()
    ks.sort()
    print(json.dumps({"setup_ms_median": round((setup[9] + setup[10]) / 2, 4), "setup_ms_min": round(setup[0], 4),
                      "setup_ms_max": round(setup[-1], 4), "solve_kernel_ms_median": round((ks[9] + ks[10]) / 2, 4),
                      "ms_per_step": round(el, 4)}))
    sys.exit(0)

out, pairs = sys.argv[1], int(sys.argv[2])
CH = sys.argv[3] if len(sys.argv) > 3 else "chained"
PK = sys.argv[4] if len(sys.argv) > 4 else "main"
doc = {"runs": []}
for i in range(pairs):
    for v in (CH, PK):
        env = dict(os.environ)
        env["KS_LIB_VARIANT"] = "" if v == "main" else v
        p = subprocess.run(["timeout", "-k", "10", "150", sys.executable, "-u", os.path.abspath(__file__), "--child"], cwd=ROOT,
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print("FAILED rc", p.returncode, v, p.stderr[-2000:], flush=True)
            sys.exit(p.returncode if p.returncode > 0 else 99)
        rec = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        rec.update(pair=i, variant=v)
        doc["runs"].append(rec)
        print(json.dumps(rec), flush=True)
diffs_setup, diffs_step = [], []
for i in range(pairs):
    a = [x for x in doc["runs"] if x["pair"] == i and x["variant"] == CH][0]
    b = [x for x in doc["runs"] if x["pair"] == i and x["variant"] == PK][0]
    diffs_setup.append(round(b["setup_ms_median"] - a["setup_ms_median"], 4))
    diffs_step.append(round(b["ms_per_step"] - a["ms_per_step"], 4))
for v in (CH, PK):
    xs = [x["setup_ms_median"] for x in doc["runs"] if x["variant"] == v]
    ys = [x["ms_per_step"] for x in doc["runs"] if x["variant"] == v]
    doc[v] = {"setup_ms": xs, "setup_spread": round(max(xs) - min(xs), 4), "ms_per_step": ys, "step_spread": round(max(ys) - min(ys), 4)}
doc["packed_minus_chained_setup_ms"] = diffs_setup
doc["packed_minus_chained_ms_per_step"] = diffs_step
print(json.dumps({k: doc[k] for k in doc if k != "runs"}, indent=1))
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
