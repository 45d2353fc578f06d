#!/usr/bin/env python3
"""A/B of library variants (KS_LIB_VARIANT names; "main" = the main build), the protocol of DESIGN §7: rounds of one C2 bench
run and one C1 line per variant in turn, one process each; medians and spreads at the end; stops at the first failing
process.  Usage: scripts/bench_ab.py OUT.json ROUNDS variant..."""
import json
import os
import subprocess
import sys
import time

out, rounds, variants = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
doc = {"protocol": "python bench.py --gpus 1 --steps 20 --warmup 5, then --full --only-solve c1 --no-cpu-baseline; "
                   "the variants in turn, %d rounds" % rounds, "runs": []}


def run(variant, args, limit):
    env = dict(os.environ)
    env["KS_LIB_VARIANT"] = "" if variant == "main" else variant
    t = time.time()
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-u", "bench.py"] + args, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        print("FAILED rc", p.returncode, variant, args, p.stderr[-2000:], flush=True)
        sys.exit(p.returncode if p.returncode > 0 else 99)
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line), time.time() - t


for r in range(rounds):
    for v in variants:
        c2, s2 = run(v, ["--gpus", "1", "--steps", "20", "--warmup", "5"], 200)
        c1, s1 = run(v, ["--full", "--only-solve", "c1", "--no-cpu-baseline", "--steps", "20", "--warmup", "5"], 200)
        roof = c1.get("roofline", {})
        rec = {"round": r, "variant": v, "c2_ms_per_step": c2["ms_per_step"], "c2_pods_per_s": c2["value"],
               "c1_kernel_ms": roof.get("kernel_ms"), "c1_ms_per_step": c1.get("ms_per_step"), "secs": [round(s2, 1), round(s1, 1)]}
        doc["runs"].append(rec)
        print(json.dumps(rec), flush=True)
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
med = lambda xs: sorted(xs)[len(xs) // 2] if len(xs) % 2 else sum(sorted(xs)[len(xs) // 2 - 1:len(xs) // 2 + 1]) / 2
doc["summary"] = {}
for v in variants:
    a = [x["c2_ms_per_step"] for x in doc["runs"] if x["variant"] == v]
    b = [x["c1_kernel_ms"] for x in doc["runs"] if x["variant"] == v and x["c1_kernel_ms"] is not None]
    doc["summary"][v] = {"c2_median": round(med(a), 4), "c2_spread": round(max(a) - min(a), 4), "c2_runs": a,
                         "c1_kernel_median": round(med(b), 4) if b else None, "c1_kernel_spread": round(max(b) - min(b), 4) if b else None,
                         "c1_kernel_runs": b}
    print(v, doc["summary"][v], flush=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
