"""Launch lists of a consolidation pass at the C5 shape (5k nodes / 100k pods, 5,100 simulations) on one GPU: the
pass's kernel_ms (HIP events) with ks_solve_opts.launch_lists clear and set, alternating on one handle after four
warm-up pairs, and ks_cons_launch_ms, the launch-list kernel's own event time.  Two clusters: C5 as the benchmark
builds it (no simulation's action is replace, so every workgroup returns at once) and C5 with every node full (most
single-node simulations replace).  Writes profiles/launch_cmd_c5.json (or the path given)."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "launch_cmd_c5.json")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "karpenter-sigs_amd"))
from karpenter_amd import Consolidator, synth

def measure(snap, label):
    t = time.time()
    c = Consolidator(json.dumps(snap))
    print(label, "handle in %.1fs, sims %d" % (time.time() - t, c.num_sims), flush=True)
    off, on, lms, wall_off, wall_on = [], [], [], [], []
    for step in range(14):
        for flag in (False, True):
            t0 = time.perf_counter()
            _, ms = c.run(0, 1, keep=True, launch_lists=flag)
            w = (time.perf_counter() - t0) * 1e3
            if step < 4:
                continue
            (on if flag else off).append(ms); (wall_on if flag else wall_off).append(w)
            if flag:
                lms.append(c.launch_ms())
    c.run(0, 1, keep=True, launch_lists=True)
    doc = c.decide(None, 1, all_sims=True, candidates=False)
    nrep = sum(s["action"] == "replace" for m in ("multi", "single") for s in doc[m]["sims"])
    med = statistics.median
    return {"shape": label, "sims": c.num_sims, "replace_sims": nrep, "steps": len(off), "order": "off, on alternating; 4 warm-up pairs",
            "kernel_ms_off": [min(off), med(off), max(off)], "kernel_ms_on": [min(on), med(on), max(on)],
            "launch_ms": [min(lms), med(lms), max(lms)],
            "run_wall_ms_off": [min(wall_off), med(wall_off), max(wall_off)], "run_wall_ms_on": [min(wall_on), med(wall_on), max(wall_on)]}


c5 = synth.config5()
full = synth.config5()
for n in full["stateNodes"]:
    n["available"] = {k: "0" for k in n["available"]}
out = {"values": "[min, median, max] over the steps, milliseconds",
       "runs": [measure(c5, "C5"), measure(full, "C5, every node full")]}
json.dump(out, open(OUT, "w"), indent=1)
print(json.dumps(out))
