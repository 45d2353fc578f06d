#!/usr/bin/env python3
"""What the launch lists cost a drop-in caller on C2 and C3.

Usage: python scripts/launch_profile.py [--steps 10] [--warmup 2] [--out profiles/launch_profile.json]
Per step, alternating, host wall-clock around calls that end in a device synchronisation:
  (a) solve_structured()                        the structured return path without launch lists
  (b) solve_structured(launch_lists=True)       the same with k_launch_lists; launch_ms is the kernel by HIP events
  (c) solve_structured() + ks_results_json      what a caller had to do before to get "launchInstanceTypes"
(a)-(c) include the Python accessor walk over every claim, which for (b) also builds the name lists.  The *_abi
figures leave Python's per-field cost out: ks_solve (+ one ks_results_nodeclaim_launch per claim for (b), +
ks_results_json for (c)) + ks_results_free, nothing copied into Python objects.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "karpenter-sigs_amd"))

from karpenter_amd import Scheduler, synth  # noqa: E402
from karpenter_amd import scheduler as ks  # noqa: E402


def _abi(l, sch, flag, with_json):
    """One C-ABI round trip in ms and (claims, launch_ms)."""
    o = ks._Opts(-1, 1, 1, 0, 0, flag)
    r = ctypes.c_void_p()
    n, nopt = ctypes.c_int(), ctypes.c_int()
    its, prices = ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.c_double)()
    t = time.perf_counter()
    ks._check(l.ks_solve(sch._h, ctypes.byref(o), ctypes.byref(r)))
    nc = l.ks_results_num_new_nodeclaims(r)
    if flag:
        for i in range(nc):
            l.ks_results_nodeclaim_launch(r, i, ctypes.byref(its), ctypes.byref(prices), ctypes.byref(n), ctypes.byref(nopt))
    if with_json:
        js = ctypes.c_void_p()
        ks._check(l.ks_results_json(r, ctypes.byref(js)))
        l.ks_free(js)
    ms = l.ks_results_launch_ms(r)
    l.ks_results_free(r)
    return (time.perf_counter() - t) * 1e3, nc, ms


def _wall(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def profile(name, snap, steps, warmup):
    sch = Scheduler(snap)
    l = ks.lib()
    ks._bind_accessors(l)
    rows = {k: [] for k in ("a", "b", "c", "a_abi", "b_abi", "c_abi", "launch_ms", "solve_kernel_ms")}
    claims = 0
    for step in range(warmup + steps):
        a, ra = _wall(lambda: sch.solve_structured())
        b, rb = _wall(lambda: sch.solve_structured(launch_lists=True))
        c, _ = _wall(lambda: sch.solve_structured(with_json=True))
        a_abi, claims, _ = _abi(l, sch, 0, False)
        b_abi, _, lms = _abi(l, sch, 1, False)
        c_abi, _, _ = _abi(l, sch, 0, True)
        if step < warmup:
            continue
        for k, v in (("a", a), ("b", b), ("c", c), ("a_abi", a_abi), ("b_abi", b_abi), ("c_abi", c_abi),
                     ("launch_ms", rb.launch_ms), ("solve_kernel_ms", ra.solve_kernel_ms)):
            rows[k].append(v)
        print("%s step %d: (a) %.3f (b) %.3f (c) %.3f ms | C-ABI (a) %.3f (b) %.3f (c) %.3f ms | launch_ms %.4f (%.4f)"
              % (name, step - warmup, a, b, c, a_abi, b_abi, c_abi, rb.launch_ms, lms), flush=True)
    out = {"config": name, "claims": claims, "steps": steps, "warmup": warmup}
    for k, v in rows.items():
        out[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "launch_profile.json"))
    ap.add_argument("--configs", default="C2,C3")
    args = ap.parse_args()
    makers = {"C2": synth.config2, "C3": synth.config3}
    results = [profile(c, makers[c](), args.steps, args.warmup) for c in args.configs.split(",")]
    doc = {"what": "ms per call, host wall-clock unless named *_ms (HIP events); see scripts/launch_profile.py",
           "build": ks.lib().ks_build_info().decode(), "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
