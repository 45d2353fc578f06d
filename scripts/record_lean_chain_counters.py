#!/usr/bin/env python3
"""Record tests/golden/lean_chain_counters.json: per problem of tests/lean_chain_cases.py the LEAN Solve's algBytes
and its claim_run_cap calls (runCapFront + runCapFull).  Run it against the library of the commit before KS_CAP_BOUND
existed, or one built with -DKS_CAP_BOUND=0 (KS_LIB_VARIANT names it): a later build's calls and capBoundSkips must add
up to the recorded calls.  Every problem is checked against the oracle first.
Usage: scripts/record_lean_chain_counters.py [output path]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "karpenter-sigs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import lean_chain_cases as cases  # noqa: E402
import problems  # noqa: E402
from karpenter_amd import Scheduler  # noqa: E402
from oracle import bridge  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "lean_chain_counters.json")
doc = {"recordedWith": os.environ.get("KS_LIB_VARIANT", ""), "cases": {}}
for name, (mk, _) in sorted(cases.CASES.items()):
    s = json.dumps(mk())
    want, _ = bridge.solve(s)
    got = Scheduler(s).solve()
    assert problems.canonical(want) == got.canonical(), name
    st = got.stats
    assert st.get("capBoundSkips", 0) == 0, "record with a build that always calls claim_run_cap"
    doc["cases"][name] = {"algBytes": st["algBytes"], "runCapCalls": st["runCapFront"] + st["runCapFull"],
                          "runs": st["runs"], "claimFull": st["claimFull"], "nclaims": st["nclaims"]}
    print(name, doc["cases"][name], flush=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=1, sort_keys=True)
    f.write("\n")
