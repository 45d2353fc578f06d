#!/usr/bin/env python3
"""Diagnostic: per-phase cycle shares of k_solve (KS_LIB_VARIANT=stats build, s_memtime stamps; another stats
build, e.g. an earlier commit's, by setting KS_LIB_VARIANT before the call).
Never used for timing numbers; read the SHARES, not the totals."""
import json
import os
import sys

os.environ.setdefault("KS_LIB_VARIANT", "stats")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "karpenter-sigs_amd"))
from karpenter_amd import Scheduler, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
cfg = sys.argv[2] if len(sys.argv) > 2 else "c2"
snap = {"c1": lambda: synth.config1(), "c2": lambda: synth.config2(n), "c3": lambda: synth.config3(n),
        "c4": lambda: synth.config4(n, max(n // 5, 1))}[cfg]()
if cfg == "c1":
    n = len(snap["pods"])
r = Scheduler(json.dumps(snap)).solve()
st = r.stats
tot = max(st["cycTotal"], 1)
print(json.dumps(st))
for k in ["cycPop", "cycNodes", "cycNodeCommit", "cycSort", "cycQuick", "cycFull", "cycFullRs", "cycFullThr",
          "cycFullMasks", "cycFullApply", "cycCommit", "cycTemplates",
          # the step's sub-phases: inside cycSort, cycCommit and cycTemplates
          "cycSortFast", "cycSortExact", "cycSortClosed", "cycRunCap", "cycCross", "cycBulk", "cycLog",
          "cycTplDerive", "cycTplStore", "cycTplMax",
          # cycTplDerive and cycLog split further: candidates + tpl_rs copy, feas_masks, the filter loop, thresholds +
          # front test; a run's queue loads past the window, its log entries (or its record)
          "cycTplCand", "cycTplFeas", "cycTplFilter", "cycTplThr", "cycLogLoad", "cycLogStore",
          # the exact re-sorts by size (inside cycSortExact)
          "cycSortExactLe12", "cycSortExactLt50", "cycSortExactGe50"]:
    if k in st:
        print("%-16s %6.1f%%  %8.1f cyc/pod" % (k, 100.0 * st[k] / tot, st[k] / n))
closed, exact = st["sortsClosed"], st["sortsExact"]
print("re-sorts with a descent %d: fast %d exact %d closed %d;  n <= 12: %d, 12 < n < 50: %d, n >= 50: %d;  tplMemoHits %d" % (
    st["sortsWithDescent"], st["sortsWithDescent"] - exact - closed, exact, closed, st["sortsLe12"], st["sortsLt50"],
    st["sortsWithDescent"] - st["sortsLe12"] - st["sortsLt50"], st["tplMemoHits"]))
print("tplMaskFills %s tplMaskHits %s runRecs %s" % (st.get("tplMaskFills"), st.get("tplMaskHits"), st.get("runRecs")))
print("sortsRegs %s sortRegsOver %s sortRegsBail %s (general re-sorts finished on the register copy / with more claims "
      "than it holds / abandoned on a failed invariant)" % (st.get("sortsRegs"), st.get("sortRegsOver"), st.get("sortRegsBail")))
if closed:
    print("cycles per closed re-sort %.0f;  closedShiftDiff %s (moved entries whose shifted value differs from a regather)" % (
        st["cycSortClosed"] / closed, st.get("closedShiftDiff", "n/a")))
if exact:
    print("cycles per exact re-sort %.0f" % (st["cycSortExact"] / exact))
print("total cyc/pod %.1f  pops %d  sorts %d slow %d  claims %d  solve_kernel_ms %.2f" % (
    tot / n, st["pops"], st["sorts"], st["sortsWithDescent"], st["nclaims"], r.solve_kernel_ms))
