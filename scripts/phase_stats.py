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
          "cycSortExactLe12", "cycSortExactLt50", "cycSortExactGe50",
          # inside cycSort: choosePivot's samples at the top frame, the regather; inside cycCross: the quick re-tests
          "cycPivot", "cycRegather", "cycCrossQuick"]:
    if k in st:
        print("%-16s %6.1f%%  %8.1f cyc/pod" % (k, 100.0 * st[k] / tot, st[k] / n))
closed, exact = st["sortsClosed"], st["sortsExact"]
print("re-sorts with a descent %d: fast %d exact %d closed %d;  n <= 12: %d, 12 < n < 50: %d, n >= 50: %d;  tplMemoHits %d" % (
    st["sortsWithDescent"], st["sortsWithDescent"] - exact - closed, exact, closed, st["sortsLe12"], st["sortsLt50"],
    st["sortsWithDescent"] - st["sortsLe12"] - st["sortsLt50"], st["tplMemoHits"]))
print("tplMaskFills %s tplMaskHits %s runRecs %s" % (st.get("tplMaskFills"), st.get("tplMaskHits"), st.get("runRecs")))
print("sortsRegs %s sortRegsOver %s sortRegsBail %s (general re-sorts finished on the register copy / with more claims "
      "than it holds / abandoned on a failed invariant)" % (st.get("sortsRegs"), st.get("sortRegsOver"), st.get("sortRegsBail")))
if "stepsOpen" in st:
    # the main-loop steps by kind, the threshold advances that move, the run capacities that come out 0
    for kind in ("Open", "Run", "Single"):
        c, k = st["cycStep" + kind], st["steps" + kind]
        print("steps %-6s %5d  %5.1f%%  %8.0f cyc/step" % (kind.lower(), k, 100.0 * c / tot, c / max(k, 1)))
    print("claim_full calls that move a threshold %d of %d (the scan's and one per run): %.1f%% (%.0f cyc each, inside cycFullThr)" % (
        st["thrMoves"], st["claimFull"] + st["runs"], 100.0 * st["cycThrMove"] / tot, st["cycThrMove"] / max(st["thrMoves"], 1)))
    calls = st["runCapFront"] + st["runCapFull"]
    print("claim_run_cap calls %d, returning 0: %d;  capBoundSkips %d;  thrBatchCalls %d thrMultiChunk %d" % (
        calls, st["runCapZero"], st["capBoundSkips"], st["thrBatchCalls"], st["thrMultiChunk"]))
    print("chainPods %d of %d main-loop steps" % (st["chainPods"], st["pops"] - st["runPods"]))
if closed:
    print("cycles per closed re-sort %.0f;  closedShiftDiff %s (moved entries whose shifted value differs from a regather)" % (
        st["cycSortClosed"] / closed, st.get("closedShiftDiff", "n/a")))
fast = st["sortsWithDescent"] - exact - closed
if fast:
    print("cycles per appended-claim (fast) re-sort %.0f" % (st["cycSortFast"] / fast))
if "sortsCross50" in st:
    print("sortsCross50 %d pivotArith %d pivotArithDiff %d;  sortsAppend50 %d appendClosed %d" % (
        st["sortsCross50"], st["pivotArith"], st["pivotArithDiff"], st["sortsAppend50"], st["appendClosed"]))
if exact:
    print("cycles per exact re-sort %.0f" % (st["cycSortExact"] / exact))
print("total cyc/pod %.1f  pops %d  sorts %d slow %d  claims %d  solve_kernel_ms %.2f" % (
    tot / n, st["pops"], st["sorts"], st["sortsWithDescent"], st["nclaims"], r.solve_kernel_ms))
