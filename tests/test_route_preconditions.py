"""What tests/test_route_matrix_gpu.py relies on, checked with the oracle and the host-only inspectors (no GPU): every
case of the route matrix (tests/resource_cases.py) has the inputs its cell needs and decides something.

The dispatch itself is not restated here: the library reports the launched k_solve instantiation and the GPU tests
compare that with the cell.  These tests pin what the dispatch reads -- the live-resource count R, topology groups,
resource-only pods (lean), a negative request (negReq) and whether the instance-type tables fit the LDS plan
(talloc) -- so that a change of a generator or of the planner shows here, on the CPU, before a GPU case goes vacuous.
They also assert that the extra resource names bind: the same snapshot without those requests (a negative request
set to 0) gets another answer from the oracle, so a kernel that ignored resource 5 or 16 would be caught."""
import json

import pytest

import problems
import resource_cases as rc
from karpenter_amd import inspect, inspect_consolidation
from oracle import bridge

SOLVE = [c["name"] for c in rc.SOLVE_CASES]
CONS = [c["name"] for c in rc.CONS_CASES]
FULL_BUDGET = 160 * 1024 - 256


def _plan(case, dims):
    return dims["plans"][str(case["budget"] or FULL_BUDGET)]


def _cell_inputs(case, R, G, lean, neg, talloc):
    """The dimensions the case's last launch needs (a lean-exit case ends in its non-lean cell, but is encoded lean)."""
    fam, rt, tl, ln = case["cells"][0]
    assert R == case["R"]
    assert (rt == R) if R in (3, 4) else (rt == 0)
    assert (G > 0) == case["topo"] == fam.endswith("_topo")
    assert neg == (1 if case["neg"] else 0)
    assert talloc == tl
    if ln:
        assert lean == 1 and tl == 1
    elif tl and rt and not case["topo"]:
        assert lean == 0  # (a lean problem with its tables in LDS would run LEAN)


@pytest.mark.parametrize("name", SOLVE)
def test_solve_case_inputs(name):
    case = rc.CASES[name]
    d = inspect(rc.snapshot(name))
    pl = _plan(case, d)
    _cell_inputs(case, d["R"], d["G"], d["lean"], d["negReq"], pl["talloc"])
    if case["neg"]:
        assert pl["tsort"] == 0
    want = rc.oracle(name)
    claims = len(want["newNodeClaims"])
    # no re-plan for NodeClaim capacity: the reported route is the case's cell alone
    assert claims <= pl["KO"]
    if case["small_lds"]:
        assert pl["KL"] < claims <= pl["KO"]
    if not case["degenerate_ok"]:
        assert claims > 0 and want["podErrors"] and any(n["pods"] for n in want["existingNodes"])
    elif len(case["cells"]) > 1:
        assert want["podErrors"], "a lean-exit case must push a pod back"
    else:
        assert claims > 0


@pytest.mark.parametrize("name", [n for n in SOLVE if rc.CASES[n]["strip"]])
def test_solve_case_binds(name):
    other = problems.canonical(bridge.solve(rc.stripped(name))[0])
    assert other != rc.oracle(name)


def _sim_key(x):
    return x["allNonPendingScheduled"], x["newNodeClaims"], (x.get("claim0") or {}).get("instanceTypeOptions")


@pytest.mark.parametrize("name", CONS)
def test_cluster_case_inputs(name):
    case = rc.CASES[name]
    d = inspect_consolidation(rc.snapshot(name))
    pl = d["simPlan"]
    _cell_inputs(case, d["R"], d["G"], d["lean"], d["negReq"], pl["talloc"])
    if case["neg"]:
        assert pl["tsort"] == 0
    want = rc.oracle(name)
    sims = want["multi"]["sims"] + want["single"]["sims"]
    assert len(sims) == d["sims"] >= 20
    if not case["degenerate_ok"]:
        assert any(s["newNodeClaims"] > 0 for s in sims) and any(s["newNodeClaims"] == 0 for s in sims)
    assert any(s["allNonPendingScheduled"] for s in sims)
    assert want["multi"]["command"]["action"] != "no-op" or want["single"]["command"]["action"] != "no-op"
    if case["reruns"]:
        assert any(p["carried"] for p in want["multi"]["path"])


@pytest.mark.parametrize("name", [n for n in CONS if rc.CASES[n]["strip"]])
def test_cluster_case_binds(name):
    want = rc.oracle(name)
    other = bridge.consolidate(rc.stripped(name), all_sims=True)[0]
    differ = 0
    for k in ("multi", "single"):
        a, b = want[k]["sims"], other[k]["sims"]
        differ += abs(len(a) - len(b)) + sum(1 for x, y in zip(a, b) if _sim_key(x) != _sim_key(y))
    commands = any(want[k]["command"] != other[k]["command"] for k in ("multi", "single"))
    assert differ >= 3 or commands, differ


def test_every_cell_of_the_matrix_has_a_case():
    """Part of the matrix's definition: each (family, rt, {lean, tl, notl}) cell, the generic cells at R = 5 and 16,
    R = 1, 2 and 8 and a negative request at R = 4 and 5 once per family."""
    have = {}
    for c in rc.CASES.values():
        have.setdefault(c["cells"][-1] if c["cells"][0][0].startswith("solve") else c["cells"][0], set()).add(c["R"])
        have.setdefault(c["cells"][0], set()).add(c["R"])
    for fam, topo in (("solve", False), ("solve_topo", True), ("sims", False), ("sims_topo", True)):
        for rt in (3, 4, 0):
            for tl, lean in ((1, 0), (0, 0)) + (((1, 1),) if rt and not topo else ()):
                assert (fam, rt, tl, lean) in have, (fam, rt, tl, lean)
        assert {5, 16} <= have[(fam, 0, 1, 0)] and {5, 16} <= have[(fam, 0, 0, 0)]
        assert {1, 2, 8} <= have[(fam, 0, 1, 0)]
        negs = {c["R"] for c in rc.CASES.values() if c["neg"] and c["cells"][0][0] == fam}
        assert negs == {4, 5}
    assert ("sims_mixed", 4, 1, 1) in have
