"""ks_solve's re-plan for NodeClaim capacity on the GPU, at reduced LDS budgets where a few hundred pods cross it.

A Solve that needs more NodeClaims than its plan has positions for (Plan::KO) stops with KE_CLAIM_CAP; the host
re-plans (make_plan's wideKO levels 1 and 2), launches again and remembers the level on the handle.  Every case of
tests/replan_cases.py (whose regime tests/test_claim_cap_plans.py proves on the CPU) compares the canonical Results of
Scheduler.solve(lds_budget=B) with the oracle's -- NodeClaims in final order with their pods in commit order -- and
asserts the launches ("stats"."route"."launches") and the last launch's plan ("stats"."plan") against the plans
ks_problem_inspect reports; no capacity is written down here.

What a failed attempt leaves behind is what the relaunch starts from: the claim state past KL in HBM, the run
records k_log_expand expands after every attempt, the claim-run carry, the remembered level and, after a lean exit, the
remembered instantiation.  The cases cross each edge from both sides: claims == KO of a level (no re-plan) and
KO + 1 (the next level), the level that is skipped because it holds fewer positions than the plan that ran, and the
budget at which no level raises KO (the Solve fails after its one launch and leaves the handle as it was)."""
import copy
import json

import pytest

import replan_cases as rp
from karpenter_amd import Consolidator, Scheduler, inspect
from karpenter_amd.scheduler import KsError
from test_solve_gpu import _diff

pytestmark = pytest.mark.gpu

OK_CASES = [n for n in rp.NAMES if rp.CASES[n]["error"] is None]


def _cells(launches):
    return [(l["family"], l["rt"], l["tl"], l["lean"]) for l in launches]


def _level_plan(name, level):
    pl = rp.levels(inspect(rp.snapshot(name)), rp.CASES[name]["budget"])[level]
    return {"wide": level, "KO": pl["KO"], "KL": pl["KL"], "talloc": pl["talloc"], "lds": pl["lds"]}


def _assert_oracle(name, got):
    want, _ = rp.oracle(name)
    d = _diff(want, got)
    assert d is None, d
    assert got.stats["nclaims"] == len(want["newNodeClaims"])


def _capacity_error(fn, ko):
    with pytest.raises(KsError) as e:
        fn()
    assert e.value.code == rp.CAPACITY, e.value
    assert "NodeClaim capacity (%d per Solve" % ko in str(e.value), e.value
    return str(e.value)


@pytest.mark.parametrize("name", OK_CASES)
def test_replan_case(name):
    case = rp.CASES[name]
    got = Scheduler(rp.snapshot(name)).solve(lds_budget=case["budget"])
    route, plan = got.stats["route"], got.stats["plan"]
    print(name, "K", rp.ks(name), "claims", got.stats["nclaims"], "launches", _cells(route["launches"]), "plan", plan,
          "runRecs", got.stats["runRecs"])
    _assert_oracle(name, got)
    assert len(route["launches"]) <= 4
    assert _cells(route["launches"]) == case["cells"], route
    assert all(l["n"] == 1 for l in route["launches"])
    assert _cells([route]) == case["cells"][-1:]  # the outer fields are the last launch's
    assert plan == _level_plan(name, case["wide"])
    if case["wide"]:  # 64 LDS-resident claims, the rest of this Solve's in HBM
        assert plan["KL"] == 64 < got.stats["nclaims"] <= plan["KO"]
    if name == "lean-runs":
        assert (got.stats["runRecs"] > 0) == (inspect(rp.snapshot(name))["logRuns"] == 1)


def test_remembered_level():
    """The handle of the K0 + 1 case: the next Solve at the same budget launches once, at level 1, with the same
    Results; so do three replicas in one launch."""
    name = "lean-K0+1"
    budget = rp.CASES[name]["budget"]
    sch = Scheduler(rp.snapshot(name))
    first = sch.solve(lds_budget=budget)
    assert len(first.stats["route"]["launches"]) == 2
    for replicas in (1, 3):
        again = sch.solve(lds_budget=budget, replicas=replicas)
        _assert_oracle(name, again)
        assert again.canonical() == first.canonical()
        launches = again.stats["route"]["launches"]
        assert _cells(launches) == [rp.L] and launches[0]["n"] == replicas, launches
        assert again.stats["plan"] == _level_plan(name, 1)


def test_capacity_error_names_the_largest_capacity():
    """K2 + 1 claims: every level ran and the last one, the largest, is the one reported -- the same error with the
    Results collected and timing_only.  The handle then solves at the default budget."""
    name = "lean-K2+1"
    case = rp.CASES[name]
    k = rp.ks(name)
    sch = Scheduler(rp.snapshot(name))
    msg = _capacity_error(lambda: sch.solve(lds_budget=case["budget"]), k[2])
    other = Scheduler(rp.snapshot(name))
    assert _capacity_error(lambda: other.solve(lds_budget=case["budget"], timing_only=True), k[2]) == msg
    for handle in (sch, other):
        got = handle.solve()
        _assert_oracle(name, got)
        assert len(got.stats["route"]["launches"]) == 1


def test_no_level_raises_the_capacity():
    """Budget 6000: both wide plans hold fewer positions than the default plan, so a Solve of K0 + 1 claims fails
    after the launch that ran, naming K0, and the handle remembers nothing: its next Solve reports the route and
    the plan of a fresh handle's."""
    name = "lean-no-raise"
    case = rp.CASES[name]
    k = rp.ks(name)
    assert k[1] <= k[0] and k[2] <= k[0]
    sch = Scheduler(rp.snapshot(name))
    _capacity_error(lambda: sch.solve(lds_budget=case["budget"]), k[0])
    got = sch.solve()
    fresh = Scheduler(rp.snapshot(name)).solve()
    print("after the failed Solve", got.stats["route"], got.stats["plan"], "fresh", fresh.stats["route"], fresh.stats["plan"])
    _assert_oracle(name, got)
    assert got.stats["route"] == fresh.stats["route"] and got.stats["plan"] == fresh.stats["plan"]
    assert got.stats["plan"]["wide"] == 0 and len(got.stats["route"]["launches"]) == 1
    # ... and at the small budget again, the same answer from one launch
    _capacity_error(lambda: sch.solve(lds_budget=case["budget"]), k[0])


def test_drift_pass_over_its_claim_capacity():
    """Consolidation reports the same condition as an error: the drift pass of tests/test_disrupt_gpu.py's
    70-replacement cluster at a budget whose plan holds fewer than 70 NodeClaims fails with KS_ERR_CAPACITY, and the
    handle then returns the reference's command at the default budget.  A failed pass reports no plan, so KO is read
    from a cluster of the same dimensions whose heaviest candidate needs 24 NodeClaims (1-cpu pods, three per
    4-cpu instance type)."""
    import disrupt_cases as dc
    from test_disrupt_gpu import both

    snap = dc.claims_case(70)
    light = copy.deepcopy(snap)
    heavy = max(light["stateNodes"], key=lambda n: len(n["pods"]))
    assert len(heavy["pods"]) == 70
    for p in heavy["pods"]:
        p["spec"]["containers"][0]["resources"]["requests"]["cpu"] = "1"
    c, lc = Consolidator(json.dumps(snap)), Consolidator(json.dumps(light))
    got, _, _ = both(light, handle=lc)
    assert len(got["command"]["replacements"]) == 24
    assert c.disrupt("drift")["plan"] == got["plan"]
    plan = None
    for budget in range(10 * 1024, 2 * 1024, -256):  # the first budget whose plan holds fewer than 70 claims
        plan = lc.disrupt("drift", lds_budget=budget)["plan"]
        if plan["KO"] < 70:
            break
        assert c.disrupt("drift", lds_budget=budget)["plan"] == plan
    print("budget", budget, "plan", plan)
    assert 24 <= plan["KO"] < 70, (budget, plan)
    with pytest.raises(KsError) as e:
        c.disrupt("drift", lds_budget=budget)
    assert e.value.code == rp.CAPACITY, e.value
    got, _, _ = both(snap, handle=c)
    assert len(got["command"]["replacements"]) == 70
