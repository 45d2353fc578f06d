"""The topology kernels at their shape edges, bit for bit against the oracle: more than 64 non-hostname domains, the
requirement-word boundary, a custom topology key, key slots past the simulations' LDS window, node indices past it, count
words outside the LDS-resident prefix, and the Solve plans with the whole count table, the small prefix alone, or no
node-domain table in LDS.  The inputs are tests/wide_topology_cases.py; tests/test_wide_topology_preconditions.py proves on
the CPU that each is in its cell and that its answer depends on the edge, so a kernel that dropped a second stride, a
word or a slot gets another answer than the one compared here.

Every test also asserts the launched k_solve family (stats.route / Consolidator.last_routes), and where a budget is
passed, that the launch's plan is the one the precondition test pinned."""
import json

import pytest

import disrupt_reference as ref
import wide_topology_cases as w
from karpenter_amd import Consolidator, Scheduler, inspect
from oracle import bridge
from test_cons_gpu import _first_diff
from test_topology_gpu import _diff

pytestmark = pytest.mark.gpu


def _solve(snapshot, want, budget=0):
    got = Scheduler(json.dumps(snapshot)).solve(lds_budget=budget)
    d = _diff(want, got.canonical())
    assert d is None, d
    route = got.stats["route"]
    assert route["family"] == "solve_topo" and route["lean"] == 0, route
    assert [l["family"] for l in route["launches"]] == ["solve_topo"], route  # no re-plan, one launch
    return got


@pytest.mark.parametrize("name", list(w.SOLVE_CASES))
def test_solve_case(name):
    """One pod whose only admissible domain sits at a stride, word or universe edge (PodErrors verbatim, with the wide
    `counts = map[...]`)."""
    _solve(w.solve(name)["snapshot"], w.oracle_solve(name))


@pytest.mark.parametrize("kind,nv", w.CLOSED_FORM)
def test_closed_forms(kind, nv):
    """2 nv identical pods over nv zones: every count of the group is read and written as the Solve goes."""
    snap = w.closed_form_case(kind, nv)["snapshot"]
    want, _ = bridge.solve(json.dumps(snap))
    want.pop("stats", None)
    _solve(snap, want)


@pytest.mark.parametrize("cell", w.PLAN_CELLS)
def test_solve_plan_cells(cell):
    """One wide problem (2686 count words, 2005 of them in the small prefix; 96 existing nodes) at the budgets whose plans
    keep the whole count table, the small prefix alone, or no node-domain table in LDS."""
    case = w.plan_case(cell)
    budget, pl = w.plan_budget(inspect(json.dumps(case["snapshot"])), cell)
    assert budget is not None
    want, _ = bridge.solve(json.dumps(case["snapshot"]))
    want.pop("stats", None)
    got = _solve(case["snapshot"], want, budget=0 if budget == w.FULL_BUDGET else budget)
    plan = got.stats["plan"]
    assert plan["wide"] == 0 and {k: plan[k] for k in ("KO", "KL", "talloc", "lds")} == \
        {k: pl[k] for k in ("KO", "KL", "talloc", "lds")}, (plan, pl)  # (lds: the plan's bytes, tcl and tdl included)
    assert got.stats["route"]["tl"] == pl["talloc"]


@pytest.mark.parametrize("name", list(w.CONS_CASES))
def test_simulation_case(name):
    """A pass over a widened cluster: every simulation's outcome and both commands, all_sims both ways."""
    c = Consolidator(json.dumps(w.cons(name)["snapshot"]))
    recs, _ = c.run(0, 1)
    recs = bytes(recs)
    launches = c.last_routes
    assert launches and {l["family"] for l in launches} == {"sims_topo"}, launches
    assert sum(l["n"] for l in launches) == c.num_sims
    for all_sims in (True, False):
        d = _first_diff(w.oracle_cons(name, all_sims), c.decide(recs, 1, all_sims))
        assert d is None, d


def test_drift_command_over_wide_zones():
    """The picked simulation's NodeClaim requirements, exported by k_disrupt_pick: a 68-value zone set over three
    requirement words, and a single zone in the third."""
    snap = w.drift_wide_zones()["snapshot"]
    c = Consolidator(json.dumps(snap))
    for all_sims in (False, True):
        got = c.disrupt("drift", all_sims=all_sims)
        assert ref.trim(got) == ref.command(snap, "drift", all_sims=all_sims)
    assert c.last_routes[-1]["family"] == "sims_topo"
    assert len(got["command"]["replacements"]) == 2
