"""The NodeClaim-capacity re-plan ladder on the CPU (no GPU): the plans of make_plan's wideKO levels as
ks_problem_inspect reports them ("plans": level 0, "widePlans": levels 1 and 2), and what
tests/test_claim_cap_replan_gpu.py relies on, checked with the oracle and inspect alone.

A wide plan gives 64 claims their LDS state and the rest of the LDS to claim positions, where the default plan gives
half the LDS to positions: KO(wide) = (avail - min(64, kAll) * clmB) / posB against max(kAll, avail / 2 / posB).  When
the LDS holds fewer than about 128 claims' state the wide plan holds fewer positions than the default one (level 2
regains some by moving the instance-type tables to HBM), so a level is not always a step up; ks_solve launches only
the levels that raise KO (replan_cases.ladder restates that from the capacities).  The preconditions pin every GPU
case to the regime it names, so that a change of a generator or of the planner fails here before a case goes
vacuous."""
import json

import pytest

import problems
import replan_cases as rp
from karpenter_amd import inspect

FULL_BUDGET = 160 * 1024 - 256
BUDGETS = [FULL_BUDGET, 6000, 9000, 14000, 24000, 40000]

# the case table's problems and the generators the ladder was first tabulated on
GENERATORS = {
    "lean-r3": lambda: rp.lean_base(300),
    "random-r4": lambda: rp.random_base(500),
    "random-topology": lambda: problems.random_problem(203, n_pods=400, n_its=30, n_nodes=5, topology=True),
}
PROBLEMS = rp.NAMES + sorted(GENERATORS)

_docs = {}


def _inspect(name):
    if name not in _docs:
        _docs[name] = inspect(rp.snapshot(name) if name in rp.CASES else json.dumps(GENERATORS[name]()))
    return _docs[name]


@pytest.mark.parametrize("name", PROBLEMS)
def test_plans_of_every_level(name):
    doc = _inspect(name)
    assert sorted(doc["plans"]) == sorted(doc["widePlans"]) == sorted(str(b) for b in BUDGETS)
    for budget in BUDGETS:
        lv = rp.levels(doc, budget)
        assert len(lv) == 3 and all(set(pl) == set(lv[0]) for pl in lv)
        for level, pl in enumerate(lv):
            where = (name, budget, level, pl)
            if pl["KO"] < 1:
                continue
            assert pl["lds"] <= budget, where
            assert 1 <= pl["KL"] <= pl["KO"] <= doc["Kcap"], where
            if level:
                assert pl["KL"] <= 64 or pl["KO"] == pl["KL"] == doc["Kcap"], where
            if level == 2:
                assert pl["talloc"] == 0, where
            if pl["talloc"]:
                assert lv[0]["talloc"] == 1, where


def test_the_listed_budgets_cover_both_orders():
    """The ladder's two shapes are both in the table: every level a step up, and wide plans below the default."""
    k = rp.ks("lean-K0")
    assert k[0] < k[1] < k[2]
    k = rp.ks("lean-no-raise")
    assert k[1] < k[0] and k[2] < k[0]
    k = rp.ks("rt4-skip-1")
    assert k[1] < k[0] < k[2]


@pytest.mark.parametrize("name", rp.NAMES)
def test_case_is_in_its_regime(name):
    case = rp.CASES[name]
    doc = _inspect(name)
    lv = rp.levels(doc, case["budget"])
    k = rp.ks(name)
    assert tuple(pl["KO"] for pl in lv) == k, "the case's own plans are not its shape's"
    assert doc["lean"] == case["lean"] and (doc["G"] > 0) == case["topo"]
    assert doc["pods"] <= 500
    want, _ = rp.oracle(name)
    claims = len(want["newNodeClaims"])
    lo, hi = case["regime"]
    assert (lo is None or claims > k[lo]) and (hi is None or claims <= k[hi]), (claims, k)
    if case["claims"] is not None:
        assert claims == case["claims"]
    assert bool(want["podErrors"]) == case["errors"]
    # the launches the capacities imply are the case's (a lean exit adds its non-lean launch at the same level)
    launched, fits = rp.ladder(k, claims)
    assert fits == (case["error"] is None)
    assert launched[-1] == case["wide"] and doc["Kcap"] > k[launched[-1]]
    if case["error"] is not None:
        assert k[case["error"]] == max(k[level] for level in launched) == k[launched[-1]] < claims
    cells = [c for i, c in enumerate(case["cells"]) if i == 0 or c != rp.X]
    assert len(cells) == len(launched)
    R = doc["R"]
    for (fam, rt, tl, lean), level in zip(cells, launched):
        assert fam == (rp.T if case["topo"] else rp.S) and rt == (R if R in (3, 4) else 0)
        assert tl == lv[level]["talloc"] and lean == (1 if case["lean"] and tl else 0)
    if rp.X in case["cells"][1:]:  # the instantiation a lean problem leaves to: same plan, tables in LDS
        assert case["lean"] and case["errors"] and lv[launched[-1]]["talloc"] == 1 and case["cells"][-1] == rp.X


def test_runs_case_fills_a_claim_in_one_run():
    """lean-runs: the run's pods are the first NodeClaim's, in NewQueue's order, and past the 64-pod window."""
    want, _ = rp.oracle("lean-runs")
    snap = json.loads(rp.snapshot("lean-runs"))
    by_size = [c for c in want["newNodeClaims"] if len(c["pods"]) == rp.RUN_PODS]
    assert len(by_size) == 1 and rp.RUN_PODS > 64 + 2
    names = [snap["pods"][i]["metadata"]["name"] for i in by_size[0]["pods"]]
    assert names == sorted(names) and all(n.startswith("pod-1000") for n in names)
    same = [p for p in snap["pods"] if p["spec"]["containers"][0]["resources"]["requests"] == {"cpu": "4000m", "memory": "512Mi"}]
    assert len(same) >= 60
