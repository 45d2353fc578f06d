"""Drift / Expiration commands on the GPU (ks_cons_disrupt: the method's single-candidate simulations, then
k_disrupt_pick's pick and export in one launch) against the Python replay of drift.go / expiration.go over the
oracle (tests/disrupt_reference.py), field for field: the ordered candidates, the command with every replacement
(nodePoolName, instanceTypeOptions, requests, requirements) and the simulations the reference runs.

A simulation keeps no commit log, so the library reports no pods per replacement; the requests (a sum over the
replacement's pods) and the NodeClaim count pin what landed where as far as the command states it."""
import copy
import json
import os
import sys

import pytest

import cons_delta
import disrupt_cases as dc
import disrupt_reference as ref
from karpenter_amd import Consolidator

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_disruption_fixtures as mdf  # noqa: E402

pytestmark = pytest.mark.gpu


def both(snap, method="drift", all_sims=False, handle=None, **kw):
    c = handle or Consolidator(json.dumps(snap))
    got = c.disrupt(method, all_sims=all_sims, **kw)
    want = ref.command(snap, method, all_sims=all_sims)
    assert got["method"] == method
    assert ref.trim(got) == want
    return got, want, c


@pytest.mark.parametrize("k", (0, 1, 2, 70))
def test_new_nodeclaims_of_the_pick(k):
    got, want, _ = both(dc.claims_case(k))
    assert len(got["command"]["replacements"]) == k


def test_seventy_claims_overflow_the_lds_resident_claims():
    """A small LDS budget: most of the 70 NodeClaims live in the HBM-resident claim state."""
    snap = dc.claims_case(70)
    c = Consolidator(json.dumps(snap))
    for budget in range(10 * 1024, 6 * 1024, -512):  # the first budget that no longer holds 70 claims in LDS
        plan = c.disrupt("drift", lds_budget=budget)["plan"]
        if plan["KL"] < 70:
            break
    assert plan["KL"] < 70 <= plan["KO"], (budget, plan)
    got, _, _ = both(snap, handle=c, lds_budget=budget)
    assert got["plan"] == plan and len(got["command"]["replacements"]) == 70


@pytest.mark.parametrize("n_its", (33, 65))
def test_instance_type_words(n_its):
    got, _, _ = both(dc.types_case(n_its))
    assert len(got["command"]["replacements"][0]["instanceTypeOptions"]) > 32 * ((n_its - 1) // 32)


@pytest.mark.parametrize("extra", (False, True), ids=("r3", "r5"))
def test_resource_counts(extra):
    got, _, c = both(dc.resources_case(extra))
    assert c.last_routes[-1]["rt"] == (0 if extra else 3)


@pytest.mark.parametrize("n", (1, 64, 65, 256, 257, 300))
def test_only_the_last_candidate_is_schedulable(n):
    got, want, _ = both(dc.count_case(n, "last"))
    assert got["command"]["candidates"] == [want["candidates"][-1]] and len(got["sims"]) == n


@pytest.mark.parametrize("which", ("first", "none"))
def test_first_and_none_schedulable(which):
    got, _, c = both(dc.count_case(65, which))
    assert got["command"]["action"] == ("replace" if which == "first" else "no-op")
    every, _, _ = both(dc.count_case(65, which), all_sims=True, handle=c)
    assert len(every["sims"]) == 65


@pytest.mark.parametrize("method", ("drift", "expiration"))
@pytest.mark.parametrize("family", ("lean", "selectors", "topology"))
def test_simulation_families(family, method):
    snap = {"lean": lambda: dc.small(seed=31, n=12, n_pending=2), "selectors": dc.selectors_case,
            "topology": dc.topology_case}[family]()
    dc.mark(snap, method, seed=9)
    got, _, c = both(snap, method, all_sims=True)
    assert c.last_routes[-1]["lean"] == (1 if family == "lean" else 0)
    assert ("topo" in c.last_routes[-1]["family"]) == (family == "topology")
    assert len(got["sims"]) == len(got["candidates"]) > 0


@pytest.mark.parametrize("scn", mdf.all_scenarios(), ids=[s["name"] for s in mdf.all_scenarios()])
def test_go_scenarios(scn):
    got, _, _ = both(scn["snapshot"], scn["method"])
    cmd = got["command"]
    assert {"action": cmd["action"], "candidates": cmd["candidates"], "replacements": len(cmd["replacements"])} == scn["expect"]


@pytest.mark.parametrize("method", ("drift", "expiration"))
def test_never_pool_command(method):
    """consolidateAfter Never: still the method's candidates; the expectation is the snapshot's without it."""
    snap = dc.mark(dc.small(seed=33, n=10), method)
    want = ref.command(snap, method)
    got = Consolidator(json.dumps(dc.never_pool(snap))).disrupt(method)
    assert ref.trim(got) == want and want["command"]["candidates"]


def test_updates_then_binary():
    """disrupt after each ks_cons_update, and on a handle loaded from the updated handle's bytes."""
    snap = dc.mark(dc.small(seed=34, n=10, n_pending=2), "drift")
    for n in snap["stateNodes"]:
        dc.fill(n)  # the moved pods need replacements
    c = Consolidator(json.dumps(snap))
    both(snap, handle=c)
    order = ref.candidates(snap, "drift")
    first = next(n for n in snap["stateNodes"] if n["name"] == order[0])
    deltas = [{"deletePods": [first["pods"][0]["metadata"]["uid"]]},
              {"removeNodes": [order[1]]},
              {"bindPods": [{"uid": snap["pendingPods"][0]["metadata"]["uid"], "node": order[2]}]},
              {"deletePods": [p["metadata"]["uid"] for p in first["pods"][1:]]}]
    cur = copy.deepcopy(snap)
    for d in deltas:
        cur = cons_delta.apply_delta(cur, d)
        c.update(d)
        got, _, _ = both(cur, handle=c)
    assert got["command"] == {"action": "delete", "candidates": [order[0]], "replacements": []}  # emptied by the updates
    cur = cons_delta.apply_delta(cur, {"removeNodes": [order[0]]})
    c.update({"removeNodes": [order[0]]})
    got, _, _ = both(cur, handle=c)
    assert got["command"]["action"] == "replace"
    loaded = Consolidator.from_binary(c.save())
    again = loaded.disrupt("drift")
    again.pop("kernel_ms"), got.pop("kernel_ms")
    assert again == got


def test_the_pass_is_undisturbed():
    snap = dc.mark(dc.small(seed=35, n=14, n_pending=2), "drift")
    c = Consolidator(json.dumps(snap))
    before = c.consolidate(all_sims=True)
    routes = c.last_routes
    got = c.disrupt("drift")
    assert got["command"]["candidates"]
    assert c.last_routes[:len(routes)] == routes and len(c.last_routes) > len(routes)
    recs, _ = c.run(0, 1)
    # the handle's pass state (plan, cached sort) is the one from before the call
    after = c.decide(recs, 1, True)
    before.pop("kernel_ms")
    assert after == before
    assert c.last_routes == routes
    again = c.disrupt("drift")  # the method's cached plan
    again.pop("kernel_ms"), got.pop("kernel_ms")
    assert again == got
    # a kept pass (records in the handle) survives the method too
    c.run(0, 1, keep=True)
    c.disrupt("expiration"), c.disrupt("drift")
    assert c.decide(None, 1, True) == before
