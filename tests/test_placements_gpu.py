"""Pods per replacement and exact requests text (ks_cons_disrupt with KS_CONS_PLACEMENTS) and Simulation Results of
one simulation of a pass (ks_cons_sim_results) against the oracle (tests/placements_reference.py), field for field:
pods in commit order as UIDs, the requests text, requirements, options; for sim_results also existingNodes and
unscheduled.  Both re-run one simulation on the k_solve instantiations that store the commit log (SLOG).

The inputs are proven on the CPU by tests/test_placements_inputs.py."""
import copy
import json
import os

import pytest

import cons_delta
import placements_cases as pc
import placements_reference as pref
from karpenter_amd import Consolidator, KsError

pytestmark = pytest.mark.gpu

CT_RUNS, CT_RUN_PODS = 24, 25  # ks_cons_sim_counters_n: runs of identical pods, pods they placed


def log_routes(c):
    return [r for r in c.last_routes if r["family"] in ("sims_log", "sims_topo_log")]


def disrupt_both(name, handle=None, method="drift", **kw):
    """disrupt(placements=True) on the case against its reference; returns (document, reference, handle)."""
    snap = pc.snapshot(name)
    c = handle or Consolidator(json.dumps(snap))
    got = c.disrupt(method, placements=True, **kw)
    want, sim = pc.reference(name, method)
    stated = pref.trim(copy.deepcopy(got))
    for r in stated["command"]["replacements"]:  # (launch_lists: the reference states no launch list)
        r.pop("launchInstanceTypes", None), r.pop("launchPrices", None)
    assert stated == want
    assert got["placements_ms"] > 0 if want["command"]["action"] == "replace" else got["placements_ms"] == 0
    return got, want, c


def candidate_order(c):
    recs, _ = c.run(0, 1)
    return [k["name"] for k in c.decide(recs, 1, all_sims=True)["candidates"]]


def sim_of(c, names, order):
    """The simulation index of the prefix `names` of the candidates' order (one name: that candidate's own)."""
    if len(names) == 1:
        return c.num_sims - c.num_candidates + order.index(names[0])
    assert names == order[:len(names)]
    return c.num_sims - c.num_candidates - (len(names) - 1)


def results_both(c, snap, names, order, **kw):
    sim = sim_of(c, names, order)
    got = c.sim_results(sim, **kw)
    assert got["sim"] == sim and got["kernel_ms"] > 0
    assert pref.trim_results(got) == pref.simulate(snap, names)
    return got, sim


# --- log block edges ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("identical", (False, True), ids=("diff", "same"))
@pytest.mark.parametrize("k", pc.EDGES)
def test_log_block_edges(k, identical):
    name = "edge_%s_%d" % ("same" if identical else "diff", k)
    snap = pc.snapshot(name)
    got, want, c = disrupt_both(name)
    assert sum(len(r["pods"]) for r in got["command"]["replacements"]) == len(
        [u for cl in pc.reference(name)[1]["newNodeClaims"] for u in cl["pods"]])
    assert [(r["family"], r["rt"], r["lean"], r["n"]) for r in log_routes(c)] == [("sims_log", 3, 1, 1)]
    # the same simulation as a pass ran it, through ks_cons_sim_results
    order = candidate_order(c)
    heavy = pc.heavy_name(snap)
    res, sim = results_both(c, snap, [heavy], order)
    assert sum(len(t["pods"]) for t in res["newNodeClaims"] + res["existingNodes"]) == k
    ctr = c.sim_counters(sim)
    if identical and k > 1:  # the pass's simulation took the run path: the pods on existing nodes came in runs
        assert ctr[CT_RUNS] >= 1 and ctr[CT_RUN_PODS] == min(k - 1, sum(pc.RUN_ROOM)), ctr[CT_RUNS:CT_RUN_PODS + 1]
    else:
        assert ctr[CT_RUNS] == 0 and ctr[CT_RUN_PODS] == 0


# --- targets ----------------------------------------------------------------------------------------------------

def test_targets_split_and_unscheduled_pending_pod():
    snap = pc.snapshot("targets")
    got, want, c = disrupt_both("targets")
    assert len(got["command"]["replacements"]) == 2
    order = candidate_order(c)
    res, _ = results_both(c, snap, [pc.heavy_name(snap)], order)
    assert len(res["existingNodes"]) == 2 and len(res["newNodeClaims"]) == 2
    assert res["unscheduled"] == ["pod-uid-000900"] and res["allNonPendingScheduled"] is True


# --- routes -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,family,rt,lean", (("selectors", "sims_log", 3, 0), ("r5", "sims_log", 0, 0),
                                                 ("topology", "sims_topo_log", 3, 0)))
def test_routes(name, family, rt, lean):
    snap = pc.snapshot(name)
    got, want, c = disrupt_both(name)
    assert [(r["family"], r["rt"], r["lean"], r["n"]) for r in log_routes(c)] == [(family, rt, lean, 1)]
    order = candidate_order(c)
    for cand in order[:3]:
        results_both(c, snap, [cand], order)
    assert {r["family"] for r in log_routes(c)} == {family}


def test_small_lds_budget_claims_past_kl():
    """TL off (the instance-type tables in HBM) and most of the 70 NodeClaims in the HBM-resident claim state."""
    c = Consolidator(json.dumps(pc.snapshot("lds")))
    for budget in range(10 * 1024, 6 * 1024, -512):
        plan = c.disrupt("drift", lds_budget=budget)["plan"]
        if plan["KL"] < 70 and c.last_routes[-1]["tl"] == 0:
            break
    assert plan["KL"] < 70 <= plan["KO"] and c.last_routes[-1]["tl"] == 0, (budget, plan, c.last_routes[-1])
    got, want, _ = disrupt_both("lds", handle=c, lds_budget=budget)
    assert len(got["command"]["replacements"]) == 70 and got["plan"] == plan
    assert [(r["family"], r["tl"]) for r in log_routes(c)] == [("sims_log", 0)]


def test_simulation_the_pass_ran_on_four_waves():
    snap = pc.mw_cluster()
    old = {k: os.environ.get(k) for k in ("KS_SIM_MW", "KS_SIM_MW_MIN")}
    os.environ.update({"KS_SIM_MW": "1", "KS_SIM_MW_MIN": "1"})
    try:
        c = Consolidator(json.dumps(snap))
        order = candidate_order(c)
        assert [r["family"] for r in c.last_routes] == ["sims_mixed"] and c.last_routes[0]["nmw"] == c.num_sims
        res, _ = results_both(c, snap, order[:1], order)  # re-run single-wave
        results_both(c, snap, order[:2], order)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert [(r["family"], r["n"]) for r in log_routes(c)] == [("sims_log", 1)] * 2


def test_multi_node_prefix_of_two():
    snap = pc.pass_cluster()
    c = Consolidator(json.dumps(snap))
    order = candidate_order(c)
    res, sim = results_both(c, snap, order[:2], order)
    assert res["candidates"] == order[:2] and sim < c.num_sims - c.num_candidates


# --- requests text ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", pc.TEXT_KINDS)
def test_requests_text(kind):
    name = "text_" + kind
    got, want, c = disrupt_both(name)
    resource, _ = pc.TEXT_MIX[kind]
    assert got["command"]["replacements"][0]["requests"][resource] == pc.TEXT_WANT[kind]
    with pytest.raises(KsError) as e:  # the same call without the flag still refuses
        c.disrupt("drift")
    assert e.value.code == -2 and "KS_CONS_PLACEMENTS" in str(e.value)
    fresh = Consolidator(json.dumps(pc.snapshot(name)))
    with pytest.raises(KsError) as e:
        fresh.disrupt("drift")
    assert e.value.code == -2


# --- calls that launch nothing extra ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("delete_empty", "delete_pick", "noop"))
def test_no_replacement_launches_nothing_extra(name):
    got, want, c = disrupt_both(name)
    assert got["placements_ms"] == 0 and log_routes(c) == []
    plain = c.disrupt("drift")
    got.pop("placements_ms")
    got.pop("kernel_ms"), plain.pop("kernel_ms")
    assert got == plain


# --- combination and state ----------------------------------------------------------------------------------------

def test_placements_with_launch_lists():
    c = Consolidator(json.dumps(pc.snapshot("targets")))
    lists = c.disrupt("drift", launch_lists=True)
    both, want, _ = disrupt_both("targets", handle=c, launch_lists=True)
    assert len(both["command"]["replacements"]) == 2
    for a, b in zip(both["command"]["replacements"], lists["command"]["replacements"]):
        assert a["launchInstanceTypes"] == b["launchInstanceTypes"] and a["launchPrices"] == b["launchPrices"]
        assert {k: v for k, v in a.items() if k != "pods"} == b
    assert c.disrupt_launch(1)[0] == both["command"]["replacements"][1]["launchInstanceTypes"]


def test_without_the_flag_the_document_is_unchanged():
    c = Consolidator(json.dumps(pc.snapshot("targets")))
    plain = c.disrupt("drift")
    assert "placements_ms" not in plain and all("pods" not in r for r in plain["command"]["replacements"])
    got = c.disrupt("drift", placements=True)
    assert list(got)[-2:] == ["placements_ms", "kernel_ms"]
    for r in got["command"]["replacements"]:
        r.pop("pods")
    got.pop("placements_ms")
    got.pop("kernel_ms"), plain.pop("kernel_ms")
    assert got == plain


def test_after_updates_and_from_binary():
    snap = pc.snapshot("updates")
    c = Consolidator(json.dumps(snap))
    got, want, _ = disrupt_both("updates", handle=c)
    first = next(n for n in snap["stateNodes"] if n["name"] == want["candidates"][0])
    deltas = [{"deletePods": [first["pods"][0]["metadata"]["uid"]]},
              {"removeNodes": [want["candidates"][1]]},
              {"bindPods": [{"uid": snap["pendingPods"][0]["metadata"]["uid"], "node": want["candidates"][2]}]}]
    cur = copy.deepcopy(snap)
    for d in deltas:
        cur = cons_delta.apply_delta(cur, d)
        c.update(d)
        got = c.disrupt("drift", placements=True)
        want_cur, _ = pref.command(cur, "drift")
        assert pref.trim(got) == want_cur and got["command"]["action"] == "replace"
    loaded = Consolidator.from_binary(c.save())
    again = loaded.disrupt("drift", placements=True)
    for doc in (again, got):
        doc.pop("kernel_ms"), doc.pop("placements_ms")
    assert again == got
    # sim_results on the loaded handle
    order = candidate_order(loaded)
    results_both(loaded, cur, order[:1], order)


def test_the_pass_is_undisturbed():
    snap = pc.snapshot("updates")
    c = Consolidator(json.dumps(snap))
    recs, _ = c.run(0, 1)
    before = bytes(recs)
    decided = c.decide(recs, 1, all_sims=True)
    order = [k["name"] for k in decided["candidates"]]
    routes = c.last_routes
    results_both(c, snap, order[:1], order)
    results_both(c, snap, order[:2], order)
    assert c.disrupt("drift", placements=True)["command"]["action"] == "replace"
    assert c.last_routes[:len(routes)] == routes
    assert c.decide(recs, 1, all_sims=True) == decided  # the handle's records and plan are the pass's
    recs, _ = c.run(0, 1)
    assert bytes(recs) == before and c.last_routes == routes


def test_sim_results_argument_errors():
    snap = pc.pass_cluster()
    c = Consolidator(json.dumps(snap))

    def refused(sim):
        with pytest.raises(KsError) as e:
            c.sim_results(sim)
        assert e.value.code == -6
        return True

    assert refused(0)  # before the first run
    c.run(0, 1)
    assert c.sim_results(0)["sim"] == 0
    assert refused(-1) and refused(c.num_sims)  # out of range
    first = snap["stateNodes"][0]["pods"][0]["metadata"]["uid"]
    c.update({"deletePods": [first]})
    assert refused(0)  # after an update, until the next run
    c.run(0, 2)
    assert c.sim_results(0)["sim"] == 0 and c.sim_results(2)["sim"] == 2
    assert refused(1)  # the other rank's simulation
