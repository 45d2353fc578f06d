"""Drift / Expiration on the host (no GPU): the method's candidates and order (ks_cons_inspect_disrupt) against
the Python replay of drift.go / expiration.go over the oracle (tests/disrupt_reference.py), the transcribed Go
scenarios, binary snapshots, ks_cons_update, and the preconditions of the GPU cases."""
import copy
import json
import os
import sys

import pytest

import cons_delta
import disrupt_cases as dc
import disrupt_reference as ref
from karpenter_amd import (encode_consolidation_binary, inspect_disruption, inspect_disruption_binary, synth)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_disruption_fixtures as mdf  # noqa: E402

METHODS = ("drift", "expiration")


def check(snap, method):
    """The library's candidates (and empties) equal the reference's; returns them."""
    got = inspect_disruption(json.dumps(snap), method)
    want = ref.candidates(snap, method)
    assert got["candidates"] == want
    by = {n["name"]: n for n in snap["stateNodes"]}
    assert got["empty"] == [n for n in want if not [p for p in by[n]["pods"] if ref.reschedulable(p)]]
    return want


@pytest.mark.parametrize("method", METHODS)
def test_every_node_marked(method):
    want = check(dc.mark(dc.small(), method), method)
    assert len(want) == 14 and want != sorted(want)  # all of them, in transition-time order


@pytest.mark.parametrize("method", METHODS)
def test_no_condition_and_status_false(method):
    snap = dc.small()
    assert check(snap, method) == []
    other = "expiration" if method == "drift" else "drift"
    assert check(dc.mark(copy.deepcopy(snap), other), method) == []  # the other method's condition only
    assert check(dc.mark(copy.deepcopy(snap), method, status="False"), method) == []
    half = [n["name"] for n in snap["stateNodes"][::2]]
    assert sorted(check(dc.mark(copy.deepcopy(snap), method, names=half), method)) == half


def test_gate_off():
    snap = dc.mark(dc.small(), "drift")
    snap["featureGates"] = {"drift": False}
    assert check(snap, "drift") == []
    snap["featureGates"] = {"drift": True}
    assert len(check(snap, "drift")) == 14
    # the gate is Drift's alone
    exp = dc.mark(dc.small(), "expiration")
    exp["featureGates"] = {"drift": False}
    assert len(check(exp, "expiration")) == 14


@pytest.mark.parametrize("method", METHODS)
def test_blocked_nodes(method):
    """do-not-disrupt node, do-not-disrupt / do-not-evict pod, nominated node, PDB-blocked pods."""
    snap = dc.mark(dc.small(pdbs=True, n=20), method)
    nodes = snap["stateNodes"]
    nodes[0]["annotations"] = {"karpenter.sh/do-not-disrupt": "true"}
    nodes[1]["pods"][0]["metadata"].setdefault("annotations", {})["karpenter.sh/do-not-disrupt"] = "true"
    nodes[2]["pods"][0]["metadata"].setdefault("annotations", {})["karpenter.sh/do-not-evict"] = "true"
    nodes[3]["nominated"] = True
    want = check(snap, method)
    assert not {n["name"] for n in nodes[:4]} & set(want)
    plain = ref.candidates(dc.mark(dc.small(n=20), method), method)
    assert 0 < len(want) < len(plain) - 4  # the budgets block more


def test_expire_after_never():
    snap = dc.mark(dc.small(), "expiration")
    for key in ("nodePools", "nodeClaimTemplates"):
        snap[key][0]["spec"]["disruption"]["expireAfter"] = "Never"
    assert check(snap, "expiration") == []
    assert len(check(dc.mark(snap, "drift"), "drift")) == 14  # Drift does not read expireAfter


@pytest.mark.parametrize("method", METHODS)
def test_tie_is_stable_up_to_twelve(method):
    snap = dc.mark(dc.small(n=12), method, tie=True)
    assert check(snap, method) == snap["candidates"]


@pytest.mark.parametrize("method", METHODS)
def test_empty_candidates(method):
    snap = dc.mark(dc.small(), method)
    for n in snap["stateNodes"][3:9:2]:
        n["pods"] = []
    got = inspect_disruption(json.dumps(snap), method)
    check(snap, method)
    assert len(got["empty"]) == 3
    assert ref.command(snap, method)["command"] == {"action": "delete", "candidates": got["empty"], "replacements": []}


@pytest.mark.parametrize("method", METHODS)
def test_never_pool_is_still_a_candidate(method):
    """consolidateAfter Never is consolidation's ShouldDisrupt, not Drift's or Expiration's."""
    snap = dc.mark(dc.small(), method)
    want = ref.candidates(snap, method)
    assert len(want) == 14
    assert inspect_disruption(json.dumps(dc.never_pool(snap)), method)["candidates"] == want


def test_do_not_consolidate_node_is_still_a_candidate():
    snap = dc.mark(dc.small(), "drift")
    want = ref.candidates(snap, "drift")
    snap["stateNodes"][5]["annotations"] = {"karpenter.sh/do-not-consolidate": "true"}
    assert inspect_disruption(json.dumps(snap), "drift")["candidates"] == want


@pytest.mark.parametrize("method", METHODS)
def test_cluster_form(method):
    """The "cluster" listings in place of "stateNodes": the conditions come from the paired NodeClaim."""
    import test_cluster_state as tcs

    with_state, with_cluster = tcs._cons_inputs(5)
    kind = dc.KIND[method]
    claims = with_cluster["cluster"]["nodeClaims"]
    by_id = {}
    for k, nc in enumerate(claims):
        conds = [{"type": kind, "status": "True" if k % 4 else "False",
                  "lastTransitionTime": synth._fmt_time(synth.NOW - 5000 + 13 * ((k * 5) % len(claims)))}]
        nc.setdefault("status", {})["conditions"] = conds
        by_id[nc["status"].get("providerID")] = conds
    for n in with_state["stateNodes"]:
        if by_id.get(n.get("providerID")):
            n["nodeClaimConditions"] = by_id[n["providerID"]]
    for s in (with_state, with_cluster):
        for key in ("nodePools", "nodeClaimTemplates"):
            s[key][0]["spec"]["disruption"]["expireAfter"] = "720h"
    want = ref.candidates(with_state, method)
    assert want
    assert inspect_disruption(json.dumps(with_cluster), method)["candidates"] == want
    assert inspect_disruption(json.dumps(with_state), method)["candidates"] == want


# ---- transcribed Go scenarios ------------------------------------------------------------------------
SCENARIOS = mdf.all_scenarios()
with open(os.path.join(HERE, "golden", "disruption_scenarios.json")) as f:
    FIXTURES = json.load(f)


def test_fixture_file_matches_generator():
    assert FIXTURES == json.loads(json.dumps(
        [{"name": s["name"], "method": s["method"], "source": s["source"], "expect": s["expect"]} for s in SCENARIOS]))
    assert len(FIXTURES) == 23


@pytest.mark.parametrize("scn", SCENARIOS, ids=[s["name"] for s in SCENARIOS])
def test_go_scenarios_pin_the_reference(scn):
    """The Go test's expected command equals the Python reference's; the library's candidates equal its."""
    want = ref.command(scn["snapshot"], scn["method"])
    cmd = want["command"]
    assert {"action": cmd["action"], "candidates": cmd["candidates"], "replacements": len(cmd["replacements"])} == scn["expect"]
    got = inspect_disruption(json.dumps(scn["snapshot"]), scn["method"])
    assert got["candidates"] == want["candidates"]


# ---- binary snapshots --------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_binary_round_trip(method):
    snap = dc.mark(dc.small(), method)
    snap["featureGates"] = {"drift": True}
    for n in snap["stateNodes"][2:5]:
        n["pods"] = []
    blob = encode_consolidation_binary(json.dumps(snap))
    doc, again = inspect_disruption_binary(blob, method)
    assert again == blob  # save -> load -> save
    assert doc == inspect_disruption(json.dumps(snap), method) and doc["candidates"] and doc["empty"]
    off = dict(snap, featureGates={"drift": False})
    doc, _ = inspect_disruption_binary(encode_consolidation_binary(json.dumps(off)), "drift")
    assert doc["candidates"] == []  # the gate travels with the handle
    bare = dc.small()
    doc, _ = inspect_disruption_binary(encode_consolidation_binary(json.dumps(bare)), method)
    assert doc["candidates"] == []  # no fields: as before


# ---- ks_cons_update ----------------------------------------------------------------------------------
def test_after_updates_equals_a_fresh_build():
    snap = dc.mark(dc.small(n_pending=2), "drift")
    order = ref.candidates(snap, "drift")
    first = next(n for n in snap["stateNodes"] if n["name"] == order[0])
    deltas = [{"deletePods": [p["metadata"]["uid"] for p in first["pods"]]},
              {"bindPods": [{"uid": snap["pendingPods"][0]["metadata"]["uid"], "node": order[1]}]},
              {"removeNodes": [order[2]]}]
    cur = copy.deepcopy(snap)
    for k, d in enumerate(deltas):
        cur = cons_delta.apply_delta(cur, d)
        got = inspect_disruption(json.dumps(snap), "drift", deltas[:k + 1])
        assert got == inspect_disruption(json.dumps(cur), "drift")
        assert got["candidates"] == ref.candidates(cur, "drift")
    assert got["empty"] == [order[0]] and order[2] not in got["candidates"]


# ---- preconditions of the GPU cases ------------------------------------------------------------------
@pytest.mark.parametrize("k", (0, 1, 2, 70))
def test_claims_cases_yield_their_claims(k):
    want = ref.command(dc.claims_case(k), "drift")
    assert len(want["command"]["replacements"]) == k
    assert want["command"]["action"] == ("replace" if k else "delete")
    assert want["sims"][0]["candidate"] == want["command"]["candidates"][0]  # the first candidate is the pick


@pytest.mark.parametrize("n_its,words", ((33, 2), (65, 3)))
def test_types_cases_span_words(n_its, words):
    want = ref.command(dc.types_case(n_its), "drift")
    (rep,) = want["command"]["replacements"]
    assert (len(rep["instanceTypeOptions"]) + 31) // 32 == words


def test_resources_cases():
    for extra, r in ((False, 3), (True, 5)):
        (rep,) = ref.command(dc.resources_case(extra), "drift")["command"]["replacements"]
        assert len(rep["requests"]) == r


@pytest.mark.parametrize("which", ("last", "first", "none"))
def test_count_cases_pick_where_they_say(which):
    snap = dc.count_case(65, which)
    want = ref.command(snap, "drift")
    order = want["candidates"]
    assert len(order) == 65
    ok = [s["candidate"] for s in want["sims"] if s["allNonPendingScheduled"]]
    assert ok == {"last": [order[-1]], "first": [order[0]], "none": []}[which]
    assert len(want["sims"]) == {"last": 65, "first": 1, "none": 65}[which]
    assert want["command"]["action"] == ("no-op" if which == "none" else "replace")
