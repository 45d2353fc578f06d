"""What tests/test_wide_topology_gpu.py relies on, checked on the CPU with the host-only inspectors and the oracle alone:
every constructed case (tests/wide_topology_cases.py) is in the cell it names, the oracle's answer has the property the
builder promises, and the answer depends on the edge (the same case with the deciding domain at position 1 gets another
answer, which names that domain).  Where the answer has a closed form it is checked against the oracle itself.

Each test prints one line per case id with the cell reached and the domain that decided (pytest -rA / -s shows them).
Nothing is skipped: the inputs are constructed, and test_the_grid_is_complete fails when a required cell has no case."""
import json

import pytest

import disrupt_reference as ref
import wide_topology_cases as w
from karpenter_amd import inspect, inspect_consolidation, synth
from oracle import bridge

FULL = str(w.FULL_BUDGET)
KIND_OF_TARGET = {"claim": "claim", "open": "claim", "node": "node", "unlabelled": "unlabelled", "error": "error"}


def _group_of(dims, key, nv, gtype):
    """The groups of the case's key, width and type: [slot, nv, small, type, host] rows."""
    slot = dims["topologyKeys"].index(key)
    return [g for g in dims["topologyGroups"] if g[0] == slot and g[1] == nv and g[3] == w._base_type(gtype) and not g[4]]


@pytest.mark.parametrize("name", list(w.SOLVE_CASES))
def test_solve_case(name):
    case = w.solve(name)
    key, nv, pos, target = case["key"], case["nv"], case["pos"], case["target"]
    dims = inspect(json.dumps(case["snapshot"]))
    # --- the cell: one non-hostname group of nv domains on the key, in the LDS-resident prefix, one group word
    groups = _group_of(dims, key, nv, case["type"])
    assert groups and all(g[2] == 1 for g in groups), dims["topologyGroups"]
    assert dims["keyValues"][dims["keyNames"].index(key)] == nv
    assert dims["tgSmall"] == dims["tgCntWords"] == nv * dims["G"] and dims["groupWords"] == 1
    assert (key in synth.FAKE_WELL_KNOWN) == (key == w.ZONE)
    pl = dims["plans"][FULL]
    assert pl["tcl"] == dims["tgCntWords"] and pl["tdl"] == dims["TK"] * dims["nodes"]
    assert dims["nodes"] == len(case["snapshot"]["stateNodes"])
    assert dims["unlabelledNodes"] == (1 if target == "unlabelled" else 0)
    # --- the answer: the pod ends in the deciding domain, by the promised route
    res = w.oracle_solve(name)
    kind, dom = w.deciding_domain(case, res)
    assert kind == KIND_OF_TARGET[target], (kind, dom)
    assert dom == case["domain"], (dom, case["domain"])
    if case["domain"]:
        assert case["domain"] == w.names(key, nv)[pos]
    if target == "open":  # the larger unconstrained pod opened the NodeClaim this pod narrowed
        claim = res["newNodeClaims"][w.where(res, case["pod"])[1]]
        assert len(res["newNodeClaims"]) == 1 and sorted(claim["pods"]) == [0, 1]
    if target == "node":
        assert not res["newNodeClaims"] and not res["podErrors"]
    if target == "unlabelled":  # the probes of the other edge domains did not fit the node
        assert len(res["newNodeClaims"]) >= 1 and not res["podErrors"]
    if target == "error":  # the whole wide map is printed
        text = res["podErrors"][str(case["pod"])]
        shown = [d for d in w.names(key, nv) if (d + ":") in text]
        assert "counts = map[" in text and len(shown) == nv, text[:300]  # every registered domain of the group
    # --- the edge decides: the same case with the deciding domain at position 1
    other = w.moved(name)
    moved_to = None
    if other is not None:
        res2, _ = bridge.solve(json.dumps(other["snapshot"]))
        res2.pop("stats", None)
        kind2, moved_to = w.deciding_domain(other, res2)
        assert kind2 == kind and moved_to == other["domain"] != dom
        assert res2 != res
    print("%s: key slot %d of %s, nv %d, %s group small=1, tcl %d tdl %d; %s -> %s (moved: %s)" % (
        name, dims["topologyKeys"].index(key), dims["topologyKeys"], nv, case["type"], pl["tcl"], pl["tdl"], kind, dom,
        moved_to))


def test_min_domains_both_sides_of_the_count():
    """65 eligible domains, summed over two strides: minDomains 64 and 65 leave the minimum at 1 (the pod lands in the
    first zone), 66 makes it 0 (no zone passes) -- so a count of 64 or 66 in place of 65 shows."""
    out = {}
    for m in (64, 65, 66):
        name = "zone-65-minDomains-%d" % m
        case, res = w.solve(name), w.oracle_solve(name)
        assert case["minDomains"] == m and case["nv"] == 65
        out[m] = w.where(res, case["pod"])[0]
    assert out == {64: "claim", 65: "claim", 66: "error"}, out


@pytest.mark.parametrize("kind,nv", w.CLOSED_FORM)
def test_closed_forms(kind, nv):
    """Answers known without the oracle (wide_topology_cases.closed_form_case), which the oracle must give."""
    case = w.closed_form_case(kind, nv)
    res, _ = bridge.solve(json.dumps(case["snapshot"]))
    per = {}
    for c in res["newNodeClaims"]:
        zones = w.claim_values(c, w.ZONE)
        assert zones is not None and len(zones) == 1, c["requirements"]
        per[zones[0]] = per.get(zones[0], 0) + len(c["pods"])
    assert sorted(per) == w.names(w.ZONE, nv)
    if kind == "even":
        assert set(per.values()) == {2} and not res["podErrors"]
    else:  # one pod per zone; the other nv pods fail
        assert set(per.values()) == {1} and len(res["podErrors"]) == nv
        assert all("counts = map[" in e for e in res["podErrors"].values()) or kind == "anti"
    print("closed form %s over %d zones: %d NodeClaims, %d errors" % (kind, nv, len(res["newNodeClaims"]), len(res["podErrors"])))


def test_cluster_node_labels_on_universe_keys_encode():
    """A label-only node (clusterNodes) with a hostname label, under a spread group: countDomains matches the group's node
    filter against all its labels, so their values need ids (ks_host.cpp); such a snapshot used to be refused."""
    case = w.solve("zone-33-spread-p32")
    assert all(w.HOST in n["labels"] for n in case["snapshot"]["clusterNodes"]) and case["snapshot"]["clusterNodes"]
    assert inspect(json.dumps(case["snapshot"]))["G"] == 1


@pytest.mark.parametrize("cell", w.PLAN_CELLS)
def test_solve_plan_cells(cell):
    case = w.plan_case(cell)
    dims = inspect(json.dumps(case["snapshot"]))
    assert dims["tgSmall"] < dims["tgCntWords"] and dims["nodes"] == 8 + w.PLAN_FULL_NODES
    zone_groups = _group_of(dims, w.ZONE, w.PLAN_NV, "spread")
    assert len(zone_groups) == w.PLAN_APPS
    # the groups are created in pod order (app order): the first 15 fill the 2048-word prefix, the rest are outside
    flags = [g[2] for g in dims["topologyGroups"][:w.PLAN_APPS]]
    n_small = 2048 // w.PLAN_NV
    assert flags == [1] * n_small + [0] * (w.PLAN_APPS - n_small) and n_small < w.PLAN_APPS
    assert [g[2] for g in _group_of(dims, w.RACK, 70, "spread")] == [1]
    assert sum(g[1] for g in dims["topologyGroups"] if g[2]) == dims["tgSmall"] > 2048 - w.PLAN_NV
    budget, pl = w.plan_budget(dims, cell)
    assert budget is not None, dims["plans"]
    if cell == "whole-table":
        assert budget == w.FULL_BUDGET and pl["tcl"] == dims["tgCntWords"] and pl["tdl"] == dims["TK"] * dims["nodes"]
    elif cell == "small-prefix":
        assert pl["tcl"] == dims["tgSmall"] and pl["tdl"] == dims["TK"] * dims["nodes"]
    else:
        assert pl["tdl"] == 0 and pl["tcl"] == dims["tgSmall"]
    assert pl["KO"] >= dims["pods"]  # no re-plan for NodeClaim capacity
    # every zone group, the three outside the prefix included, puts its app's pod in the one admissible zone
    res, _ = bridge.solve(json.dumps(case["snapshot"]))
    landed = {"claim": 0, "node": 0}
    zone_of_node = {n["name"]: n["labels"][w.ZONE] for n in case["snapshot"]["stateNodes"]}
    for pod, zone in case["zones"].items():
        kind, at = w.where(res, pod)
        landed[kind] += 1
        got = zone_of_node[at] if kind == "node" else w.claim_values(res["newNodeClaims"][at], w.ZONE)[0]
        assert got == zone, (pod, got, zone)
    assert landed["claim"] >= 3 and landed["node"] >= 3 and not res["podErrors"]
    for pod in list(case["zones"])[n_small:]:
        assert w.where(res, pod)[0] == "claim"
    kind, at = w.where(res, case["rack"][0])
    assert kind == "claim" and w.claim_values(res["newNodeClaims"][at], w.RACK) == [case["rack"][1]]
    print("plan cell %s: budget %d, tcl %d (tgSmall %d of %d count words), tdl %d" % (
        cell, budget, pl["tcl"], dims["tgSmall"], dims["tgCntWords"], pl["tdl"]))


def _sims(doc):
    return [(tuple(x["candidates"]), x["allNonPendingScheduled"], x["newNodeClaims"],
             tuple((x.get("claim0") or {}).get("instanceTypeOptions") or ()))
            for k in ("multi", "single") for x in doc[k]["sims"]]


def _single(doc):
    return {x["candidates"][0]: (x["allNonPendingScheduled"], x["newNodeClaims"]) for x in doc["single"]["sims"]}


def _differ(a, b):
    return sum(1 for x, y in zip(_sims(a), _sims(b)) if x != y) + abs(len(_sims(a)) - len(_sims(b)))


@pytest.mark.parametrize("name", list(w.CONS_CASES))
def test_simulation_case(name):
    case = w.cons(name)
    snap = case["snapshot"]
    dims = inspect_consolidation(json.dumps(snap))
    want = w.oracle_cons(name, True)
    sims = _sims(want)
    assert dims["G"] > 0 and dims["sims"] == len(sims) >= 19
    assert any(s[2] > 0 for s in sims) and any(s[1] for s in sims)
    wide = [g for g in dims["topologyGroups"] if not g[4] and g[1] >= 65]
    assert {g[3] for g in wide} == {w.TG_SPREAD, w.TG_AFFINITY, w.TG_ANTI}
    shown = ""
    if name == "wide-zones":
        assert dims["topologyKeys"] == [w.ZONE] and all(g[1] == 70 for g in wide) and dims["nodes"] <= 10
    if name == "key-slots":
        # the fifth and sixth key slots: their groups decide simulations (without them the oracle answers otherwise)
        assert dims["TK"] == 6 and dims["nodes"] <= 10
        late = set(dims["topologyKeys"][4:])
        assert {g[0] for g in wide} == set(range(6)) and late < set(case["keys"])
        stripped = w.strip_apps(snap, lambda a, spec: bool(w.spec_keys(spec) & late))
        assert inspect_consolidation(json.dumps(stripped))["TK"] == 4
        n = _differ(want, bridge.consolidate(json.dumps(stripped), all_sims=True)[0])
        assert n >= 1
        # and one pod each is pinned to a node by a slot-4 / slot-5 domain alone: without room there, a NodeClaim
        single = _single(want)
        for mover, (receiver, key) in case["movers"].items():
            assert dims["topologyKeys"].index(key) >= 4 and single[mover][1] == 0, (mover, key, single[mover])
        for r, m, key in w.SLOT_PAIRS:
            other = bridge.consolidate(json.dumps(w.sim_key_slots(full=(r,))["snapshot"]), all_sims=True)[0]
            assert _single(other)["node-%05d" % m][1] >= 1
        shown = "key slots 4, 5 = %s decide %d simulations and those of %s" % (sorted(late), n, sorted(case["movers"]))
    if name == "non-small":
        # owned groups 15.. (apps 15-19: pods are dealt the apps in NewTopology's order) are outside the prefix
        assert dims["tgSmall"] < dims["tgCntWords"] and dims["tgSmall"] <= 2048 and dims["nodes"] <= 10
        owned = dims["topologyGroups"][:dims["groupsOwned"]]
        n_small = 2048 // 130
        assert [g[2] for g in owned] == [1] * n_small + [0] * (len(owned) - n_small) and len(owned) == 20
        assert {g[3] for g in owned[n_small:]} == {w.TG_SPREAD, w.TG_AFFINITY, w.TG_ANTI}
        assert dims["simPlan"]["tcl"] == dims["tgSmall"]
        stripped = w.strip_apps(snap, lambda a, spec: a is not None and a >= n_small)
        d2 = inspect_consolidation(json.dumps(stripped))
        assert d2["groupsOwned"] == n_small and all(g[2] for g in d2["topologyGroups"][:n_small])
        n = _differ(want, bridge.consolidate(json.dumps(stripped), all_sims=True)[0])
        assert n >= 1
        shown = "owned groups %d-19 outside the prefix decide %d simulations" % (n_small, n)
    if name == "many-nodes":
        assert dims["nodes"] == w.MANY_NODES > 256 and dims["TK"] == 2
        assert len(snap["candidates"]) <= 24 and sum(1 for c in snap["candidates"] if int(c[5:]) > 256) >= 2
        single = _single(want)
        for mover in case["movers"]:
            assert single[mover] == (True, 0), (mover, single[mover])  # joins the anchor on its receiver
        # each receiver decides its mover's simulation: full, the pod needs a NodeClaim
        for r, m in zip(w.RECEIVERS, w.MOVERS):
            other = bridge.consolidate(json.dumps(w.sim_many_nodes(full=(r,))["snapshot"]), all_sims=True)[0]
            assert _single(other)["node-%05d" % m] == (True, 1)
        shown = "receivers %s decide the simulations of %s" % (list(w.RECEIVERS), sorted(case["movers"]))
    pl = dims["simPlan"]
    assert pl["tdl"] == 0 and pl["tcl"] == dims["tgSmall"]  # a simulation keeps the small prefix only
    print("%s: %d nodes, %d sims, TK %d, tgSmall %d of %d count words, %d wide groups; %s" % (
        name, dims["nodes"], dims["sims"], dims["TK"], dims["tgSmall"], dims["tgCntWords"], len(wide), shown))


def test_drift_case():
    """The first drifted node's two pods need a NodeClaim each: one whose zone set spans three requirement words (all
    70 zones but the two its anti-affinity refuses), one pinned to the last zone (a bit of the third word)."""
    case = w.drift_wide_zones()
    want = ref.command(case["snapshot"], "drift")
    cmd = want["command"]
    assert cmd["action"] == "replace" and cmd["candidates"] == [case["candidate"]] == want["candidates"][:1]
    sets = sorted((w.claim_values(r, w.ZONE) for r in cmd["replacements"]), key=len)
    assert len(sets) == 2 and sets[0] == [case["anchor"]] == [w.names(w.ZONE, 70)[69]]
    assert sets[1] == [z for z in w.names(w.ZONE, 70) if z not in case["refused"]] and len(sets[1]) == 68
    dims = inspect_consolidation(json.dumps(case["snapshot"]))
    assert dims["G"] > 0 and dims["topologyKeys"] == [w.ZONE] and dims["nodes"] == 6
    assert all(g[1] == 70 for g in dims["topologyGroups"])
    print("drift over 70 zones: replacements in %s and in %d zones" % (sets[0], len(sets[1])))


def test_the_grid_is_complete():
    """Part of the grid's definition: every nv x {spread, affinity, anti-affinity} x {first, word
    boundary, lane boundary, last}; every placement target per type; the custom key; minDomains around the count."""
    have = {(c.args[1], c.args[2], c.args[3], c.args[0], (c.args[4:] or ("claim",))[0])
            for c in w.SOLVE_CASES.values() if c.func is w.solve_case}
    for nv in w.NVS:
        for gtype in w.TYPES:
            for pos in w.positions(nv):
                assert (nv, gtype, pos, w.ZONE, "claim") in have, (nv, gtype, pos)
        assert {0, 31, 32, nv - 1} <= set(w.positions(nv)) and (nv <= 64 or {63, 64} <= set(w.positions(nv)))
    for gtype in w.TYPES + ("inverse",):
        for target in w.TARGETS:
            assert any(h[1] == gtype and h[4] == target for h in have), (gtype, target)
        assert any(h[1] == gtype and h[3] == w.RACK for h in have)
    for extra in ("spread-tie", "spread-notin", "affinity-bootstrap"):
        assert any(h[1] == extra for h in have)
    assert {"zone-65-minDomains-%d" % m for m in (64, 65, 66)} <= set(w.SOLVE_CASES)
    assert set(w.CONS_CASES) == {"wide-zones", "key-slots", "non-small", "many-nodes"}
    assert set(w.PLAN_CELLS) == {"whole-table", "small-prefix", "no-node-domains"}
