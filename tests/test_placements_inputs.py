"""The inputs of the placement tests, proven where there is no GPU: the reference helper (tests/placements_reference.py)
runs on every case tests/test_placements_gpu.py uses, and each case is what it claims to be: the stated action, the
mixed formats on one NodeClaim, the commit counts at the log block's edges."""
import json

import pytest

import placements_cases as pc
import placements_reference as pref
from oracle import bridge


@pytest.mark.parametrize("name", sorted(pc.BUILDERS))
def test_case_yields_the_stated_action(name):
    want, sim = pc.reference(name)
    cmd = want["command"]
    assert cmd["action"] == pc.ACTION.get(name, "replace")
    if cmd["action"] == "replace":
        assert sim["allNonPendingScheduled"] and cmd["replacements"] == sim["newNodeClaims"]
        for claim in cmd["replacements"]:
            assert claim["pods"] and len(set(claim["pods"])) == len(claim["pods"])
    else:
        assert cmd["replacements"] == []


@pytest.mark.parametrize("identical", (False, True), ids=("diff", "same"))
@pytest.mark.parametrize("k", pc.EDGES)
def test_edge_cases_commit_exactly_k(k, identical):
    name = "edge_%s_%d" % ("same" if identical else "diff", k)
    snap = pc.snapshot(name)
    want, sim = pc.reference(name)
    assert want["command"]["candidates"] == [pc.heavy_name(snap)] and not snap["pendingPods"]
    placed = [u for c in sim["newNodeClaims"] for u in c["pods"]] + [u for n in sim["existingNodes"] for u in n["pods"]]
    assert len(placed) == k and sim["unscheduled"] == []
    by = pc.pods_by_uid(snap)
    cpus = [by[u]["spec"]["containers"][0]["resources"]["requests"]["cpu"] for u in placed]
    assert cpus[0] == "8" and sim["newNodeClaims"][0]["pods"][0] == placed[0]  # the pod no node holds: a replace
    cpus, k = cpus[1:], k - 1
    if identical:
        assert len(set(cpus)) <= 1
        # first fit: 70 on the first node with room (a run longer than the 64-pod window), 10 on the next, the
        # rest on one NodeClaim
        on_nodes = [len(n["pods"]) for n in sim["existingNodes"]]
        assert on_nodes == [r for r in (min(k, 70), min(max(k - 70, 0), 10)) if r]
        assert [len(c["pods"]) for c in sim["newNodeClaims"]] == [1 + max(k - 80, 0)]
    else:
        assert len(set(cpus)) == k


@pytest.mark.parametrize("kind", pc.TEXT_KINDS)
def test_text_cases_mix_formats_on_one_nodeclaim(kind):
    snap = pc.snapshot("text_" + kind)
    want, sim = pc.reference("text_" + kind)
    assert len(sim["newNodeClaims"]) == 1
    resource, texts = pc.TEXT_MIX[kind]
    assert pref.formats_on(sim["newNodeClaims"][0]["pods"], pc.pods_by_uid(snap), resource) == texts
    assert sim["newNodeClaims"][0]["requests"][resource] == pc.TEXT_WANT[kind]


def test_targets_case_splits_the_pods():
    want, sim = pc.reference("targets")
    assert len(sim["newNodeClaims"]) == 2 and len(sim["existingNodes"]) == 2
    assert sim["unscheduled"] == ["pod-uid-000900"] and sim["allNonPendingScheduled"]


def test_pass_cluster_prefix_of_two():
    snap = pc.pass_cluster()
    doc, _ = bridge.consolidate(json.dumps(snap), all_sims=True)
    names = [c["name"] for c in doc["candidates"]]
    assert len(names) >= 3
    two = pref.simulate(snap, names[:2])
    one = pref.simulate(snap, names[:1])
    pending = {p["metadata"]["uid"] for p in snap["pendingPods"]}
    moved = lambda s: {u for c in s["newNodeClaims"] for u in c["pods"]} | {u for n in s["existingNodes"] for u in n["pods"]}
    assert len(moved(two) - pending) > len(moved(one) - pending) > 0


def test_mw_cluster_reference():
    snap = pc.mw_cluster()
    doc, _ = bridge.consolidate(json.dumps(snap), all_sims=True)
    names = [c["name"] for c in doc["candidates"]]
    sim = pref.simulate(snap, names[:1])
    assert sim["candidates"] == names[:1] and (sim["newNodeClaims"] or sim["existingNodes"])
