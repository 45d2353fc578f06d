"""Launch lists of disruption commands on the GPU (k_launch_lists_sims behind a consolidation pass,
k_launch_lists_export behind a Drift / Expiration pick) against the oracle (tests/launch_cmd_cases.py): names and
prices equal, the prices as exact doubles.  Every case first asserts on the oracle's document that it exercises what
it claims, so a case that stops reaching its edge fails instead of passing vacuously."""
import copy
import json
import os

import pytest

import cons_delta
import disrupt_cases as dc
import launch_cases as lc
import launch_cmd_cases as cc
from karpenter_amd import Consolidator, synth
from karpenter_amd.scheduler import KsError

pytestmark = pytest.mark.gpu

KS_ERR_UNSUPPORTED, KS_ERR_ARG = -2, -6


def narrowed(replacement):
    return (synth.CT + " In [spot]") in replacement["requirements"]


def check_command(snap, c, got, want, world1=True):
    """One command of a decide document against the oracle's: unchanged but for the added keys, and its launch list
    (in the document, and through claim_launch on the owner) equal to the reference."""
    assert cc.strip_added(got) == want
    if want["action"] != "replace":
        assert "sim" not in got
        return None
    names, prices, nopt = cc.expected_launch(snap, want["replacement"])
    rep = got["replacement"]
    if world1 or got["sim"] < 0:
        assert rep["launchInstanceTypes"] == names and rep["launchPrices"] == prices
    if got["sim"] >= 0 and world1:
        assert c.claim_launch(got["sim"]) == (names, prices, nopt)
    return names, prices, nopt


def consolidate(snap, key, **kw):
    want = cc.oracle_consolidate(key, snap)
    c = Consolidator(json.dumps(snap))
    got = c.consolidate(launch_lists=True, **kw)
    got.pop("kernel_ms")
    assert cc.strip_added(got) == want
    lists = {m: check_command(snap, c, got[m]["command"], want[m]["command"]) for m in ("multi", "single")}
    return c, got, want, lists


@pytest.mark.parametrize("name", [n for n in cc.CONS_CASES if n not in ("mw",)])
def test_consolidation_commands(name):
    builder, props = cc.CONS_CASES[name]
    snap = builder()
    want = cc.oracle_consolidate(name, snap)
    multi = want["multi"]["command"]
    assert multi["action"] == "replace" and len(multi["candidates"]) > 1 and narrowed(multi["replacement"])
    if "multi" in props:
        assert len(multi["replacement"]["instanceTypeOptions"]) == props["multi"]
    if name == "flip":  # the narrowed order is not the order under the claim's own requirements
        rep = multi["replacement"]
        assert cc.order_options(snap, rep["instanceTypeOptions"], cc.unnarrowed(rep["requirements"]))[0] != \
            cc.expected_launch(snap, rep)[0]
    if name == "single":
        single = want["single"]
        assert single["command"]["action"] == "replace" and len(single["command"]["candidates"]) == 1
        sim = next(s for s in single["sims"] if s["action"] == "replace")
        assert set(sim["priceOptions"]) < set(sim["claim0"]["instanceTypeOptions"])
    if name == "two-templates":
        assert multi["replacement"]["nodePoolName"] == "default" and snap["nodeClaimTemplates"][1]["metadata"]["name"] == "default"
    c, got, _, _ = consolidate(snap, name)
    assert c.launch_ms() > 0
    if name == "topology":  # a two-phase launch: the long prefixes, then the single-node simulations on another stream
        assert len(c.last_routes) >= 2 and all("topo" in r["family"] for r in c.last_routes[:2])
    # the multi-node probe's options after filterByPrice and after filterOutSameType differ: the wrong block would show
    probe = got["multi"]["path"][-1] if got["multi"]["path"][-1]["action"] == "replace" else None
    if name.startswith("cut-"):
        assert probe and probe["sameTypeOptions"] and set(probe["sameTypeOptions"]) < set(probe["priceOptions"])


def test_mixed_launch_routes():
    """A pass whose simulations run as one sims_mixed launch (tests/test_cons_mw_gpu.py's shape and switches)."""
    snap = cc.mw_case()
    env = {"KS_SIM_MW": "1", "KS_SIM_MW_MIN": "1"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c, got, want, _ = consolidate(snap, "mw")
        routes = c.last_routes
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert want["multi"]["command"]["action"] == "replace"
    assert routes[0]["family"] in ("sims_mixed", "sims_mw")


@pytest.mark.parametrize("kind", cc.CARRIED_KINDS)
def test_carried_probe(kind):
    snap = cc.carried_case(kind)
    want = cc.oracle_consolidate("carried-" + kind, snap)
    cmd = want["multi"]["command"]
    assert cmd["action"] == "replace" and cmd["candidates"] == ["cand-0", "cand-1"] and narrowed(cmd["replacement"])
    assert want["multi"]["path"][1]["carried"] and want["multi"]["path"][1]["mid"] == 1
    names, prices, _ = cc.expected_launch(snap, cmd["replacement"])
    assert prices[0] == 0.05 and len(set(prices)) < len(prices)
    assert cc.order_options(snap, cmd["replacement"]["instanceTypeOptions"], cc.unnarrowed(cmd["replacement"]["requirements"]))[0] != names
    c, got, _, _ = consolidate(snap, "carried-" + kind)
    assert got["multi"]["command"]["sim"] == -1 and c.last_reruns >= 1
    # world 2 on one GPU: the carried probe's list is local, whoever owns the pass's simulations
    ranks = [Consolidator(json.dumps(snap)) for _ in range(2)]
    recs = b"".join(bytes(ranks[r].run(r, 2, launch_lists=True)[0]) for r in range(2))
    doc = ranks[0].decide(recs, 2, fetch=lambda s: ranks[s % 2].claim_requirements(s))
    assert cc.strip_added(doc) == want
    check_command(snap, ranks[0], doc["multi"]["command"], cmd, world1=False)
    assert doc["multi"]["command"]["replacement"]["launchPrices"] == prices


def test_slots_are_not_simulations():
    """rank 1 of world 2: slot k holds simulation 2k + 1."""
    snap = cc.single_case()
    c, got, want, lists = consolidate(snap, "single")
    sims = {m: got[m]["command"]["sim"] for m in ("multi", "single")}
    odd = [m for m in sims if sims[m] % 2 == 1]
    assert odd, sims
    r1 = Consolidator(json.dumps(snap))
    r1.run(1, 2, launch_lists=True)
    for m in odd:
        assert r1.claim_launch(sims[m]) == lists[m]
    with pytest.raises(KsError) as e:
        r1.claim_launch(sims[odd[0]] - 1)
    assert e.value.code == KS_ERR_ARG


def test_other_actions_and_the_flag_off():
    snap = cc.cut_case(33)
    c, got, want, _ = consolidate(snap, "cut-33")
    deleted = c.num_sims - 1  # the last single-node simulation: a delete
    assert want["single"]["command"]["action"] == "delete"
    with pytest.raises(KsError) as e:
        c.claim_launch(deleted)
    assert e.value.code == KS_ERR_ARG
    c.run(0, 1)  # the flag off: no rows
    assert c.launch_ms() == 0
    with pytest.raises(KsError) as e:
        c.claim_launch(got["multi"]["command"]["sim"])
    assert e.value.code == KS_ERR_ARG


def written(records, record_bytes):
    """The records' bytes with the words no kernel writes cleared (they hold whatever the device allocation held):
    the three between RF_CLAIM and RF_HDR (words 13 .. 15), and RF_CLAIM (word 12) of a simulation without a
    NodeClaim (RF_NCLAIMS, word 1, is 0), which the SIM epilogue stores only for NewNodeClaims[0]."""
    out = bytearray(records)
    for at in range(0, len(out), record_bytes):
        out[at + 52:at + 64] = bytes(12)
        if out[at + 4:at + 8] == bytes(4):
            out[at + 48:at + 52] = bytes(4)
    return bytes(out)


@pytest.mark.parametrize("name", ("cut-33", "topology"))
def test_nothing_changes_when_off(name):
    snap = cc.CONS_CASES[name][0]()
    a, b = Consolidator(json.dumps(snap)), Consolidator(json.dumps(snap))
    ra = written(a.run(0, 1, launch_lists=True)[0], a.record_bytes)
    on = a.decide(ra, 1, True)
    routes_on = a.last_routes
    ra_off = written(a.run(0, 1)[0], a.record_bytes)
    routes_off = a.last_routes
    rb = written(b.run(0, 1)[0], b.record_bytes)
    assert ra == ra_off == rb
    assert routes_on == b.last_routes  # both handles' first pass (a topology plan's first launch has two phases)
    off, never = a.decide(ra_off, 1, True), b.decide(rb, 1, True)
    assert off == never == cc.strip_added(on) and on != off
    b.run(0, 1)
    assert routes_off == b.last_routes  # ... and their second
    dc.mark(snap, "drift")
    for n in snap["stateNodes"]:
        dc.fill(n)
    a, b = Consolidator(json.dumps(snap)), Consolidator(json.dumps(snap))
    d_on, d_off, d_never = a.disrupt("drift", launch_lists=True), a.disrupt("drift"), b.disrupt("drift")
    for d in (d_on, d_off, d_never):
        d.pop("kernel_ms")
    assert d_on["command"]["action"] == "replace" and "launchPrices" in d_on["command"]["replacements"][0]
    assert d_off == d_never == cc.strip_added(d_on)


def test_lifecycle():
    """A second pass on the handle, a pass after ks_cons_update, and a handle loaded from the updated one's bytes."""
    snap = cc.cut_case(65)
    c, got, want, lists = consolidate(snap, "cut-65")
    recs, _ = c.run(0, 1, launch_lists=True)  # the rows are refilled
    again = c.decide(recs, 1)
    assert again == got and c.claim_launch(got["multi"]["command"]["sim"]) == lists["multi"]
    node = snap["stateNodes"][2]
    delta = {"deletePods": [node["pods"][0]["metadata"]["uid"]]}
    cur = cons_delta.apply_delta(copy.deepcopy(snap), delta)
    want2 = cc.oracle_consolidate("cut-65-updated", cur)
    assert want2["multi"]["command"]["action"] == "replace"
    c.update(delta)
    for handle in (c, Consolidator.from_binary(c.save())):
        doc = handle.consolidate(launch_lists=True)
        doc.pop("kernel_ms")
        assert cc.strip_added(doc) == want2
        check_command(cur, handle, doc["multi"]["command"], want2["multi"]["command"])


def test_duplicate_names_are_refused():
    snap = dc.mark(cc.duplicate_names_case(), "drift")
    for n in snap["stateNodes"]:
        dc.fill(n)
    c = Consolidator(json.dumps(snap))
    with pytest.raises(KsError) as e:
        c.run(0, 1, launch_lists=True)
    assert e.value.code == KS_ERR_UNSUPPORTED
    with pytest.raises(KsError) as e:
        c.disrupt("drift", launch_lists=True)
    assert e.value.code == KS_ERR_UNSUPPORTED
    # the flag off: as a handle that never asked
    d = Consolidator(json.dumps(snap))
    assert written(c.run(0, 1)[0], c.record_bytes) == written(d.run(0, 1)[0], d.record_bytes)
    x, y = c.disrupt("drift"), d.disrupt("drift")
    x.pop("kernel_ms"), y.pop("kernel_ms")
    assert x == y and x["command"]["action"] == "replace"


# ---- Drift / Expiration ---------------------------------------------------------------------------------------

def check_disrupt(name, snap, c, method="drift", **kw):
    want, lists = cc.oracle_disrupt(name, snap, method)
    got = c.disrupt(method, launch_lists=True, **kw)
    assert got["method"] == method
    assert cc.strip_added({k: got[k] for k in ("candidates", "command", "sims")}) == want
    reps = got["command"]["replacements"]
    assert len(reps) == len(lists)
    for i, (rep, (names, prices, nopt)) in enumerate(zip(reps, lists)):
        assert rep["launchInstanceTypes"] == names and rep["launchPrices"] == prices
        assert c.disrupt_launch(i) == (names, prices, nopt)
    with pytest.raises(KsError) as e:
        c.disrupt_launch(len(lists))
    assert e.value.code == KS_ERR_ARG
    assert (c.launch_ms() > 0) == bool(lists)
    return got, want, lists


EXPECT = {"claims-1": 1, "claims-2": 2, "claims-70": 70}


@pytest.mark.parametrize("name", list(cc.DISRUPT_CASES))
def test_disrupt_replacements(name):
    snap = cc.DISRUPT_CASES[name]()
    want, lists = cc.oracle_disrupt(name, snap)
    assert want["command"]["action"] == "replace" and len(lists) == EXPECT.get(name, 1)
    if name == "types-130":
        assert lists[0][2] > lc.CUT == len(lists[0][0])
    if name in ("types-65", "types-130"):
        assert len(set(lists[0][1])) < len(lists[0][1])
    if name in ("selectors", "topology"):  # the claim's record carries more than the pool's requirements
        assert len(want["command"]["replacements"][0]["requirements"]) > 2
    if name == "last-of-300":
        assert want["command"]["candidates"] == [want["candidates"][-1]] and len(want["candidates"]) == 300
    c = Consolidator(json.dumps(snap))
    check_disrupt(name, snap, c)
    off = c.disrupt("drift")  # the flag off on the same handle: no lists, no accessor
    assert "launchPrices" not in json.dumps(off) and c.launch_ms() == 0
    with pytest.raises(KsError) as e:
        c.disrupt_launch(0)
    assert e.value.code == KS_ERR_ARG


def test_expiration_replacements():
    """The other method: Expired conditions, no Drifted one, ties and a second option word."""
    snap = cc.expiration_case()
    want, lists = cc.oracle_disrupt("expiration", snap, "expiration")
    assert want["command"]["action"] == "replace" and lists[0][2] == 65 and len(set(lists[0][1])) < 65
    assert cc.oracle_disrupt("expiration", snap, "drift")[0]["candidates"] == []
    c = Consolidator(json.dumps(snap))
    check_disrupt("expiration", snap, c, method="expiration")
    nothing = c.disrupt("drift", launch_lists=True)  # no drifted candidate: nothing launched
    assert nothing["command"]["action"] == "no-op" and c.launch_ms() == 0


def test_seventy_claims_past_the_lds_resident_claims():
    snap = cc.DISRUPT_CASES["claims-70"]()
    c = Consolidator(json.dumps(snap))
    for budget in range(10 * 1024, 6 * 1024, -512):  # as tests/test_disrupt_gpu.py: the first budget below 70 LDS claims
        plan = c.disrupt("drift", lds_budget=budget)["plan"]
        if plan["KL"] < 70:
            break
    assert plan["KL"] < 70 <= plan["KO"], (budget, plan)
    got, _, lists = check_disrupt("claims-70", snap, c, lds_budget=budget)
    assert got["plan"] == plan and len(lists) == 70


@pytest.mark.parametrize("which", ("none", "empty"))
def test_commands_without_replacements(which):
    if which == "none":
        snap = lc.eighths(dc.count_case(65, "none"))
    else:
        snap = lc.eighths(dc.claims_case(1))
        for n in snap["stateNodes"]:
            n["pods"] = []
    want, lists = cc.oracle_disrupt("no-replacement-" + which, snap)
    assert want["command"]["action"] == ("no-op" if which == "none" else "delete") and not lists
    c = Consolidator(json.dumps(snap))
    check_disrupt("no-replacement-" + which, snap, c)
    assert c.launch_ms() == 0
