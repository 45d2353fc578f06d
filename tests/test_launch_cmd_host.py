"""The reference of the disruption-command launch lists on the oracle alone (no GPU): the cases of
tests/launch_cmd_cases.py exercise what tests/test_launch_cmd_gpu.py says they do, and the new C-ABI exists."""
import copy
import json

import pytest

import cons_delta
import disrupt_cases as dc
import launch_cases as lc
import launch_cmd_cases as cc
from karpenter_amd import synth
from karpenter_amd import scheduler


def replace_commands():
    """(case, snapshot, replacement) of every consolidation replace command of the suite."""
    out = []
    for name, (builder, _) in cc.CONS_CASES.items():
        snap = builder()
        doc = cc.oracle_consolidate(name, snap)
        out += [(name, snap, doc[m]["command"]["replacement"]) for m in ("multi", "single")
                if doc[m]["command"]["action"] == "replace"]
    for kind in cc.CARRIED_KINDS:
        snap = cc.carried_case(kind)
        doc = cc.oracle_consolidate("carried-" + kind, snap)
        out.append(("carried-" + kind, snap, doc["multi"]["command"]["replacement"]))
    return out


def test_cut_cases_have_the_stated_counts():
    for name, (builder, props) in cc.CONS_CASES.items():
        cmd = cc.oracle_consolidate(name, builder())["multi"]["command"]
        assert cmd["action"] == "replace", name
        if "multi" in props:
            assert len(cmd["replacement"]["instanceTypeOptions"]) == props["multi"], name
    assert {31, 32, 33, 65, 99, 100, 101} <= set(cc.CUTS)
    names, prices, n = cc.expected_launch(cc.wide_case(), cc.oracle_consolidate("wide-236", cc.wide_case())["multi"]["command"]["replacement"])
    assert n == 236 and len(names) == len(prices) == lc.CUT and prices == sorted(prices)


@pytest.mark.parametrize("kind", cc.CARRIED_KINDS)
def test_the_carried_case_is_carried_and_narrowed(kind):
    snap = cc.carried_case(kind)
    doc = cc.oracle_consolidate("carried-" + kind, snap)
    cmd = doc["multi"]["command"]
    assert [(p["mid"], p["carried"]) for p in doc["multi"]["path"]] == [(2, False), (1, True)]
    assert cmd["action"] == "replace" and cmd["candidates"] == ["cand-0", "cand-1"]
    assert (synth.CT + " In [spot]") in cmd["replacement"]["requirements"]
    names, prices, n = cc.expected_launch(snap, cmd["replacement"])
    assert n == 4 and names[0] == "small-4" and prices[0] == 0.05  # the spot offering, not the on-demand 0.1
    un, _ = cc.order_options(snap, cmd["replacement"]["instanceTypeOptions"], cc.unnarrowed(cmd["replacement"]["requirements"]))
    assert un != names


def test_ties_and_orders_across_the_suite():
    ties = 0
    for name, snap, rep in replace_commands():
        names, prices, n = cc.expected_launch(snap, rep)
        assert n == len(rep["instanceTypeOptions"]) and len(names) == min(n, lc.CUT) and prices == sorted(prices)
        assert all(a[1].encode() < b[1].encode() for a, b in zip(zip(prices, names), zip(prices[1:], names[1:])) if a[0] == b[0])
        ties += len(set(prices)) < len(prices)
    for name, builder in cc.DISRUPT_CASES.items():
        if name in ("types-65", "types-130"):
            _, lists = cc.oracle_disrupt(name, builder())
            ties += any(len(set(p)) < len(p) for _, p, _ in lists)
    assert ties >= 3
    # the narrowed order differs from the claim's own
    snap = cc.flip_case()
    rep = cc.oracle_consolidate("flip", snap)["multi"]["command"]["replacement"]
    assert cc.order_options(snap, rep["instanceTypeOptions"], cc.unnarrowed(rep["requirements"]))[0] != cc.expected_launch(snap, rep)[0]


def test_the_lifecycle_and_disrupt_cases_on_the_oracle():
    snap = cc.cut_case(65)
    delta = {"deletePods": [snap["stateNodes"][2]["pods"][0]["metadata"]["uid"]]}
    cur = cons_delta.apply_delta(copy.deepcopy(snap), delta)
    assert cc.oracle_consolidate("cut-65-updated", cur)["multi"]["command"]["action"] == "replace"
    for name, builder in cc.DISRUPT_CASES.items():
        want, lists = cc.oracle_disrupt(name, builder())
        assert want["command"]["action"] == "replace" and lists, name
        for names, prices, nopt in lists:
            assert len(names) == min(nopt, lc.CUT) and prices == sorted(prices)
    want, lists = cc.oracle_disrupt("expiration", cc.expiration_case(), "expiration")
    assert want["command"]["action"] == "replace" and lists[0][2] == 65
    assert cc.oracle_disrupt("expiration", cc.expiration_case(), "drift")[0]["candidates"] == []
    assert len(cc.oracle_disrupt("claims-70", cc.DISRUPT_CASES["claims-70"]())[1]) == 70
    assert cc.oracle_disrupt("types-130", cc.DISRUPT_CASES["types-130"]())[1][0][2] > lc.CUT


def test_strip_added_removes_only_the_added_keys():
    doc = {"command": {"action": "replace", "sim": 3, "replacement": {"instanceTypeOptions": ["a"], "launchPrices": [1.0],
                                                                        "launchInstanceTypes": ["a"]}}, "sims": [{"x": 1}]}
    assert cc.strip_added(doc) == {"command": {"action": "replace", "replacement": {"instanceTypeOptions": ["a"]}}, "sims": [{"x": 1}]}


def test_the_c_abi_and_the_python_mirror_exist():
    import inspect

    l = scheduler._cons_lib()
    for sym in ("ks_cons_claim_launch", "ks_cons_disrupt_launch", "ks_cons_launch_ms", "ks_cons_instance_type_name"):
        assert hasattr(l, sym)
    c = scheduler.Consolidator
    for fn in (c.run, c.disrupt, c.consolidate):
        assert inspect.signature(fn).parameters["launch_lists"].default is False
    assert all(hasattr(c, m) for m in ("claim_launch", "disrupt_launch", "launch_ms"))
    assert json.dumps(dc.KIND)  # (the cases module imports)
