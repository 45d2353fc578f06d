"""Snapshots and the reference for the launch lists of disruption commands (tests/test_launch_cmd_gpu.py,
test_launch_cmd_host.py, test_launch_cmd_abi_c.py): what ToNodeClaim hands the cloud provider for a consolidation
replacement (ks_cons_run + ks_cons_decide / ks_cons_claim_launch) and for every Drift / Expiration replacement
(ks_cons_disrupt / ks_cons_disrupt_launch).

The expected lists come from the oracle alone.  Consolidation: the oracle's command carries the replacement's
instanceTypeOptions and its requirements, already narrowed to spot where consolidation.go:181-188 narrows them; each
option is priced with launch_cases.option_price under the zone and capacity-type requirements, the options are
sorted by (price, name bytewise) and cut at 100.  Drift / Expiration: the picked candidate's Solve on the oracle,
whose NewNodeClaims carry "launchInstanceTypes".  Every snapshot goes through launch_cases.eighths first, so prices
are exact through JSON and ties are plentiful."""
import copy
import json

import carry_scenarios
import disrupt_cases as dc
import disrupt_reference as ref
import launch_cases as lc
from karpenter_amd import synth

ADDED_KEYS = ("launchInstanceTypes", "launchPrices", "sim")


# ---- references -----------------------------------------------------------------------------------------------

def order_options(snap, names, requirements):
    """(names in OrderByPrice order, their prices) of the options `names` under the oracle's requirement strings."""
    reqs = dict(lc.parse_requirement(t) for t in requirements)
    by_name = {it["name"]: it for it in snap["instanceTypes"]}
    priced = sorted((lc.option_price(by_name[n], reqs.get(synth.ZONE), reqs.get(synth.CT)), n.encode()) for n in names)
    return [n.decode() for _, n in priced], [p for p, _ in priced]


def expected_launch(snap, replacement):
    """(launch names, launch prices, option count) of an oracle replacement {instanceTypeOptions, requirements}."""
    names, prices = order_options(snap, replacement["instanceTypeOptions"], replacement["requirements"])
    return names[:lc.CUT], prices[:lc.CUT], len(names)


def unnarrowed(requirements):
    """The requirement strings without the capacity-type entry consolidation narrowed."""
    return [t for t in requirements if not t.startswith(synth.CT + " ")]


def strip_added(doc):
    """A decide / disrupt document without the keys launch lists add."""
    if isinstance(doc, dict):
        return {k: strip_added(v) for k, v in doc.items() if k not in ADDED_KEYS}
    if isinstance(doc, list):
        return [strip_added(v) for v in doc]
    return doc


_memo = {}


def oracle_consolidate(key, snap):
    from oracle import bridge

    if key not in _memo:
        _memo[key] = bridge.consolidate(json.dumps(snap), all_sims=False)[0]
    return _memo[key]


def oracle_disrupt(key, snap, method="drift"):
    """(the reference command document, [(launch names, prices, option count) per replacement])."""
    from oracle import bridge

    k = ("disrupt", key, method)
    if k not in _memo:
        want = ref.command(snap, method)
        lists = []
        if want["command"]["action"] == "replace":
            _, _, text = ref._Solves(snap).input(want["command"]["candidates"][0])
            res = bridge.solve(text)[0]
            assert [c["instanceTypeOptions"] for c in res["newNodeClaims"]] == \
                [r["instanceTypeOptions"] for r in want["command"]["replacements"]]
            by_name = {it["name"]: it for it in snap["instanceTypes"]}
            for c in res["newNodeClaims"]:
                reqs = dict(lc.parse_requirement(t) for t in c["requirements"])
                names = c["launchInstanceTypes"]
                prices = [lc.option_price(by_name[n], reqs.get(synth.ZONE), reqs.get(synth.CT)) for n in names]
                lists.append((names, prices, len(c["instanceTypeOptions"])))
        _memo[k] = (want, lists)
    return _memo[k]


# ---- consolidation --------------------------------------------------------------------------------------------

def cut_case(nopt):
    """A multi-node replace of all 6 candidates whose command has exactly nopt options after filterOutSameType
    (checked on the oracle: the count follows the number of instance types), narrowed to spot."""
    n = nopt + 17
    return lc.eighths(synth.cluster_snapshot(6, 2, n_its=n, it_range=(n - 10, n), seed=8, spot_frac=0))


def wide_case():
    """236 options: the cut drops more than half."""
    return lc.eighths(synth.cluster_snapshot(8, 3, n_its=300, it_range=(250, 300), seed=5))


FLIPPED = ["fake-it-%d" % i for i in (20, 21, 22, 23, 24, 25)]


def flip_case():
    """cut_case(33) with six option types whose spot prices rise (in pairs of one price) where their on-demand
    prices fall: under the narrowed requirements (spot only) they order the other way round than under the claim's
    own, and the name decides within a pair."""
    snap = cut_case(33)
    for k, name in enumerate(FLIPPED):
        it = next(t for t in snap["instanceTypes"] if t["name"] == name)
        for o in it["offerings"]:
            o["price"] = (16 + k // 2) / 8 if o["capacityType"] == "spot" else (8 - k) / 8
    return snap


def single_case():
    """Full nodes of one 500m pod each, one of them on the most expensive type: a single-node replace whose
    filterByPrice output is a strict subset of the NodeClaim's options."""
    snap = dc.lean(4, n_its=40, pods_of=lambda j: [("500m", None, None)])
    big = snap["instanceTypes"][39]
    n = snap["stateNodes"][0]
    n["labels"][synth.IT_LABEL] = big["name"]
    n["capacity"] = dict(big["capacity"])
    return lc.eighths(snap)


def carried_case(kind):
    """carry_scenarios.make(kind, 0) with keep-2 full and spot offerings: the multi-node command is a replace of
    cand-0 and cand-1 chosen from the carried probe, narrowed to spot; three more 4-cpu types with mixed spot /
    on-demand prices give the list an order."""
    snap = carry_scenarios.make(kind, 0)
    keep2 = next(n for n in snap["stateNodes"] if n["name"] == "keep-2")
    for p in [keep2["pods"][0]] + [p for p in snap["clusterPods"] if p["metadata"]["name"] == keep2["pods"][0]["metadata"]["name"]]:
        p["spec"]["containers"][0]["resources"]["requests"]["cpu"] = "4"
    keep2["available"]["cpu"] = "0"
    small = next(t for t in snap["instanceTypes"] if t["name"] == "small-4")
    small["offerings"].append({"capacityType": "spot", "zone": "test-zone-1", "price": 0.05, "available": True})
    for name, spot, od in (("small-4b", 0.375, 0.125), ("small-4c", 0.125, 0.5), ("Small-4a", 0.125, 0.25)):
        snap["instanceTypes"].append(synth.fake_instance_type(name, 4, 8, pods=20, offerings=[
            {"capacityType": "spot", "zone": "test-zone-1", "price": spot, "available": True},
            {"capacityType": "on-demand", "zone": "test-zone-1", "price": od, "available": True}]))
    pools = snap.get("instanceTypesByNodePool")
    if pools:
        for k in pools:
            pools[k] = list(range(len(snap["instanceTypes"])))
    return snap


def two_templates_case():
    """Two templates whose lists overlap and end inside an option word (launch_cases.many_claims_lean_case's
    ranges): a tainted pool-a over types [0, 40) comes first, the nodes' pool over [20, 90) second, so the
    replacement's positions map through tpl_it_beg."""
    snap = lc.eighths(synth.cluster_snapshot(6, 2, n_its=90, it_range=(80, 90), seed=8, spot_frac=0))
    taint = {"key": "dedicated", "value": "a", "effect": "NoSchedule"}
    pool_a = synth.node_pool("pool-a", weight=50, taints=[taint])
    pool_a["spec"]["disruption"] = copy.deepcopy(snap["nodePools"][0]["spec"]["disruption"])
    snap["nodePools"] = [pool_a] + snap["nodePools"]
    snap["nodeClaimTemplates"] = [pool_a] + snap["nodeClaimTemplates"]
    snap["instanceTypesByNodePool"] = {"pool-a": list(range(0, 40)), "default": list(range(20, 90))}
    return snap


def topology_case():
    """A topology cluster (a two-phase launch: multi-node prefixes first, single-node simulations on a second stream)."""
    return lc.eighths(synth.cluster_snapshot(10, 3, n_its=60, it_range=(40, 60), seed=23, spot_frac=0.3, topology=6))


def mw_case():
    """tests/test_cons_mw_gpu.py's first shape (with KS_SIM_MW=1 KS_SIM_MW_MIN=1: a sims_mixed launch)."""
    return lc.eighths(synth.cluster_snapshot(40, 8, n_its=60, seed=1, spot_frac=0.3, it_range=(4, 40)))


CUTS = (31, 32, 33, 65, 99, 100, 101, 113)
# name -> (builder, {"multi": expected option count or None, "single": ...}); None: that method's command is no replace
CONS_CASES = {
    **{"cut-%d" % n: ((lambda n=n: cut_case(n)), {"multi": n}) for n in CUTS},
    "wide-236": (wide_case, {"multi": 236}),
    "flip": (flip_case, {"multi": 33}),
    "single": (single_case, {}),
    "two-templates": (two_templates_case, {}),
    "topology": (topology_case, {}),
    "mw": (mw_case, {}),
}
CARRIED_KINDS = ("pref-node", "late-carry")


def duplicate_names_case():
    """cut_case(31) with one option's name given to a second instance type of the template."""
    snap = cut_case(31)
    snap["instanceTypes"][21]["name"] = snap["instanceTypes"][20]["name"]
    return snap


# ---- Drift / Expiration ---------------------------------------------------------------------------------------

def _drift(builder, full=False, ties=False):
    def build():
        snap = builder()
        if full:  # no room anywhere: the moved pods need replacements
            for n in snap["stateNodes"]:
                dc.fill(n)
        if ties:  # prices in groups of about three, unrelated to the list order
            n = len(snap["instanceTypes"])
            for i, it in enumerate(snap["instanceTypes"]):
                for o in it["offerings"]:
                    o["price"] = ((i * 7) % max(n // 3, 1) + 1) / 8
        return lc.eighths(snap)

    return build


def expiration_case():
    """disrupt_cases.types_case(65) with the nodes Expired instead of Drifted, prices in tie groups."""
    return _drift(lambda: dc.mark(dc.types_case(65), "expiration", seed=3), ties=True)()


DISRUPT_CASES = {
    "claims-1": _drift(lambda: dc.claims_case(1)),
    "claims-2": _drift(lambda: dc.claims_case(2)),
    "claims-70": _drift(lambda: dc.claims_case(70)),
    "types-33": _drift(lambda: dc.types_case(33)),
    "types-65": _drift(lambda: dc.types_case(65), ties=True),
    "types-130": _drift(lambda: dc.types_case(130), ties=True),
    "selectors": _drift(dc.selectors_case, full=True),
    "topology": _drift(dc.topology_case, full=True),
    "last-of-300": _drift(lambda: dc.count_case(300, "last")),
}
