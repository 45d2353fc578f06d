"""Snapshot builders and references for the launch-list tests (tests/test_launch_gpu.py, test_launch_host.py,
test_launch_abi_c.py): NodeClaimTemplate.ToNodeClaim's OrderByPrice and its cut to 100 instance types.

Every price is a multiple of 1/8 (exact in binary, and exact through any JSON number writer and parser), except
where a case says otherwise (1e300, whose shortest decimal form round-trips).  The expected lists are the oracle's
"launchInstanceTypes"; the expected prices come from `claim_prices` below, a few lines over the snapshot's
offerings and the claim's structured requirements."""
import json

import numpy as np

import problems
from karpenter_amd import synth

ZONES = ["test-zone-1", "test-zone-2", "test-zone-3"]
CTS = ["spot", "on-demand"]
CUT = 100
CUT_SIZES = [1, 31, 32, 33, 63, 64, 65, 99, 100, 101, 128, 257, 800]
MAX_PRICE = 1.7976931348623157e308  # math.MaxFloat64


def offers(price, zones=ZONES, cts=CTS):
    return [{"capacityType": ct, "zone": z, "price": price, "available": True} for z in zones for ct in cts]


def one_template(its, pods, template=None):
    snap = synth.benchmark_snapshot(0, 0, diverse=False)
    snap["instanceTypes"] = its
    snap["instanceTypesByNodePool"] = {"default-pool": list(range(len(its)))}
    if template is not None:
        snap["nodeClaimTemplates"] = [template]
    snap["pods"] = pods
    return snap


def small_pod(i=0, **kw):
    return synth.pod(i, cpu="100m", mem="64Mi", **kw)


# ---- the cut and the lane / word edges ------------------------------------------------------------------------

def cut_case(n, prices):
    """One template of n instance types that one small pod keeps all of; prices run against list position:
    "desc" (the last is the cheapest) or "shuffle" (a fixed permutation: 7919 is prime and divides no size)."""
    its = []
    for i in range(n):
        p = (n - i) / 8 if prices == "desc" else ((i * 7919) % n + 1) / 8
        its.append(synth.fake_instance_type("fake-it-%d" % i, 4, 8, offerings=offers(p)))
    return one_template(its, [small_pod()])


def fits_prefix_case():
    """150 types of 1 .. 150 cpu, prices descending; a 20-cpu pod: Fits removes the first 20 of the list, 130 stay."""
    its = [synth.fake_instance_type("fake-it-%d" % i, i + 1, 512, offerings=offers((150 - i) / 8)) for i in range(150)]
    return one_template(its, [synth.pod(0, cpu="20", mem="64Mi")])


# ---- ties -----------------------------------------------------------------------------------------------------

def tie_names(n):
    """Names whose bytewise order differs from the numeric one (it-10 < it-9), from the list order (reversed) and,
    for every fifth, by case (It-2 < it-1)."""
    return [("It-%d" if i % 5 == 2 else "it-%d") % i for i in reversed(range(n))]


def tie_groups_case():
    """120 options in price groups of 7; the group of positions 98 .. 104 straddles the cut."""
    names = tie_names(120)
    its = [synth.fake_instance_type(nm, 4, 8, offerings=offers((((i * 37) % 120) // 7 + 1) / 8)) for i, nm in enumerate(names)]
    return one_template(its, [small_pod()])


def all_equal_case():
    return one_template([synth.fake_instance_type(nm, 4, 8, offerings=offers(0.5)) for nm in tie_names(130)], [small_pod()])


def signs_case():
    """0.0 and -0.0 compare equal in Go (the name decides between them), a negative price sorts first, 1e300 last."""
    prices = [("a", 0.0), ("b", -0.0), ("c", 0.0), ("d", -0.0), ("e", -1.5), ("f", 1e300), ("g", 0.125), ("h", -0.0),
              ("i", -1.5), ("j", 0.0)]
    return one_template([synth.fake_instance_type("sign-%s" % nm, 4, 8, offerings=offers(p)) for nm, p in prices],
                        [small_pod()])


# ---- requirements decide the price ----------------------------------------------------------------------------

def _matrix_price(j, zi, ci):
    return ((j * 5 + zi * 7 + ci * 11 + (j * zi) % 3) % 13 + 1) / 8


def matrix_its(unavailable_cheapest=True):
    """12 types whose price differs per (zone, capacity type).  Type 3's cheapest offering is unavailable (or, for the
    comparison, available): it must not be the key."""
    its = []
    for j in range(12):
        offs = [{"capacityType": ct, "zone": z, "price": _matrix_price(j, zi, ci), "available": True}
                for zi, z in enumerate(ZONES) for ci, ct in enumerate(CTS)]
        if j == 3:
            offs.append({"capacityType": "spot", "zone": ZONES[0], "price": 0.0, "available": not unavailable_cheapest})
        its.append(synth.fake_instance_type("mx-%02d" % j, 4, 8, offerings=offs))
    return its


def _not_in_zone(values):
    return {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
        {"matchExpressions": [{"key": synth.ZONE, "operator": "NotIn", "values": values}]}]}}}


REQUIREMENT_CASES = {
    "zone-in": lambda: one_template(matrix_its(), [small_pod(node_selector={synth.ZONE: ZONES[1]})]),
    "zone-notin": lambda: one_template(matrix_its(), [small_pod(affinity=_not_in_zone([ZONES[0]]))]),
    "spot": lambda: one_template(matrix_its(), [small_pod(node_selector={synth.CT: "spot"})]),
    "neither": lambda: one_template(matrix_its(), [small_pod()]),
    # the comparison for "neither": the same list with type 3's cheapest offering available
    "neither-available": lambda: one_template(matrix_its(unavailable_cheapest=False), [small_pod()]),
}
# (case, the unrestricted case its order must differ from)
REQUIREMENT_DIFFERS = [("zone-in", "neither"), ("zone-notin", "neither"), ("spot", "neither"),
                       ("neither", "neither-available")]


# ---- many claims ----------------------------------------------------------------------------------------------

def eighths(snap):
    """The snapshot with every offering price rounded to a multiple of 1/8 (at least 1/8); in place."""
    for it in snap["instanceTypes"]:
        for o in it["offerings"]:
            o["price"] = max(1, round(o["price"] * 8)) / 8
    return snap


def many_claims_case(n_big=150, seed=11, lists=((0, 32), (20, 84)), selectors=True):
    """About n_big NodeClaims over two templates whose lists differ in length and overlap (positions map through
    tpl_it_beg): pool-a (first, tainted) takes the tolerating pods, pool-b the rest.  90 types of 7 or 8 cpu with
    per-(zone, capacity type) prices and many ties; no two big pods (4 .. 7 cpu) share a type.  A third of the pods
    select a zone or spot, so the claims' records differ (selectors=False: none do, and the Solve is LEAN).
    lists: the two templates' ranges of types.  With selectors the lists are whole option words (32 and 64 types):
    the non-LEAN Solve fails its own host check ("options beyond its template's list") on a template whose list ends
    inside a word that a longer template uses, with or without launch lists; the LEAN case below has such lists."""
    rng = np.random.default_rng(seed)
    its = []
    for i in range(90):
        offs = [{"capacityType": ct, "zone": z, "price": int(rng.integers(1, 9)) / 8, "available": bool(rng.random() < 0.9)}
                for z in ZONES for ct in CTS]
        offs[0]["available"] = offs[3]["available"] = offs[4]["available"] = True  # every zone, spot and on-demand stay
        its.append(synth.fake_instance_type("mc-%02d" % i, 7 + i % 2, 16, pods=20, offerings=offs))
    taint = {"key": "dedicated", "value": "a", "effect": "NoSchedule"}
    tpl_a = synth.node_pool("pool-a", weight=50, taints=[taint])
    tpl_b = synth.node_pool("pool-b", weight=10)
    pods = []
    for i in range(n_big):
        kw = {}
        u = rng.random() if selectors else 1.0
        if u < 0.15:
            kw["node_selector"] = {synth.ZONE: ZONES[int(rng.integers(3))]}
        elif u < 0.25:
            kw["node_selector"] = {synth.CT: "spot"}
        elif u < 0.33:
            kw["affinity"] = _not_in_zone([ZONES[int(rng.integers(3))]])
        if i % 2:
            kw["tolerations"] = [{"key": "dedicated", "operator": "Equal", "value": "a", "effect": "NoSchedule"}]
        pods.append(synth.pod(i, cpu="%dm" % int(rng.choice(range(4000, 7001, 500))), mem="%dMi" % int(rng.choice([512, 1024])), **kw))
    for i in range(60):
        pods.append(synth.pod(n_big + i, cpu="250m", mem="128Mi"))
    snap = synth.benchmark_snapshot(0, 0, diverse=False)
    snap["instanceTypes"] = its
    snap["instanceTypesByNodePool"] = {"pool-a": list(range(*lists[0])), "pool-b": list(range(*lists[1]))}
    snap["nodeClaimTemplates"] = [tpl_a, tpl_b]
    snap["pods"] = [pods[int(i)] for i in rng.permutation(len(pods))]
    return snap


def many_claims_lean_case():
    """The same pods without selectors over lists of 40 and 70 types: both end inside an option word."""
    return many_claims_case(lists=((0, 40), (20, 90)), selectors=False)


def lean_case():
    """Resource-only pods (the LEAN Solve): tests/replan_cases.py's base, 40 NodeClaims."""
    import replan_cases as rp

    return eighths(rp.lean_base(40))


def replan_case():
    """A Solve that re-plans for NodeClaim capacity (one NodeClaim more than the level-0 plan holds at the budget)."""
    import replan_cases as rp

    name = "lean-K0+1"
    return eighths(json.loads(rp.snapshot(name))), rp.CASES[name]["budget"]


def duplicate_names_case():
    its = [synth.fake_instance_type(nm, 4, 8, offerings=offers((i + 1) / 8)) for i, nm in enumerate(["dup-a", "dup-b", "dup-a"])]
    return one_template(its, [small_pod()])


# ---- random ---------------------------------------------------------------------------------------------------

# 16 problems from tests/problems.py's generator: requirements and taints in all, topology for the odd seeds.  "wide":
# 400 instance types in one template, for claims past the cut; "pools": 40 types over up to three templates.  (400
# types over several templates are left out: on some of them the non-LEAN Solve fails its own host check, "options
# beyond its template's list", with or without launch lists.)  The seeds were chosen on the oracle alone: every
# problem has NodeClaims, and together they give at least 3 claims of more than 100 options and at least 3 with two
# options at one price (test_launch_host.py and test_launch_gpu.py assert it).
RANDOM_CASES = ([("wide", s) for s in (7101, 7102, 7104, 7105, 7107, 7108, 7111, 7112)] +
                [("pools", s) for s in (7100, 7101, 7102, 7104, 7105, 7107, 7108, 7115)])
RANDOM_IDS = ["%s-%d" % c for c in RANDOM_CASES]


def random_case(case):
    shape, seed = case
    kw = dict(n_its=400, n_templates=1) if shape == "wide" else dict(n_its=40)
    return eighths(problems.random_problem(seed, n_pods=60, topology=bool(seed % 2), affinity=bool(seed % 4 == 1), **kw))


# ---- references -----------------------------------------------------------------------------------------------

def _allows(req, value):
    """Requirement.Has for one value; req: (op, values) or None for an absent key."""
    if req is None:
        return True
    op, values = req
    return {"In": value in values, "NotIn": value not in values, "Exists": True, "DoesNotExist": False}[op]


def option_price(it, zone_req, ct_req):
    ps = [o["price"] for o in it["offerings"]
          if o.get("available", True) and _allows(zone_req, o["zone"]) and _allows(ct_req, o["capacityType"])]
    return min(ps) if ps else MAX_PRICE


def claim_prices(snap, claim):
    """[price per entry of claim["launch"]] from the snapshot's available offerings and the claim's structured
    zone / capacity-type requirements."""
    reqs = {k: (op, vals) for k, op, vals, _, _ in claim["requirements"]}
    by_name = {it["name"]: it for it in snap["instanceTypes"]}
    return [option_price(by_name[n], reqs.get(synth.ZONE), reqs.get(synth.CT)) for n in claim["launch"]]


def parse_requirement(text):
    """("key", (op, values)) of one entry of the oracle's "requirements" ("key In [a b]", "key Exists", ...)."""
    parts = text.split(" ", 2)
    vals = parts[2].strip("[]").split() if len(parts) > 2 and parts[2].startswith("[") else []
    return parts[0], (parts[1], vals)


def oracle_claim_stats(snap, oracle_doc):
    """(claims with more than 100 options, claims with two options at one price) in the oracle's Results."""
    by_name = {it["name"]: it for it in snap["instanceTypes"]}
    wide = ties = 0
    for c in oracle_doc["newNodeClaims"]:
        reqs = dict(parse_requirement(t) for t in c["requirements"])
        ps = [option_price(by_name[n], reqs.get(synth.ZONE), reqs.get(synth.CT)) for n in c["instanceTypeOptions"]]
        wide += len(ps) > CUT
        ties += len(set(ps)) < len(ps)
    return wide, ties


_memo = {}


def oracle(key, snap):
    """The oracle's Results of a snapshot, once per process per key."""
    from oracle import bridge

    if key not in _memo:
        _memo[key] = bridge.solve(json.dumps(snap))[0]
    return _memo[key]
