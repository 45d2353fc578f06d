"""LEAN Solve: the per-template requirement / offering bitsets kept in LDS (KS_TPL_MASKS).  A NewNodeClaim
that misses the memo of the last one reads them instead of deriving them again; only Fits still reads the pod.
Every GPU case is bit-exact parity of the canonical Results -- the pod errors, which print each template's
failure flags, included -- with the oracle; tplMaskFills / tplMaskHits show which path ran (both 0 on a build with
the switch at 0, which ks_problem_inspect reports as "tplMasks": the default build).  Shapes: 70 instance
types per template (one 64-position chunk plus a tail of 6), at most 42 pods, one pod per NodeClaim (the
instance types hold one pod), so every pod is a NewNodeClaim.

Pods of two shapes can only alternate in NewQueue's order when they tie on cpu and memory (queue.go:83-112 sorts by
both before the UID), so shape B is shape A plus one unit of an extended resource that only some instance types
carry: a fourth resource, which the LEAN instantiation for four resources covers.

An instance type with a complement requirement (an irregular position, checked per position by rs_intersects) is
expressible: the snapshot's instance-type requirements take NotIn."""
import copy
import json

import pytest

import problems
from karpenter_amd import Scheduler, inspect, synth
from oracle import bridge

VENDOR = "fake.com/vendor-a"
N_ITS = 70


def _its(n=N_ITS, offerings_for=None, complement=False, vendor=True):
    """n instance types of one pod each: cpu 1..8, 2 Gi per cpu; the large ones (cpu > 4) carry one VENDOR unit.
    offerings_for(i) -> an offering list for type i (None: the default five).  complement: every third type states
    its size as NotIn of the other size (an irregular position of the feasibility tables)."""
    out = []
    for i in range(n):
        cpu = i % 8 + 1
        large = cpu > 4 and 2 * cpu > 8
        it = synth.fake_instance_type("it-%02d" % i, cpu, 2 * cpu, pods=1,
                                      offerings=offerings_for(i) if offerings_for else None,
                                      extra_capacity={VENDOR: "1"} if large and vendor else None)
        if complement and i % 3 == 0:
            for r in it["requirements"]:
                if r["key"] == "size":
                    r["operator"], r["values"] = "NotIn", ["small" if large else "large"]
        out.append(it)
    return out


def _pod(i, shape):
    p = synth.pod(i, cpu="500m", mem="256Mi")
    if shape == "B":
        p["spec"]["containers"][0]["resources"]["requests"][VENDOR] = "1"
    return p


SMALL = [{"key": "size", "operator": "In", "values": ["small"]}]


def _snapshot(pods, its, templates):
    """templates: [(name, requirements, limits or None)]; every template lists every instance type."""
    snap = synth.benchmark_snapshot(0, 1, 1, diverse=False)
    snap["instanceTypes"] = its
    snap["nodeClaimTemplates"] = [synth.node_pool(n, requirements=r) for n, r, _ in templates]
    snap["nodePools"] = [synth.node_pool(n, requirements=r, limits=l) for n, r, l in templates if l]
    snap["instanceTypesByNodePool"] = {n: list(range(len(its))) for n, _, _ in templates}
    snap["pods"] = pods
    return snap


def _solve_both(snap):
    s = json.dumps(snap)
    want, _ = bridge.solve(s)
    got = Scheduler(s).solve()
    return problems.canonical(want), got


def _assert_parity(want, got):
    g = got.canonical()
    for key in ("newNodeClaims", "existingNodes", "podErrors"):
        if want[key] != g[key] and isinstance(want[key], list):
            for i, (a, b) in enumerate(zip(want[key], g[key])):
                assert a == b, "%s[%d]: want %s\n got %s" % (key, i, json.dumps(a)[:1500], json.dumps(b)[:1500])
        assert want[key] == g[key], key
    assert want == g


def _lean(got):
    r = got.stats["route"]
    return r["family"] == "solve" and r["lean"] == 1


def _masks_built():
    return inspect(synth.benchmark_snapshot(1, 1, 1, diverse=False))["tplMasks"] == 1


def _check_counters(got, fills, claims):
    """fills rows derived; every other NewNodeClaim that missed the memo read its row (0 and 0 on a build without
    the table)."""
    st = got.stats
    print("claims %d tplMemoHits %d tplMaskFills %d tplMaskHits %d" % (
        claims, st["tplMemoHits"], st["tplMaskFills"], st["tplMaskHits"]))
    assert _lean(got)
    if _masks_built():
        assert st["tplMaskFills"] == fills
        assert st["tplMaskHits"] == claims - fills - st["tplMemoHits"]
    else:
        assert (st["tplMaskFills"], st["tplMaskHits"]) == (0, 0)


ALTERNATING = [_pod(i, "AB"[i % 2]) for i in range(40)]


@pytest.mark.gpu
@pytest.mark.parametrize("complement", [False, True])
def test_two_templates_alternating_shapes(complement):
    """Template 0 admits the small instance types only, none of which carries the extended resource: shape A opens
    its NodeClaims there, shape B fails it (no instance type: the flags come from the row) and opens on template 1.
    The shapes alternate, so no NewNodeClaim finds its own key in the memo and every one after a template's first
    reads that template's row.  complement: a third of the instance types are irregular positions."""
    snap = _snapshot(copy.deepcopy(ALTERNATING), _its(complement=complement),
                     [("small-pool", SMALL, None), ("open-pool", [], None)])
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    assert not want["podErrors"]
    pools = [c["nodePoolName"] for c in want["newNodeClaims"]]
    assert len(pools) == 40 and pools.count("small-pool") == 20 and pools.count("open-pool") == 20
    assert got.stats["tplMemoHits"] == 0
    _check_counters(got, fills=2, claims=40)


@pytest.mark.gpu
def test_instance_types_without_a_matching_offering():
    """The template wants on-demand capacity in test-zone-1.  Every other instance type offers spot there and
    on-demand elsewhere: its zone and capacity-type requirements both intersect the template's, and no offering
    has both -- the offering row differs from the requirement row."""
    def offerings(i):
        if i % 2 == 0:
            return None
        return [{"capacityType": "spot", "zone": "test-zone-1", "price": 1.0, "available": True},
                {"capacityType": "on-demand", "zone": "test-zone-2", "price": 1.0, "available": True}]
    reqs = [{"key": synth.ZONE, "operator": "In", "values": ["test-zone-1"]},
            {"key": synth.CT, "operator": "In", "values": ["on-demand"]}]
    snap = _snapshot(copy.deepcopy(ALTERNATING), _its(offerings_for=offerings), [("zonal-pool", reqs, None)])
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    assert not want["podErrors"] and len(want["newNodeClaims"]) == 40
    for c in want["newNodeClaims"]:
        assert all(int(n[3:]) % 2 == 0 for n in c["instanceTypeOptions"]), "a type without the offering was kept"
    _check_counters(got, fills=1, claims=40)


def _unfit_pods(first):
    """40 alternating pods and two that no instance type fits.  first: by cpu, so NewQueue pops them before any
    row exists and their failures fill the rows; otherwise by memory under a smaller cpu request, so they are
    popped last and their failure flags come from rows filled long before."""
    pods = copy.deepcopy(ALTERNATING)
    for k in range(2):
        pods.append(synth.pod(100 + k, cpu="1000", mem="256Mi") if first
                    else synth.pod(100 + k, cpu="100m", mem="4000Gi"))
    return pods


@pytest.mark.gpu
@pytest.mark.parametrize("first", [True, False])
def test_pod_no_instance_type_fits(first):
    snap = _snapshot(_unfit_pods(first), _its(), [("small-pool", SMALL, None), ("open-pool", [], None)])
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    assert len(want["podErrors"]) == 2 and len(want["newNodeClaims"]) == 40
    st = got.stats
    print("pops %d tplMaskFills %d tplMaskHits %d" % (st["pops"], st["tplMaskFills"], st["tplMaskHits"]))
    assert _lean(got)
    if _masks_built():
        assert st["tplMaskFills"] == 2
        # first: both rows were filled by the failing pods, so every claim that missed the memo read one
        assert st["tplMaskHits"] == 40 - st["tplMemoHits"] - (0 if first else 2)


@pytest.mark.gpu
def test_bypassed_under_a_nodepool_limit():
    """Under a limit the candidates depend on what the NodePool has left: nothing is kept, nothing is read."""
    snap = _snapshot(copy.deepcopy(ALTERNATING), _its(), [("limited-pool", [], {"cpu": "60"})])
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    assert want["newNodeClaims"]
    assert _lean(got)
    assert (got.stats["tplMaskFills"], got.stats["tplMaskHits"], got.stats["tplMemoHits"]) == (0, 0, 0)


@pytest.mark.gpu
def test_lean_route_without_room_for_the_table():
    """64 templates of 40 instance types and three resources: the instance-type tables take 150 KiB of LDS, the plan
    keeps them (the Solve stays LEAN) and leaves the rows out -- every NewNodeClaim derives as before."""
    names = ["pool-%02d" % t for t in range(64)]
    pods = [_pod(i, "A") for i in range(20)] + [synth.pod(20 + i, cpu="400m", mem="256Mi") for i in range(20)]
    snap = _snapshot(pods, _its(40, vendor=False), [(n, [], None) for n in names])
    full = inspect(snap)["plans"][str(160 * 1024 - 256)]
    assert (full["talloc"], full["tmask"]) == (1, 0)
    want, got = _solve_both(snap)
    _assert_parity(want, got)
    assert len(want["newNodeClaims"]) == 40 and _lean(got)
    assert (got.stats["tplMaskFills"], got.stats["tplMaskHits"]) == (0, 0)


# --- the plan (host only) ----------------------------------------------------------------------------

def _r16(b):
    return (b + 15) & ~15


def _plan_snapshot(ntpl, n_its):
    names = ["pool-%02d" % t for t in range(ntpl)]
    snap = synth.benchmark_snapshot(4, 1, 1, diverse=False)
    snap["instanceTypes"] = synth.fake_instance_types(n_its)
    snap["nodeClaimTemplates"] = [synth.node_pool(n) for n in names]
    snap["instanceTypesByNodePool"] = {n: list(range(n_its)) for n in names}
    return snap


@pytest.mark.parametrize("ntpl", [1, 2, 64])
@pytest.mark.parametrize("tw", [1, 2, 13])
def test_plan_counts_the_table(ntpl, tw):
    """make_plan's bytes for the table are the kernel's carve: NTPL rows of 2 * TW words, then NTPL flag words, each
    array rounded to 16 bytes; a plan with the table is that much larger than the same plan without it would be
    (the claim capacity is the pods' here, so nothing else moves), and stays inside its budget.  (A problem holds at
    most 64 templates -- the toleration mask is one 64-bit word; scripts/tpl_mask_plan_main.cpp runs the arithmetic
    alone at 65.)"""
    n_its = {1: 20, 2: 40, 13: 400}[tw]
    doc = inspect(_plan_snapshot(ntpl, n_its))
    assert (doc["templates"], doc["TW"], doc["lean"]) == (ntpl, tw, 1)
    for budget, pl in doc["plans"].items():
        want = _r16(4 * ntpl * 2 * tw) + _r16(4 * ntpl) if pl["tmask"] else 0
        assert pl["tmaskBytes"] == want, (budget, pl)
        assert pl["tmask"] == 0 or (doc["tplMasks"] == 1 and pl["talloc"] == 1), (budget, pl)
        assert pl["tmask"] == 0 or pl["lds"] <= int(budget), (budget, pl)
    # the whole LDS: the rows are in unless the instance-type tables leave no room for them and 64 claims (64
    # templates of 40 types: 150 KiB of tables) or do not fit themselves (64 templates of 400 types)
    full = doc["plans"][str(160 * 1024 - 256)]
    if doc["tplMasks"]:
        assert full["tmask"] == (0 if ntpl == 64 and tw > 1 else 1)
        assert full["talloc"] == (0 if ntpl == 64 and tw == 13 else 1)


def test_plan_leaves_the_table_out_when_it_does_not_fit():
    """64 templates of 400 instance types: the instance-type tables alone outgrow every budget, the Solve is not
    routed LEAN and no table is planned; with 64 templates of 20 types the tables fit the whole LDS and the rows
    with them, while a 6000-byte budget holds neither."""
    big = inspect(_plan_snapshot(64, 400))
    assert all(pl["tmask"] == 0 and pl["tmaskBytes"] == 0 for pl in big["plans"].values())
    small = inspect(_plan_snapshot(64, 20))
    if small["tplMasks"]:
        assert small["plans"][str(160 * 1024 - 256)]["tmask"] == 1
    assert small["plans"]["6000"]["tmask"] == 0
