"""Problems of the LEAN Solve's fresh-NodeClaim table (KS_TPL_TABLE): tests/test_tpl_table_gpu.py compares the
GPU's Results with the oracle's on them, tests/test_tpl_table_preconditions.py proves on the oracle and the snapshot
alone that each one is in the cell its name says.

Pods of different request classes only alternate in NewQueue's order when they tie on cpu and memory (queue.go:83-112
sorts by both before the UID), so the classes differ in an extended resource that only some instance types carry: a
fourth resource, which the LEAN instantiation for four resources covers.  A "big" pod asks for 5 cpu of instance types
of at most 8, more than half the largest one, so no two share a NodeClaim: every pod opens one, and with the classes
alternating no open finds its own key in the memo."""
import replan_cases
import resource_cases
from karpenter_amd import synth

VENDOR = "fake.com/vendor-a"
IT_EDGES = [1, 31, 32, 33, 63, 64, 65, 129]  # option words and 64-position chunks: one short, exact, one over
CAP_ENV = "KS_TPL_TABLE_MAX_BYTES"


def big_its(n):
    """n instance types of 8, 7, 6, 5 cpu in turn (7.9 ... 4.9 allocatable: a 5-cpu pod fits the first three and no
    second one joins it); the even ones carry two VENDOR units."""
    return [synth.fake_instance_type("it-%03d" % i, 8 - i % 4, 2 * (8 - i % 4), pods=10,
                                     extra_capacity={VENDOR: "2"} if i % 2 == 0 else None) for i in range(n)]


def big_pod(i, units):
    p = synth.pod(i, cpu="5", mem="1Gi")
    if units:
        p["spec"]["containers"][0]["resources"]["requests"][VENDOR] = str(units)
    return p


def one_pod_its(n=70):
    """n instance types that hold one pod each (pods capacity 1): cpu 1..8, 2 Gi per cpu; the large ones (cpu > 4, the
    "size" label's) carry one VENDOR unit."""
    return [synth.fake_instance_type("it-%02d" % i, i % 8 + 1, 2 * (i % 8 + 1), pods=1,
                                     extra_capacity={VENDOR: "1"} if i % 8 + 1 > 4 else None) for i in range(n)]


def small_pod(i, units):
    p = synth.pod(i, cpu="500m", mem="256Mi")
    if units:
        p["spec"]["containers"][0]["resources"]["requests"][VENDOR] = str(units)
    return p


SMALL = [{"key": "size", "operator": "In", "values": ["small"]}]


def snapshot(pods, its, templates=(("default-pool", [], None, None),), daemons=()):
    """templates: (name, requirements, limits or None, taints or None); every template lists every instance type."""
    snap = synth.benchmark_snapshot(0, 1, 1, diverse=False)
    snap["instanceTypes"] = its
    snap["nodeClaimTemplates"] = [synth.node_pool(n, requirements=r, taints=t) for n, r, _, t in templates]
    snap["nodePools"] = [synth.node_pool(n, requirements=r, limits=l, taints=t) for n, r, l, t in templates if l]
    snap["instanceTypesByNodePool"] = {n: list(range(len(its))) for n, _, _, _ in templates}
    snap["daemonSetPods"] = list(daemons)
    snap["pods"] = pods
    return snap


def alternating(n_its, classes=2, n_pods=12, daemons=()):
    """n_pods big pods of `classes` request classes (0, 1, 2 VENDOR units) in turn."""
    return snapshot([big_pod(i, i % classes) for i in range(n_pods)], big_its(n_its), daemons=daemons)


def daemon():
    d = synth.pod(100000, cpu="500m", mem="64Mi")
    d["spec"]["tolerations"] = [{"operator": "Exists"}]
    return d


def small_alternating(templates, n_pods=40, unfit=0):
    """Small pods of classes 0 / 1 VENDOR units in turn on one-pod instance types; `unfit` more that nothing holds."""
    pods = [small_pod(i, i % 2) for i in range(n_pods)]
    pods += [synth.pod(1000 + k, cpu="1000", mem="256Mi") for k in range(unfit)]
    return snapshot(pods, one_pod_its(), templates)


def front_without_offering():
    """The largest instance type -- the only member of the template's Pareto front -- offers spot in zone 1 and
    on-demand in zone 2; the template wants on-demand in zone 1.  Zone and capacity type both intersect, no offering
    has both: the type leaves every NodeClaim's options on the offering test alone, and the record's front flag is
    false."""
    snap = synth.benchmark_snapshot(300, 20, 5, diverse=False)
    p = snap["instanceTypes"][-1]["offerings"][0]["price"]
    snap["instanceTypes"][-1] = synth.fake_instance_type("fake-it-19", 20, 40, pods=200, offerings=[
        {"capacityType": "spot", "zone": "test-zone-1", "price": p, "available": True},
        {"capacityType": "on-demand", "zone": "test-zone-2", "price": p, "available": True}])
    snap["nodeClaimTemplates"] = [synth.node_pool("default-pool", requirements=[
        {"key": synth.ZONE, "operator": "In", "values": ["test-zone-1"]},
        {"key": synth.CT, "operator": "In", "values": ["on-demand"]}])]
    return snap


def all_distinct(n=40):
    """n pods, no two with the same requests: n request classes (2 to 5.9 cpu on instance types of up to 20)."""
    pods = [synth.pod(i, cpu="%dm" % (2000 + 100 * i), mem="128Mi") for i in range(n)]
    return snapshot(pods, synth.fake_instance_types(20))


def pods_only(n=30):
    """Pods without requests: the only live resource is the pod count (R = 1, the generic instantiation)."""
    return snapshot([synth.pod(i) for i in range(n)], synth.fake_instance_types(8))


def more_resources(k):
    """150 pods x 20 instance types with k more live resource names: R = 3 + k."""
    return resource_cases.with_resources(synth.benchmark_snapshot(150, 20, 11, diverse=False), k, 17)


NONINLINE_BUDGET = 14000


def non_inline(plan):
    """More NodeClaims than the plan keeps in LDS (KL) and no more than it has positions for (KO), at the reduced
    lds_budget of the re-plan ladder's tests: the claims past KL live in HBM.  plan: ks_problem_inspect's plan of this
    shape at NONINLINE_BUDGET."""
    assert plan["KL"] + 2 <= plan["KO"], plan
    return replan_cases.lean_base(min(plan["KL"] + 6, plan["KO"]))


def non_inline_shape():
    return replan_cases.lean_base(300)


LIMIT_2 = (("limited-pool", [], {"cpu": "12"}, None), ("open-pool", [], None, None))
LIMIT_3 = (("limited-pool", [], {"cpu": "12"}, None), ("small-pool", SMALL, None, None), ("open-pool", [], None, None))
NO_FIT = (("small-pool", SMALL, None, None), ("open-pool", [], None, None))
TAINTED = (("tainted-pool", [], None, [{"key": "dedicated", "value": "infra", "effect": "NoSchedule"}]),
           ("open-pool", [], None, None))

# name -> (builder, expectations).  R: live resources; lean: the LEAN Solve runs it (R 3 or 4); claims / errors: the
# oracle's counts; alternate: consecutive opening pods differ in request class (every open misses the memo); limited:
# the first template has a NodePool limit and takes that many NodeClaims; pools: NodeClaims per template.
CASES = {}
for _n in IT_EDGES:
    CASES["its_%d" % _n] = (lambda n=_n: alternating(n), dict(R=4, lean=True, claims=12, errors=0, alternate=True))
CASES.update({
    "three_classes": (lambda: alternating(33, classes=3), dict(R=4, lean=True, claims=12, errors=0, alternate=True)),
    "daemon": (lambda: alternating(33, daemons=[daemon()]), dict(R=4, lean=True, claims=12, errors=0, alternate=True)),
    "r1": (pods_only, dict(R=1, lean=False, claims=1, errors=0)),
    # C2's shape small, as in test_claim_run_cross_gpu.py: at 700 pods x 60 types no open repeats the last one's key
    # (tests/golden/lean_step_counters.json pins tplMemoHits 0 there), at 600 x 8 both kinds of open occur (32 of 56)
    "r3_cross_11": (lambda: synth.benchmark_snapshot(700, 60, 42, diverse=False), dict(R=3, lean=True, claims=11, errors=0)),
    "r3_mixed": (lambda: synth.benchmark_snapshot(600, 8, 3, diverse=False), dict(R=3, lean=True, claims=56, errors=0,
                                                                                 memo=32)),
    "r5": (lambda: more_resources(2), dict(R=5, lean=False, errors=0)),
    "r16": (lambda: more_resources(13), dict(R=16, lean=False, errors=0)),
    "limit_2": (lambda: small_alternating(LIMIT_2), dict(R=4, lean=True, claims=40, errors=0, limited=True,
                                                          pools={"limited-pool": 2, "open-pool": 38})),
    "limit_3": (lambda: small_alternating(LIMIT_3), dict(R=4, lean=True, claims=40, errors=0, limited=True,
                                                          pools={"limited-pool": 2, "small-pool": 18, "open-pool": 20})),
    "no_fit": (lambda: small_alternating(NO_FIT, unfit=2), dict(R=4, lean=True, claims=40, errors=2, alternate=True,
                                                                 pools={"small-pool": 20, "open-pool": 20})),
    "taint": (lambda: small_alternating(TAINTED), dict(R=4, lean=True, claims=40, errors=0, alternate=True,
                                                       pools={"open-pool": 40})),
    "front_no_offering": (front_without_offering, dict(R=3, lean=True, claims=13, errors=0)),
    "all_distinct": (all_distinct, dict(R=3, lean=True, errors=0)),
})
NAMES = list(CASES)

_memo = {}


def snapshot_json(name):
    """The case's snapshot as JSON text, built once per process."""
    import json

    if name not in _memo:
        _memo[name] = json.dumps(CASES[name][0]())
    return _memo[name]


def oracle(name):
    """The oracle's canonical Results, computed once per process and shared by the tests."""
    import problems
    from oracle import bridge

    key = ("oracle", name)
    if key not in _memo:
        _memo[key] = problems.canonical(bridge.solve(snapshot_json(name))[0])
    return _memo[key]


def request_class(pod):
    """The pod's request vector as a hashable key (the encoder's classes, up to renaming)."""
    return tuple(sorted(pod["spec"]["containers"][0]["resources"].get("requests", {}).items()))
