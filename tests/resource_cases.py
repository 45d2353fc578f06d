"""Generators and the case table of the k_solve route matrix (tests/test_route_matrix_gpu.py, checked on the CPU by
tests/test_route_preconditions.py).

k_solve is instantiated per (family, RT, TL, LEAN): RT is the live-resource count R when it is 3 or 4 and 0 (the
generic code) otherwise, and R counts the resource names some pod, daemon or NodePool limit mentions.  The random
problems of the suite have R = 4 and the clusters R = 3, so these generators add resource names that somebody
requests (with_resources, with_cluster_resources), take names away (no_requests, cpu_only, drop_gpu) and make a
request negative (negative_request).  Every added name is requested by at least one pod, so it is live, and sized so
that it decides placements: the same snapshot without those requests (strip_requests) gets another answer from the
oracle, which test_route_preconditions.py asserts for every case."""
import copy

import numpy as np

import problems
from karpenter_amd import synth

# ephemeral-storage and hugepages-2Mi are byte quantities, the rest plain counts
EXTRA_NAMES = ["ephemeral-storage", "hugepages-2Mi"] + ["example.com/res-%02d" % k for k in range(14)]
_UNIT = {"ephemeral-storage": "Gi", "hugepages-2Mi": "Mi"}


def _q(name, units):
    return "%d%s" % (units, _UNIT.get(name, ""))


def _pod_lists(snap):
    """Every list of pods that are scheduled or simulated (not clusterPods: cluster_snapshot lists the bound pods
    there too, as the same objects)."""
    out = [snap.get("pods", []), snap.get("pendingPods", [])]
    out += [n.get("pods", []) for n in snap.get("stateNodes", [])]
    return out


def _requests(p):
    return p["spec"]["containers"][0]["resources"].setdefault("requests", {})


def _sync_cluster_pods(snap):
    """clusterPods entries follow their bound pods (matched by uid) after a deepcopy or an edit."""
    if not snap.get("clusterPods"):
        return
    by_uid = {p["metadata"]["uid"]: p for lst in _pod_lists(snap) for p in lst if p["metadata"].get("uid")}
    snap["clusterPods"] = [by_uid.get(p["metadata"].get("uid") or "", p) for p in snap["clusterPods"]]


def with_resources(snap, k, seed, share=0.5):
    """A Solve snapshot with k more live resource names: capacity on every instance type (growing with its cpu)
    and node (capacity and a part of it available), requested by `share` of the pods, 1 to 3 names each; pod j < k
    always requests name j, so all k are live.  Sizes: a type of c cpus has 3c units, a pod asks for 1 to 6."""
    snap = copy.deepcopy(snap)
    rng = np.random.default_rng(seed)
    names = EXTRA_NAMES[:k]
    for it in snap["instanceTypes"]:
        c = int(it["capacity"]["cpu"])
        for n in names:
            it["capacity"][n] = _q(n, 3 * c)
    for node in snap["stateNodes"]:
        c = int(node["capacity"]["cpu"])
        for n in names:
            node["capacity"][n] = _q(n, 3 * c)
            node["available"][n] = _q(n, int(rng.integers(0, 3 * c + 1)))
    for j, p in enumerate(snap["pods"]):
        want = []
        if j < k:
            want.append(names[j])
        if rng.random() < share:
            want += [names[int(i)] for i in rng.choice(k, size=min(k, int(rng.integers(1, 4))), replace=False)]
        for n in want:
            _requests(p)[n] = _q(n, int(rng.integers(1, 7)))
    return snap


def _cluster_units(j, cpus):
    """Units of extra name j on an instance type: 2 per cpu for the two byte quantities, 1 per 2 cpus (at least 1)
    for the counted ones, so those stay scarce however many names share the pods' requests."""
    return 2 * cpus if j < 2 else max(1, cpus // 2)


def with_cluster_resources(snap, k, seed, share=0.6):
    """synth.cluster_snapshot output with k more live names: an instance type of c cpus has 2c units of the first two
    names and c / 2 of the others (_cluster_units); `share` of the bound pods ask for 1 to 4 units of 1 or 2 names (up
    to k / 2 + 1 when k is large), only while their node has them left, and every pending pod for one name; each
    node's available is its capacity minus what its own pods request.  The first k bound pods request name j each,
    so all k are live."""
    snap = copy.deepcopy(snap)
    rng = np.random.default_rng(seed)
    names = EXTRA_NAMES[:k]
    cpus = {}
    for it in snap["instanceTypes"]:
        c = cpus[it["name"]] = int(it["capacity"]["cpu"])
        for j, n in enumerate(names):
            it["capacity"][n] = _q(n, _cluster_units(j, c))
    forced = 0
    for node in snap["stateNodes"]:
        c = cpus[node["labels"][synth.IT_LABEL]]
        total = {n: _cluster_units(j, c) for j, n in enumerate(names)}
        left = dict(total)
        for p in node["pods"]:
            want = []
            if forced < k:
                want.append(names[forced])
                forced += 1
            if rng.random() < share:
                want += [names[int(i)] for i in rng.choice(k, size=min(k, int(rng.integers(1, max(3, k // 2 + 2)))),
                                                           replace=False)]
            for n in want:
                u = min(int(rng.integers(1, 5)), left[n])
                if u > 0:
                    _requests(p)[n] = _q(n, u)
                    left[n] -= u
        for n in names:
            node["capacity"][n] = _q(n, total[n])
            node["available"][n] = _q(n, left[n])
    for p in snap.get("pendingPods", []):
        n = names[int(rng.integers(k))]
        _requests(p)[n] = _q(n, int(rng.integers(1, 5)))
    _sync_cluster_pods(snap)
    return snap


def strip_requests(snap, names=None):
    """The same snapshot with the pods' requests of `names` (default: every EXTRA_NAMES entry) removed; capacities
    and availabilities stay.  What a case's answer is compared with to show that the names bind."""
    snap = copy.deepcopy(snap)
    names = set(EXTRA_NAMES if names is None else names)
    for lst in _pod_lists(snap):
        for p in lst:
            req = _requests(p)
            for n in names & set(req):
                del req[n]
    _sync_cluster_pods(snap)
    return snap


def drop_gpu(snap):
    """R = 3 from problems.random_problem's R = 4: nobody requests example.com/gpu."""
    return strip_requests(snap, ["example.com/gpu"])


def _only(snap, keep):
    snap = copy.deepcopy(snap)
    for lst in _pod_lists(snap) + [snap.get("daemonSetPods", [])]:
        for p in lst:
            for c in p["spec"]["containers"] + p["spec"].get("initContainers", []):
                req = c.get("resources", {}).get("requests")
                if req is not None:
                    for n in set(req) - set(keep):
                        del req[n]
    for pool in snap.get("nodePools", []) + snap.get("nodeClaimTemplates", []):
        lim = pool["spec"].get("limits")
        if lim:
            pool["spec"]["limits"] = {n: v for n, v in lim.items() if n in keep}
    for node in snap["stateNodes"]:
        node["daemonSetRequests"] = {n: v for n, v in node.get("daemonSetRequests", {}).items() if n in keep}
    _sync_cluster_pods(snap)
    return snap


def no_requests(snap):
    """R = 1: no pod or daemon requests anything and no NodePool limit names a resource; only `pods` is live."""
    return _only(snap, ())


def cpu_only(snap):
    """R = 2: cpu and pods."""
    return _only(snap, ("cpu",))


def negative_request(snap, pods=(3,), value="-500m"):
    """The cpu request of the given pods (indices into the Solve's pods, or into the cluster's pending + bound pods
    in node order) set below zero: dims.negReq, which turns off the threshold filter's sorted lists (Plan::tsort)
    and a Solve's live node list."""
    snap = copy.deepcopy(snap)
    flat = [p for lst in _pod_lists(snap) for p in lst]
    for i in pods:
        _requests(flat[i])["cpu"] = value
    _sync_cluster_pods(snap)
    return snap


def zero_negative(snap):
    """negative_request's stripped variant: the negative cpu requests set to 0."""
    snap = copy.deepcopy(snap)
    for lst in _pod_lists(snap):
        for p in lst:
            if str(_requests(p).get("cpu", "")).startswith("-"):
                _requests(p)["cpu"] = "0"
    _sync_cluster_pods(snap)
    return snap


def lean_extra(snap, name="ephemeral-storage"):
    """benchmark_snapshot with one more name on every pod (R = 4, still resource-only): fake instance type i has
    3 (i + 1) Gi, every pod asks for 1 to 6 Gi by its index."""
    snap = copy.deepcopy(snap)
    for it in snap["instanceTypes"]:
        it["capacity"][name] = _q(name, 3 * int(it["capacity"]["cpu"]))
    for j, p in enumerate(snap["pods"]):
        _requests(p)[name] = _q(name, 1 + (j * 7) % 6)
    return snap


# ---- the case table ------------------------------------------------------------------------------------------
# A cell is the k_solve instantiation a launch must report: (family, rt, tl, lean).  Every case names the cell(s)
# its launches must hit, in order for a Solve (a re-planned Solve launches twice); a consolidation pass may launch
# its cell more than once (a topology plan launches in two phases) but nothing else.

def _solve_base(seed, topo=False, big=False):
    if big:  # claims spill past Plan::KL at the reduced budgets (tests/test_solve_gpu.py's small-LDS shape)
        return problems.random_problem(seed, n_pods=120 if topo else 400, n_its=30, n_nodes=5, topology=topo,
                                       affinity=topo)
    return problems.random_problem(seed, n_pods=120 if not topo else 150, n_nodes=8, topology=topo, affinity=topo)


def _lean_base(seed, literal=False, push_back=False):
    snap = synth.benchmark_snapshot(600 if literal else 300, 60, seed, diverse=False, literal=literal)
    if push_back:  # pods too large for every instance type are pushed back: shared UIDs then leave the LEAN kernel
        for k in range(3):
            big = synth.pod(900000 + k, cpu="1000", mem="1Gi")
            big["metadata"].pop("uid", None)
            snap["pods"].insert(100 * (k + 1), big)
    return snap


def _cluster(seed, topo=0, sel=False, n_its=60, ppn=10, it_range=(6, 30), limits=None):
    return synth.cluster_snapshot(24, ppn, n_its=n_its, it_range=it_range, seed=seed, n_pending=3, topology=topo,
                                  pod_selectors=sel, limits=limits)


# A negative request decides something only where pods are retried: NewQueue orders pods by cpu descending, so the
# negative ones come last, and a NodeClaim's options only ever shrink.  Under a NodePool cpu limit that stops some
# replacements, pods that found no room are retried after the negative ones made some on the remaining nodes.
_NEG_PODS = (0, 5, 17, 33, 52, 71, 100, 130, 160, 200)
_NEG_LIMIT = {(0, 4): "200", (0, 5): "150", (1, 4): "300", (1, 5): "300"}


def _volume_cluster(seed, k):
    snap = synth.cluster_snapshot(14, 4, n_its=40, it_range=(4, 20), seed=seed, n_pending=2, topology=6)
    snap = with_cluster_resources(snap, k, seed)
    pods = snap["pendingPods"] + [p for n in snap["stateNodes"] for p in n["pods"]]
    snap["volumeDrivers"] = problems.add_volumes(np.random.default_rng(seed), pods, snap["stateNodes"])
    return snap


def _carry_cluster(seed, k):
    import carry_scenarios as cs

    return with_cluster_resources(cs.random_cluster(seed, topology=True), k, seed)


def _case(name, kind, make, cells, R, strip=None, budget=0, neg=False, topo=False, env=None, small_lds=False,
          reruns=False, degenerate_ok=False):
    return dict(name=name, kind=kind, make=make, cells=cells, R=R, strip=strip, budget=budget, neg=neg, topo=topo,
                env=env or {}, small_lds=small_lds, reruns=reruns, degenerate_ok=degenerate_ok)


def _solve_cases():
    S, T = "solve", "solve_topo"
    sr = strip_requests
    out = [
        # --- Solve, no topology
        _case("solve-rt3-lean", "solve", lambda: _lean_base(7), [(S, 3, 1, 1)], 3, degenerate_ok=True),
        _case("solve-rt3-lean-exit", "solve", lambda: _lean_base(441, True, True), [(S, 3, 1, 1), (S, 3, 1, 0)], 3,
              degenerate_ok=True),
        _case("solve-rt3-tl", "solve", lambda: drop_gpu(_solve_base(14)), [(S, 3, 1, 0)], 3),
        _case("solve-rt3-notl", "solve", lambda: drop_gpu(_solve_base(203, big=True)), [(S, 3, 0, 0)], 3, budget=9000,
              small_lds=True),
        _case("solve-rt4-lean", "solve", lambda: lean_extra(_lean_base(7)), [(S, 4, 1, 1)], 4, strip=sr,
              degenerate_ok=True),
        _case("solve-rt4-lean-exit", "solve", lambda: lean_extra(_lean_base(441, True, True)),
              [(S, 4, 1, 1), (S, 4, 1, 0)], 4, strip=sr, degenerate_ok=True),
        _case("solve-rt4-tl", "solve", lambda: _solve_base(14), [(S, 4, 1, 0)], 4, strip=drop_gpu),
        _case("solve-rt4-notl", "solve", lambda: _solve_base(242, big=True), [(S, 4, 0, 0)], 4, budget=9000,
              small_lds=True),
        _case("solve-rt0-tl-R5", "solve", lambda: with_resources(_solve_base(11), 1, 1), [(S, 0, 1, 0)], 5, strip=sr),
        _case("solve-rt0-tl-R8", "solve", lambda: with_resources(_solve_base(14), 4, 2), [(S, 0, 1, 0)], 8, strip=sr),
        _case("solve-rt0-tl-R16", "solve", lambda: with_resources(_solve_base(17), 12, 3), [(S, 0, 1, 0)], 16, strip=sr),
        _case("solve-rt0-notl-R5", "solve", lambda: with_resources(_solve_base(203, big=True), 1, 4), [(S, 0, 0, 0)], 5,
              strip=sr, budget=14000, small_lds=True),
        _case("solve-rt0-notl-R16", "solve", lambda: with_resources(_solve_base(203, big=True), 12, 5), [(S, 0, 0, 0)],
              16, strip=sr, budget=40000, small_lds=True),
        _case("solve-rt0-R1", "solve", lambda: no_requests(_solve_base(11)), [(S, 0, 1, 0)], 1),
        _case("solve-rt0-R2", "solve", lambda: cpu_only(_solve_base(14)), [(S, 0, 1, 0)], 2),
        _case("solve-neg-R4", "solve", lambda: negative_request(_solve_base(14), (3, 40, 77)), [(S, 4, 1, 0)], 4,
              strip=zero_negative, neg=True),
        _case("solve-neg-R5", "solve", lambda: negative_request(with_resources(_solve_base(11), 1, 1), (3, 40, 77)),
              [(S, 0, 1, 0)], 5, strip=zero_negative, neg=True),
        # --- Solve + topology
        _case("topo-rt3-tl", "solve", lambda: drop_gpu(_solve_base(27, True)), [(T, 3, 1, 0)], 3, topo=True),
        _case("topo-rt3-notl", "solve", lambda: drop_gpu(_solve_base(203, True, True)), [(T, 3, 0, 0)], 3, topo=True,
              budget=9000),
        _case("topo-rt4-tl", "solve", lambda: _solve_base(27, True), [(T, 4, 1, 0)], 4, topo=True, strip=drop_gpu),
        _case("topo-rt4-notl", "solve", lambda: _solve_base(203, True, True), [(T, 4, 0, 0)], 4, topo=True, budget=9000),
        _case("topo-rt0-tl-R5", "solve", lambda: with_resources(_solve_base(35, True), 1, 6), [(T, 0, 1, 0)], 5,
              topo=True, strip=sr),
        _case("topo-rt0-tl-R8", "solve", lambda: with_resources(_solve_base(27, True), 4, 7), [(T, 0, 1, 0)], 8,
              topo=True, strip=sr),
        _case("topo-rt0-tl-R16", "solve", lambda: with_resources(_solve_base(35, True), 12, 8), [(T, 0, 1, 0)], 16,
              topo=True, strip=sr),
        _case("topo-rt0-notl-R5", "solve", lambda: with_resources(_solve_base(203, True, True), 1, 9), [(T, 0, 0, 0)], 5,
              topo=True, strip=sr, budget=14000),
        _case("topo-rt0-notl-R16", "solve", lambda: with_resources(_solve_base(203, True, True), 12, 10),
              [(T, 0, 0, 0)], 16, topo=True, strip=sr, budget=40000),
        _case("topo-rt0-R1", "solve", lambda: no_requests(_solve_base(27, True)), [(T, 0, 1, 0)], 1, topo=True),
        _case("topo-rt0-R2", "solve", lambda: cpu_only(_solve_base(35, True)), [(T, 0, 1, 0)], 2, topo=True),
        _case("topo-neg-R4", "solve", lambda: negative_request(_solve_base(27, True), (3, 40, 77)), [(T, 4, 1, 0)], 4,
              topo=True, strip=zero_negative, neg=True),
        _case("topo-neg-R5", "solve", lambda: negative_request(with_resources(_solve_base(35, True), 1, 6), (3, 40, 77)),
              [(T, 0, 1, 0)], 5, topo=True, strip=zero_negative, neg=True),
    ]
    return out


# The instance types that take a cluster's tables out of the simulations' LDS plan (simPlan.talloc == 0), by
# (topology, R): the smallest count on a grid of 50 (the tables cost about 20 bytes x instance types x R against a
# 40 KiB budget, 64 KiB with topology).  These clusters run 5 pods per node, which keeps the oracle under 2 s.
NOTL_ITS = {(0, 3): 500, (0, 4): 350, (0, 5): 300, (0, 16): 100, (1, 3): 800, (1, 4): 600, (1, 5): 450, (1, 16): 100}


def _cons_cases():
    out = []
    wcr = with_cluster_resources
    sr = strip_requests
    for topo, fam, tag, t in ((0, "sims", "sims", 0), (6, "sims_topo", "simstopo", 1)):
        def C(seed, topo=topo, **kw):  # (topology clusters run 5 pods per node: the oracle needs 3x as long there)
            kw.setdefault("ppn", 5 if topo else 10)
            return _cluster(seed, topo=topo, **kw)

        lean = 0 if topo else 1
        out += [
            _case(tag + "-rt3-tl", "cons", lambda C=C, t=t: C(31, sel=True), [(fam, 3, 1, 0)], 3, topo=bool(topo)),
            _case(tag + "-rt3-notl", "cons", lambda C=C, t=t: C(32, n_its=NOTL_ITS[(t, 3)], ppn=5), [(fam, 3, 0, 0)], 3, topo=bool(topo)),
            _case(tag + "-rt4-tl", "cons", lambda C=C, t=t: wcr(C(33, sel=True), 1, 1), [(fam, 4, 1, 0)], 4, strip=sr,
                  topo=bool(topo)),
            _case(tag + "-rt4-notl", "cons", lambda C=C, t=t: wcr(C(34, n_its=NOTL_ITS[(t, 4)], ppn=5), 1, 2), [(fam, 4, 0, 0)], 4, strip=sr,
                  topo=bool(topo)),
            _case(tag + "-rt0-tl-R5", "cons", lambda C=C, t=t: wcr(C(35, ppn=10), 2, 3), [(fam, 0, 1, 0)], 5, strip=sr, topo=bool(topo)),
            _case(tag + "-rt0-tl-R8", "cons", lambda C=C, t=t: wcr(C(36, ppn=10), 5, 4), [(fam, 0, 1, 0)], 8, strip=sr, topo=bool(topo)),
            _case(tag + "-rt0-tl-R16", "cons", lambda C=C, t=t: wcr(C(37, n_its=20, it_range=(4, 20)), 13, 5), [(fam, 0, 1, 0)], 16, strip=sr,
                  topo=bool(topo)),
            _case(tag + "-rt0-notl-R5", "cons", lambda C=C, t=t: wcr(C(38, n_its=NOTL_ITS[(t, 5)], ppn=5), 2, 6), [(fam, 0, 0, 0)], 5,
                  strip=sr, topo=bool(topo)),
            _case(tag + "-rt0-notl-R16", "cons", lambda C=C, t=t: wcr(C(39, n_its=NOTL_ITS[(t, 16)], ppn=5), 13, 7), [(fam, 0, 0, 0)], 16,
                  strip=sr, topo=bool(topo)),
            _case(tag + "-rt0-R1", "cons", lambda C=C, t=t: no_requests(C(40)), [(fam, 0, 1, 0)], 1, topo=bool(topo),
                  degenerate_ok=True),
            _case(tag + "-rt0-R2", "cons", lambda C=C, t=t: cpu_only(C(41)), [(fam, 0, 1, 0)], 2, topo=bool(topo)),
            _case(tag + "-neg-R4", "cons", lambda C=C, t=t: negative_request(wcr(C(42, limits={"cpu": _NEG_LIMIT[(t, 4)]}, ppn=10), 1, 8), _NEG_PODS, "-20"),
                  [(fam, 4, 1, 0)], 4, strip=zero_negative, neg=True, topo=bool(topo)),
            _case(tag + "-neg-R5", "cons", lambda C=C, t=t: negative_request(wcr(C(42, limits={"cpu": _NEG_LIMIT[(t, 5)]}, ppn=10), 2, 8), _NEG_PODS, "-20"),
                  [(fam, 0, 1, 0)], 5, strip=zero_negative, neg=True, topo=bool(topo)),
        ]
        if not topo:
            out += [
                _case("sims-rt3-lean", "cons", lambda C=C, t=t: C(30), [(fam, 3, 1, 1)], 3),
                _case("sims-rt4-lean", "cons", lambda C=C, t=t: wcr(C(33), 1, 1), [(fam, 4, 1, 1)], 4, strip=sr),
            ]
    out += [
        _case("simstopo-volumes-R5", "cons", lambda: _volume_cluster(45, 2), [("sims_topo", 0, 1, 0)], 5, strip=sr,
              topo=True),
        _case("simstopo-carry-R5", "cons", lambda: _carry_cluster(6, 3), [("sims_topo", 0, 1, 0)], 5, strip=sr, topo=True,
              reruns=True),
        # multi-wave (KS_SIM_MW=1, KS_SIM_MW_MIN=1): one mixed launch; rt = 3 is tests/test_cons_mw_gpu.py's
        _case("mixed-rt4", "cons", lambda: wcr(_cluster(33), 1, 1), [("sims_mixed", 4, 1, 1)], 4, strip=sr,
              env={"KS_SIM_MW": "1", "KS_SIM_MW_MIN": "1"}),
    ]
    return out


SOLVE_CASES = _solve_cases()
CONS_CASES = _cons_cases()
CASES = {c["name"]: c for c in SOLVE_CASES + CONS_CASES}
assert len(CASES) == len(SOLVE_CASES) + len(CONS_CASES)

_cache = {}


def snapshot(name):
    """The case's snapshot as JSON text (built once per process)."""
    import json

    if name not in _cache:
        _cache[name] = json.dumps(CASES[name]["make"]())
    return _cache[name]


def stripped(name):
    import json

    c = CASES[name]
    return None if c["strip"] is None else json.dumps(c["strip"](json.loads(snapshot(name))))


_oracle = {}


def oracle(name, all_sims=True):
    """The oracle's answer (computed once per process): canonical Results of a Solve case, the consolidation
    document of a cluster case."""
    from oracle import bridge

    key = (name, all_sims)
    if key not in _oracle:
        if CASES[name]["kind"] == "solve":
            _oracle[key] = problems.canonical(bridge.solve(snapshot(name))[0])
        else:
            _oracle[key] = bridge.consolidate(snapshot(name), all_sims=all_sims)[0]
    return _oracle[key]
