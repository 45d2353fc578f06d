"""Generators and the case table of the NodeClaim-capacity re-plan ladder (tests/test_claim_cap_replan_gpu.py, checked
on the CPU by tests/test_claim_cap_plans.py).

A Solve that creates more NodeClaims than its LDS plan has positions for (Plan::KO) stops with KE_CLAIM_CAP; ks_solve
then re-plans (make_plan's wideKO level 1: 64 LDS-resident claims and the rest of the LDS to positions; level 2: the
instance-type tables leave the LDS as well), launches again and remembers the level on the handle.  At a reduced
lds_budget the capacities are small enough to cross with a few hundred pods.  K0, K1 and K2 below are the KO of levels
0, 1 and 2 at a case's budget as ks_problem_inspect reports them ("plans", "widePlans"); no case states one as a number.

The LEAN base: fake.InstanceTypes(8) (1 to 8 cpu), one template, n_big pods of 4 to 7 cpu, no two of which share an
8-cpu instance type (7.9 cpu allocatable), and 150 small pods that join them.  The oracle makes exactly one NodeClaim
per big pod, so a case chooses its claim count."""
import json

import numpy as np

import problems
from karpenter_amd import synth

S, T = "solve", "solve_topo"
CAPACITY = -3  # KS_ERR_CAPACITY

BIG_CPU = ["%dm" % c for c in range(4000, 7001, 500)]
BIG_MEM = ["512Mi", "1024Mi", "1536Mi", "2048Mi"]


RUN_PODS = 80


def lean_base(n_big, seed=5, n_same=0, n_small=150, run=False):
    """n_same of the big pods are identical (4000m, 512Mi).
    run: RUN_PODS identical pods of 7500m and 10Mi, popped first, and one more instance type that holds exactly
    those (601 cpu, 1Gi, RUN_PODS pods): they fill the first NodeClaim in one run that reaches past the 64-pod queue
    window, which the LEAN Solve logs as a record.  No two big pods fit that type's memory, so every big pod still
    opens a NodeClaim of its own: n_big + 1 claims."""
    snap = synth.benchmark_snapshot(0, 8, seed, diverse=False)
    rng = np.random.default_rng(seed)
    pods = []
    if run:
        snap["instanceTypes"].append(synth.fake_instance_type("fake-it-wide", 601, 1, pods=RUN_PODS))
        snap["instanceTypesByNodePool"]["default-pool"].append(8)
        pods = [synth.pod(100000 + i, cpu="7500m", mem="10Mi") for i in range(RUN_PODS)]
    for i in range(n_big):
        if i < n_same:
            pods.append(synth.pod(i, cpu=BIG_CPU[0], mem=BIG_MEM[0]))
        else:
            pods.append(synth.pod(i, cpu=BIG_CPU[int(rng.integers(len(BIG_CPU)))], mem=BIG_MEM[int(rng.integers(len(BIG_MEM)))]))
    for i in range(n_small):
        pods.append(synth.pod(n_big + i, cpu=synth.CPU_CHOICES[int(rng.integers(5))], mem=synth.MEM_CHOICES[int(rng.integers(4))]))
    snap["pods"] = [pods[int(i)] for i in rng.permutation(len(pods))]
    return snap


def lean_exit_base(n_big=230):
    """Shared UIDs and a NodePool cpu limit of 1300: the limit admits 162 NodeClaims of 8 cpu, after which pods are
    pushed back and the LEAN kernel leaves (KE_LEAN_EXIT) -- after the claim count has passed K0."""
    snap = lean_base(n_big)
    for i, p in enumerate(snap["pods"]):
        p["metadata"]["uid"] = "shared-%d" % (i % 25)
    snap["nodePools"] = [synth.node_pool("default-pool", limits={"cpu": "1300"})]
    return snap


def random_base(n_pods):
    return problems.random_problem(203, n_pods=n_pods, n_its=30, n_nodes=5)


def topo_base(n_anti=230, n_plain=100, n_zonal=6, n_its=100, seed=9):
    """G > 0: n_anti pods with required hostname anti-affinity on their own app label (one NodeClaim each, with a
    hostname placeholder), n_plain ordinary pods and a few pods with zonal spread; a Topology that is not empty."""
    snap = synth.benchmark_snapshot(0, n_its, seed, diverse=False)
    snap.pop("emptyTopology")
    rng = np.random.default_rng(seed)
    pods = []
    for i in range(n_anti):
        p = synth.pod(i, cpu=synth.CPU_CHOICES[int(rng.integers(5))], mem=synth.MEM_CHOICES[int(rng.integers(4))],
                      labels={"app": "anti"})
        p["spec"]["affinity"] = {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
            {"labelSelector": {"matchLabels": {"app": "anti"}}, "topologyKey": synth.HOSTNAME}]}}
        pods.append(p)
    for i in range(n_plain):
        pods.append(synth.pod(n_anti + i, cpu=synth.CPU_CHOICES[int(rng.integers(5))],
                              mem=synth.MEM_CHOICES[int(rng.integers(4))], labels={"app": "plain"}))
    for i in range(n_zonal):
        p = synth.pod(n_anti + n_plain + i, cpu="250m", mem="256Mi", labels={"app": "zonal"})
        p["spec"]["topologySpreadConstraints"] = [{"maxSkew": 1, "topologyKey": synth.ZONE, "whenUnsatisfiable": "DoNotSchedule",
                                                   "labelSelector": {"matchLabels": {"app": "zonal"}}}]
        pods.append(p)
    snap["pods"] = [pods[int(i)] for i in rng.permutation(len(pods))]
    return snap


# ---- the case table ------------------------------------------------------------------------------------------
# make(k): the snapshot, given k = (K0, K1, K2) of the case's shape at its budget: the LEAN cases choose their claim
# count from them, and `shape` builds a snapshot with the same plans (test_claim_cap_plans.py checks that they are the
# case's own); shape None: the plans are read from the case's snapshot, which does not depend on them.
# regime: the interval of the oracle's claim count, (lo, hi] as indices into k (None: open above) -- the launches follow
# from it: up to K0 one launch, up to K1 a second at level 1 (skipped where K1 <= K0), up to K2 one more at level 2.
# cells: every launch of a fresh handle's Solve, in order, as (family, rt, tl, lean); wide: the last launch's level;
# error: the Solve fails with KS_ERR_CAPACITY naming k[error].

def _case(name, shape, make, budget, regime, cells, wide, lean, topo=False, error=None, errors=False, claims=None):
    return dict(name=name, shape=shape, make=make, budget=budget, regime=regime, cells=cells, wide=wide, lean=lean, topo=topo,
                error=error, errors=errors, claims=claims)


def _lean_shape():
    return lean_base(300)  # (Kcap is the pod count: above every level's KO here, as in the cases themselves)


L, X, N = (S, 3, 1, 1), (S, 3, 1, 0), (S, 3, 0, 0)

CASE_LIST = [
    # --- LEAN, R = 3, budget 14000: K0 < K1 < K2
    _case("lean-K0", _lean_shape, lambda k: lean_base(k[0]), 14000, (None, 0), [L], 0, 1),
    _case("lean-K0+1", _lean_shape, lambda k: lean_base(k[0] + 1), 14000, (0, 1), [L, L], 1, 1),
    _case("lean-K1", _lean_shape, lambda k: lean_base(k[1]), 14000, (0, 1), [L, L], 1, 1),
    _case("lean-K1+1", _lean_shape, lambda k: lean_base(k[1] + 1), 14000, (1, 2), [L, L, N], 2, 1),
    _case("lean-K2", _lean_shape, lambda k: lean_base(k[2]), 14000, (1, 2), [L, L, N], 2, 1),
    _case("lean-K2+1", _lean_shape, lambda k: lean_base(k[2] + 1), 14000, (2, None), [L, L, N], 2, 1, error=2),
    # 60 identical pods among the big ones, and a run past the queue window (lean_base) that logs a run record at the
    # start of the attempt that ends in KE_CLAIM_CAP; K0 + 1 claims
    _case("lean-runs", lambda: lean_base(300, run=True), lambda k: lean_base(k[0], n_same=60, run=True), 14000, (0, 1),
          [L, L], 1, 1),
    # KE_CLAIM_CAP at the (K0 + 1)-th claim, the wide LEAN launch, KE_LEAN_EXIT at the first push-back under shared
    # UIDs (the limit admits 162 claims > K0), then the non-LEAN instantiation with the wide plan (ks_solve's loop:
    # a lean exit keeps the plan, a claim-cap exit keeps the instantiation)
    _case("lean-exit", _lean_shape, lambda k: lean_exit_base(), 14000, (0, 1), [L, L, X], 1, 1, errors=True, claims=162),
    # --- the LEAN base at 6000 (tables in HBM, so not the LEAN kernel): K1 and K2 are below K0, no level raises KO
    _case("lean-no-raise", _lean_shape, lambda k: lean_base(k[0] + 1), 6000, (0, None), [N], 0, 1, error=0),
    # --- random problems, R = 4, not lean
    # 14000: K1 < K0 < K2, level 1 is skipped
    _case("rt4-skip-1", None, lambda k: random_base(500), 14000, (0, 2), [(S, 4, 1, 0), (S, 4, 0, 0)], 2, 0,
          errors=True),
    # --- topology, budget 24000
    _case("topo", None, lambda k: topo_base(), 24000, (0, 1), [(T, 3, 1, 0), (T, 3, 1, 0)], 1, 0,
          topo=True),
]
CASES = {c["name"]: c for c in CASE_LIST}
assert len(CASES) == len(CASE_LIST)
NAMES = [c["name"] for c in CASE_LIST]

_memo = {}


def _once(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def levels(doc, budget):
    """The plans of levels 0, 1 and 2 at `budget` from an inspect document."""
    return [doc["plans"][str(budget)]] + list(doc["widePlans"][str(budget)])


def ks(name):
    """(K0, K1, K2) of the case's shape at its budget."""
    from karpenter_amd import inspect

    c = CASES[name]
    shape = (lambda: json.dumps(c["shape"]())) if c["shape"] else (lambda: snapshot(name))
    return _once(("ks", name), lambda: tuple(pl["KO"] for pl in levels(inspect(shape()), c["budget"])))


def snapshot(name):
    """The case's snapshot as JSON text (built once per process)."""
    c = CASES[name]
    return _once(("snap", name), lambda: json.dumps(c["make"](ks(name) if c["shape"] else None)))


def oracle(name):
    """The oracle's canonical Results (computed once per process) and the seconds it took."""
    import time

    from oracle import bridge

    def run():
        t = time.perf_counter()
        want = problems.canonical(bridge.solve(snapshot(name))[0])
        return want, time.perf_counter() - t

    return _once(("oracle", name), run)


def ladder(k, claims):
    """ks_solve's re-plan loop on a fresh handle, from the capacities alone: the levels it launches for a Solve of
    `claims` NodeClaims (level 0, then every level that raises KO while the claims exceed it) and whether the last
    one holds them."""
    out, top = [0], k[0]
    for level in (1, 2):
        if claims > top and k[level] > top:
            out.append(level)
            top = k[level]
    return out, claims <= top
