"""Problems and the oracle protocol for the static feasibility matrix ("Static feasibility
matrix"; Scheduler.static_feasibility).

The problems carry no topology terms, no volume limits and no negative requests, so the matrix's definitions are
exact for them: a set bit is what the reference does for that pod alone.

Oracle protocol (oracle/bridge.py as it stands; nothing here reads the library's encoding):

  templates   for pod p and template t, the oracle solves the snapshot reduced to that pod, that NodePool with its
              instance types, the DaemonSet pods and no state nodes.  It schedules the pod iff some state of p's chain
              has options in row (s, t); the claim's instanceTypeOptions equal the row of the first such state; for a
              single-state pod that fails, its message falls in the class of the row's code.
  nodes       for pod p and node n, the oracle solves the snapshot reduced to that pod and that node with no
              NodePools (the oracle accepts a snapshot without one).  It places the pod on the node iff some state's
              bit n is set; for a single-state pod that is bit (state0, n).

The template problems have no state nodes (a NodePool's remaining limits subtract its nodes' capacity, which the
reduced snapshot would lose); the node problems' single NodePool has no limit and no node carries a
PreferNoSchedule taint (the relaxation that tolerates them exists only while a NodePool has such a taint, which the
node protocol's snapshot has not)."""
import functools
import json
import os
import subprocess

import numpy as np

import feasibility_cases as fc
import problems
from karpenter_amd import synth

GPU = "example.com/gpu"
FPGA = "example.com/fpga"
DAEMON_CPU_M = 100
TOL_SPOTTY = {"key": "spotty", "operator": "Exists", "effect": "PreferNoSchedule"}


def _daemon():
    d = synth.pod(100000, cpu="%dm" % DAEMON_CPU_M, mem="64Mi")
    d["spec"]["tolerations"] = [{"operator": "Exists"}]
    return d


def _requests(pod, **req):
    pod["spec"]["containers"][0]["resources"]["requests"] = dict(req)
    return pod


def _largest_alloc_cpu_m(its):
    """Allocatable cpu of the largest type in milli-CPU (capacity - kubeReserved 100m, fake/instancetype.go)."""
    return max(int(it["capacity"]["cpu"]) for it in its) * 1000 - 100


def _extra_pods(its, first):
    """Pods beyond fc.it_pods: In / NotIn on zone and on capacity type, and the two requests that decide Fits on
    their own (with the daemon overhead): one milli-CPU above the largest Allocatable, and exactly it."""
    edge = _largest_alloc_cpu_m(its) - DAEMON_CPU_M
    aff = fc._affinity
    pods = [
        synth.pod(first, cpu="100m", mem="64Mi", node_selector={synth.ZONE: "test-zone-3"}, tolerations=[fc.TOL_ALL]),
        synth.pod(first + 1, cpu="100m", mem="64Mi", tolerations=[fc.TOL_ALL], affinity=aff(
            [{"key": synth.ZONE, "operator": "NotIn", "values": ["test-zone-1", "test-zone-2"]},
             {"key": synth.CT, "operator": "In", "values": ["spot"]}])),
        synth.pod(first + 2, cpu="100m", mem="64Mi", tolerations=[fc.TOL_ALL], affinity=aff(
            [{"key": synth.CT, "operator": "NotIn", "values": ["on-demand"]}])),
        synth.pod(first + 3, cpu="100m", mem="64Mi", node_selector={synth.CT: "on-demand"}, tolerations=[fc.TOL_ALL]),
        _requests(synth.pod(first + 4, tolerations=[fc.TOL_ALL]), cpu="%dm" % (edge + 1), memory="64Mi"),
        _requests(synth.pod(first + 5, tolerations=[fc.TOL_ALL]), cpu="%dm" % edge, memory="64Mi"),
    ]
    return pods


def list_case(n_its, seed, limits=None):
    """One tainted template over n_its instance types (R = 3): fc.it_case's pods (In / NotIn / Exists /
    DoesNotExist / Gt / Lt on a single-valued key, with and without the toleration) plus _extra_pods, one DaemonSet
    pod for the overhead.  Offerings: every fifth type has its zone-3 offering unavailable, every seventh offers spot
    in zone 3 too (a zone x capacity-type pair only some types offer)."""
    snap = fc.it_case(n_its, min(n_its, 50), 16, seed, key=fc.INT)
    for i, it in enumerate(snap["instanceTypes"]):
        if i % 5 == 2:
            for o in it["offerings"]:
                if o["zone"] == "test-zone-3":
                    o["available"] = False
        if i % 7 == 3:
            it["offerings"].append({"capacityType": "spot", "zone": "test-zone-3", "price": it["offerings"][0]["price"],
                                    "available": True})
    snap["pods"] += _extra_pods(snap["instanceTypes"], len(snap["pods"]))
    snap["daemonSetPods"] = [_daemon()]
    if limits is not None:
        snap["nodeClaimTemplates"][0]["spec"]["limits"] = limits
    return snap


def three_template_case():
    """Three templates over lists of 40, 33 and 7 (TW = 2): one NoSchedule taint, one PreferNoSchedule (chains that
    only add that toleration), one untainted; a pod with OR'd required terms (a chain that drops them one by one)."""
    snap = fc.three_template_snapshot()
    n = len(snap["pods"])
    ints = fc._int_values(snap["instanceTypes"])
    por = synth.pod(n, cpu="100m", mem="64Mi", tolerations=[fc.TOL_GOLD])
    por["spec"]["affinity"] = {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
        {"matchExpressions": [{"key": fc.INT, "operator": "In", "values": ["4000"]}]},
        {"matchExpressions": [{"key": fc.INT, "operator": "In", "values": [ints[20]]}]},
        {"matchExpressions": [{"key": "size", "operator": "In", "values": ["large"]}]}]}}}
    snap["pods"].append(por)
    snap["pods"].append(synth.pod(n + 1, cpu="100m", mem="64Mi", tolerations=[fc.TOL_GOLD, TOL_SPOTTY],
                                  node_selector={synth.ZONE: "test-zone-3"}))
    snap["daemonSetPods"] = [_daemon()]
    return snap


def five_resource_case():
    """R = 5: cpu, memory, pods and two extended resources that only some of 33 types carry."""
    its = []
    for i in range(33):
        extra = {}
        if i % 3 == 0:
            extra[GPU] = str(1 + i % 4)
        if i % 11 == 5:
            extra[FPGA] = "1"
        its.append(synth.fake_instance_type("it-%04d" % i, 1 + i, 2 * (1 + i), pods=110, extra_capacity=extra or None))
    pool = synth.node_pool("pool-0")
    pods = []
    for i, req in enumerate([{"cpu": "1"}, {"cpu": "1", GPU: "1"}, {"cpu": "2", GPU: "4"}, {"cpu": "1", GPU: "5"},
                             {"cpu": "1", FPGA: "1"}, {"cpu": "30", FPGA: "1"}, {"cpu": "1", GPU: "1", FPGA: "1"},
                             {"cpu": "500m", "memory": "60Gi", GPU: "2"}, {"cpu": "40"}]):
        pods.append(_requests(synth.pod(i), **req))
    pods += _extra_pods(its, len(pods))
    snap = fc._snapshot(its, {"pool-0": list(range(33))}, [pool], [], pods)
    snap["daemonSetPods"] = [_daemon()]
    return snap


HP = [("", 80, "TCP"), ("10.0.0.1", 8080, "TCP"), ("", 53, "UDP")]


def _port(ip, port, proto):
    e = {"containerPort": port, "hostPort": port, "protocol": proto}
    if ip:
        e["hostIP"] = ip
    return e


def node_case(n_nodes, seed, n_pods=24):
    """n_nodes existing nodes (fc.make_nodes: a third tainted, some lacking the labels the pods name) and no usable
    template for most pods' sake; fc.node_pod's kinds, then pods that want a host port some nodes hold, and a pod
    that node 0 has room for exactly while nodes 1 .. 3 are one unit short in cpu, memory and pods in turn."""
    rng = np.random.default_rng(seed)
    its = fc.make_its(4, 4, irregular=False)
    pool = synth.node_pool("pool-0")
    nodes = fc.make_nodes(rng, n_nodes)
    for i, n in enumerate(nodes):
        if i % 4 == 1:
            ip, port, proto = HP[(i // 4) % len(HP)]
            n["hostPortUsage"] = {"default/bound-%d" % i: [{"ip": ip or "0.0.0.0", "port": port, "protocol": proto}]}
        if i % 5 == 2:
            n["daemonSetRequests"] = {"cpu": "250m"}
    exact = {"cpu": "1750m", "memory": "3Gi", "pods": "1"}
    for i, short in enumerate([None, ("cpu", "1749m"), ("memory", str(3 * synth.GI - 1)), ("pods", "0")]):
        if i < n_nodes:
            nodes[i]["available"] = dict(exact, **({short[0]: short[1]} if short else {}))
            nodes[i]["daemonSetRequests"] = {}
            nodes[i]["taints"] = []
    k = max(0, n_pods - 5)
    pods = [fc.node_pod(rng, i, n_nodes) for i in range(k)]
    for j, (ip, port, proto) in enumerate(HP):
        p = synth.pod(k + j, cpu="100m", mem="64Mi", tolerations=[fc.TOL_ALL])
        p["spec"]["containers"][0]["ports"] = [_port(ip, port, proto)]
        pods.append(p)
    pods.append(_requests(synth.pod(k + 3, tolerations=[fc.TOL_ALL]), cpu="1750m", memory="3Gi"))
    pods.append(_requests(synth.pod(k + 4, tolerations=[fc.TOL_ALL]), cpu="1750m", memory=str(3 * synth.GI + 1)))
    return fc._snapshot(its, {"pool-0": [0, 1, 2, 3]}, [pool], nodes, pods)


def negative_request_case():
    snap = list_case(7, 5)
    snap["pods"][0]["spec"]["containers"][0]["resources"]["requests"]["cpu"] = "-1"
    return snap


LIST_SIZES = (1, 31, 32, 33, 64, 65)            # TW 1, 1, 1, 2, 2, 3
NODE_SIZES = (1, 31, 32, 33, 63, 64, 65, 257)   # NWN 1 .. 9; ragged last words at 33, 65, 257; two blocks at 257
# NodePool limits over list_case(33): cpu capacities 1 .. 33, of which the NodePool's `special Exists` admits the
# large types only (cpu >= 5).  A limit equal to one type's capacity (cpu 5: that type is the one option, the test is
# <=), one unit below the smallest capacity (no candidate: FC_LIMITS), a strict subset of the candidates (cpu <= 8).
LIMITS = {"limit-one": {"cpu": "5"}, "limit-none": {"cpu": "999m"}, "limit-subset": {"cpu": "8"}}


@functools.lru_cache(maxsize=None)
def problem(name):
    if name.startswith("list-"):
        n = int(name[5:])
        return list_case(n, 400 + n)
    if name.startswith("limit-"):
        return list_case(33, 433, limits=LIMITS[name])
    if name == "three-templates":
        return three_template_case()
    if name == "five-resources":
        return five_resource_case()
    if name.startswith("nodes-"):
        n = int(name[6:])
        return node_case(n, 500 + n, n_pods=24 if n < 257 else 13)
    raise KeyError(name)


TEMPLATE_PROBLEMS = ["list-%d" % n for n in LIST_SIZES] + ["three-templates", "five-resources"] + sorted(LIMITS)
NODE_PROBLEMS = ["nodes-%d" % n for n in NODE_SIZES]
ALL_PROBLEMS = TEMPLATE_PROBLEMS + NODE_PROBLEMS


# --- the oracle protocol ---------------------------------------------------------------------------------

def error_class(msg, codes):
    """The FC_* class of one NodePool's part of the reference's error text."""
    if "exceed limits" in msg:
        return codes["FC_LIMITS"]
    if "did not tolerate" in msg:
        return codes["FC_TAINTS"]
    if "no instance type" in msg:
        return codes["FC_NO_IT"]
    assert "incompatible requirements" in msg, msg
    return codes["FC_COMPAT"]


def oracle_template(bridge, snap, p, t):
    """(scheduled, sorted instanceTypeOptions or None, error text or None) of pod p against template t alone."""
    tpl = snap["nodeClaimTemplates"][t]
    name = tpl["metadata"]["name"]
    one = dict(snap, pods=[snap["pods"][p]], nodeClaimTemplates=[tpl], stateNodes=[], clusterPods=[],
               nodePools=[x for x in snap["nodePools"] if x["metadata"]["name"] == name],
               instanceTypesByNodePool={name: snap["instanceTypesByNodePool"].get(name, [])})
    res, _ = bridge.solve(json.dumps(one))
    assert not res["existingNodes"]
    if res["newNodeClaims"]:
        assert len(res["newNodeClaims"]) == 1 and res["newNodeClaims"][0]["pods"] == [0] and not res["podErrors"]
        return True, sorted(res["newNodeClaims"][0]["instanceTypeOptions"]), None
    return False, None, res["podErrors"]["0"]


def oracle_node(bridge, snap, p, node):
    """Whether the oracle places pod p on `node` alone (no NodePools)."""
    one = dict(snap, pods=[snap["pods"][p]], nodeClaimTemplates=[], nodePools=[], instanceTypesByNodePool={},
               instanceTypes=[], stateNodes=[node], clusterPods=[])
    res, _ = bridge.solve(json.dumps(one))
    assert not res["newNodeClaims"]
    placed = [e for e in res["existingNodes"] if e["pods"]]
    if placed:
        assert placed == [{"name": node["name"], "pods": [0]}] and not res["podErrors"], res
        return True
    return False  # (without a template the reference collects no error for the pod: the empty node entry says it all)


def check_against_oracle(bridge, snap, f):
    """Every (pod, template) and (pod, node) pair of `snap` against the matrix `f`; returns the pairs compared."""
    codes, meta, pairs = f.codes, f.meta, 0
    by_name = {n["name"]: n for n in snap["stateNodes"]}
    for p in range(len(snap["pods"])):
        states = list(f.states(p))
        for t in range(meta["NTPL"]):
            ok, opts, msg = oracle_template(bridge, snap, p, t)
            live = [s for s in states if f.tpl_count[s, t] > 0]
            assert ok == bool(live), (p, t, msg, [int(f.tpl_code[s, t]) for s in states])
            if ok:
                assert opts == sorted(f.options(p, live[0] - states[0], t)), (p, t)
            elif len(states) == 1:
                assert error_class(msg, codes) == int(f.tpl_code[states[0], t]) & 0xff, (p, t, msg, int(f.tpl_code[states[0], t]))
            pairs += 1
        for i, name in enumerate(meta["nodes"]):
            got = any((int(f.node_bits[s, i >> 5]) >> (i & 31)) & 1 for s in states)
            assert oracle_node(bridge, snap, p, by_name[name]) == got, (p, name)
            pairs += 1
    return pairs


def check_shape(f):
    """Invariants of the arrays alone: counts are popcounts, failing rows are all zero, no bit past a list or past N,
    meta indexes every array."""
    m = f.meta
    S, NTPL, N, TW, NWN = m["S"], m["NTPL"], m["N"], m["TW"], m["NWN"]
    assert f.tpl_code.shape == (S, NTPL) and f.tpl_count.shape == (S, NTPL) and f.tpl_options.shape == (S, NTPL, TW)
    assert f.node_bits.shape == (S, NWN) and f.node_count.shape == (S,) and NWN == (N + 31) // 32
    assert len(m["templates"]) == NTPL and len(m["nodes"]) == N and len(m["statePod"]) == S
    assert sum(m["podNState"]) == S
    for p, (s0, ns) in enumerate(zip(m["podState0"], m["podNState"])):
        assert m["statePod"][s0:s0 + ns] == [p] * ns
    pop = lambda a: int(sum(bin(int(w)).count("1") for w in a.ravel()))
    for s in range(S):
        for t in range(NTPL):
            n = len(m["templates"][t]["instanceTypes"])
            assert pop(f.tpl_options[s, t]) == f.tpl_count[s, t], (s, t)
            assert (f.tpl_count[s, t] > 0) == (f.tpl_code[s, t] == 0), (s, t)
            for q in range(n, 32 * TW):
                assert not (int(f.tpl_options[s, t, q >> 5]) >> (q & 31)) & 1, (s, t, q)
        assert pop(f.node_bits[s]) == f.node_count[s], s
        for i in range(N, 32 * NWN):
            assert not (int(f.node_bits[s, i >> 5]) >> (i & 31)) & 1, (s, i)


# --- the matrix as a bound on a Solve ----------------------------------------------------------------------

SOLVE_SEEDS = (3, 14, 27)


def solve_problem(seed):
    """problems.random_problem without topology, volumes and host ports: 100 pods, 9 nodes, three templates."""
    return problems.random_problem(seed, n_pods=100, n_nodes=9, n_templates=3)


def check_bounds_solve(f, existing_nodes, new_nodeclaims, pod_errors):
    """Every pod a Solve put on node n has bit n set in some state; every NewNodeClaim's options are a subset of the
    union over each of its pods' states of row (s, t); every pod unschedulable() names is in the pod errors.

    Asserted for the pods none of whose states is in meta["undefinedKeyStates"].  For the others the bound does not
    hold, and the reference shows it: Requirements.Compatible denies a custom label key the target does not define
    unless the operator is NotIn / DoesNotExist (requirements.go:163-174), and a NodeClaim or node gains the key when
    such a pod lands on it, so a later pod with In on that key joins a target its own row refuses
    (test_static_feasibility_host.py pins one such Solve).  Returns (placements checked, placements of the other
    pods that lie outside their rows)."""
    soft = set(f.meta["undefinedKeyStates"])
    node_ix = {n: i for i, n in enumerate(f.meta["nodes"])}
    tpl_ix = {t["nodePool"]: i for i, t in enumerate(f.meta["templates"])}
    checked = outside = 0
    for e in existing_nodes:
        i = node_ix[e["name"]]
        for p in e["pods"]:
            ok = any((int(f.node_bits[s, i >> 5]) >> (i & 31)) & 1 for s in f.states(p))
            if soft.intersection(f.states(p)):
                outside += not ok
                continue
            assert ok, (p, e["name"])
            checked += 1
    for c in new_nodeclaims:
        t = tpl_ix[c["nodePoolName"]]
        for p in c["pods"]:
            union = set()
            for j in range(f.meta["podNState"][p]):
                union |= set(f.options(p, j, t))
            ok = set(c["instanceTypeOptions"]) <= union
            if soft.intersection(f.states(p)):
                outside += not ok
                continue
            assert ok, (p, c["nodePoolName"])
            checked += 1
    never = f.unschedulable()
    assert set(never) <= {int(k) for k in pod_errors}, sorted(never)
    return checked, outside


# --- the C99 client (tests/c/feasibility_check.c) ------------------------------------------------------------

def c_client(mode, snap, tmp_path):
    import __graft_entry__

    __graft_entry__.build_abi_check()
    path = tmp_path / "snap.json"
    path.write_text(json.dumps(snap))
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "feasibility_check")
    out = subprocess.run([exe, mode, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout)


def c_client_agrees(doc, f):
    assert doc["meta"] == f.meta
    assert [[r[0] for r in st] for st in doc["tpl"]] == f.tpl_code.tolist()
    assert [[r[1] for r in st] for st in doc["tpl"]] == f.tpl_count.tolist()
    assert [[r[2] for r in st] for st in doc["tpl"]] == f.tpl_options.tolist()
    assert [r[0] for r in doc["node"]] == f.node_count.tolist() and [r[1] for r in doc["node"]] == f.node_bits.tolist()
    assert (doc["bytes_read"], doc["bytes_written"]) == (f.bytes_read, f.bytes_written)
