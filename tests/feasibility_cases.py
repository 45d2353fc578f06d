"""Cases and a plain reference for the two feasibility tables: k_feasibility's pod-state x
instance-type rows and k_feasibility_nodes's pod-state x existing-node rows.

The reference computes both tables from the snapshot JSON alone.  Requirements are Python sets and ints
(pkg/scheduling/requirement.go: a value set, a complement flag, Gt / Lt bounds), never bitsets; nothing here
reads the library's encoding.  tests/test_feasibility_reference.py checks it against the oracle's requirement
algebra on the CPU; tests/test_feasibility_rows_gpu.py compares the kernels' words with it bit for bit.

Node bit (state, node) = every taint of the node is tolerated by the state's tolerations (taints.go:38-50) AND the
strict Requirements.Compatible of the node's labels with the state (requirements.go:163-174, no
AllowUndefinedWellKnownLabels): every key of the state is a node label unless the state's operator on it is NotIn
or DoesNotExist, and on every shared key the node's value is one the state admits.

Instance-type bit (state, template, position) = the state tolerates the template's taints AND, for X = the state's
requirements and for X = the template's, every covered key X holds passes at that position.  A key passes when
the instance type lacks it, holds it as DoesNotExist, or holds a value X admits.  Covered keys come from the
snapshot: the keys some instance type constrains, plus zone and capacity-type, minus those some instance type
holds with more than one value.  A DoesNotExist position passes whatever X says: whether it intersects depends on
the operator of the whole NodeClaim record (requirements.go:248-252), which k_solve tests per step.  A position
whose instance type holds a complement requirement (NotIn / Exists / Gt / Lt) on the key is "irregular": the
host's position tables (ks_host.cpp, "feasibility tables") list it under none of the key's rows, so the table's
bit there is 0 whenever X holds the key, and k_solve decides such positions with the exact per-position check.
The reference pins that 0.

Scope: every pod's first relaxation state, and the later states of pods without preferred terms, pod (anti-)
affinity or spread constraints and with at most one required term -- those differ from the first only by the
PreferNoSchedule toleration Preferences.Relax adds (preferences.go:38-58).  States of other chains are left to
the end-to-end tests."""
import numpy as np

from karpenter_amd import synth

INT = "integer"
SLOT = "example.com/slot"
TEAMS = ["red", "blue", "green"]
ZONES = ["test-zone-1", "test-zone-2", "test-zone-3"]
ARCHS = ["amd64", "arm64"]
GOLD = {"key": "dedicated", "value": "gold", "effect": "NoSchedule"}
TOL_GOLD = {"key": "dedicated", "operator": "Equal", "value": "gold", "effect": "NoSchedule"}
TOL_ALL = {"operator": "Exists"}
TOL_PNS = {"operator": "Exists", "effect": "PreferNoSchedule"}
COMPLEMENT_OPS = ("NotIn", "Exists", "Gt", "Lt")


# --- requirement.go on sets and ints ---------------------------------------------------------------------

class Req:
    def __init__(self, complement, values=(), gt=None, lt=None):
        self.complement, self.values, self.gt, self.lt = complement, set(values), gt, lt

    def __repr__(self):
        return "Req(%s, %s, gt=%s, lt=%s)" % (self.complement, sorted(self.values), self.gt, self.lt)


def req_of(expr):
    """NewRequirement (requirement.go:45-86)."""
    op, vals = expr["operator"], expr.get("values") or []
    if op == "In":
        return Req(False, vals)
    if op == "NotIn":
        return Req(True, vals)
    if op == "Exists":
        return Req(True)
    if op == "DoesNotExist":
        return Req(False)
    if op == "Gt":
        return Req(True, gt=int(vals[0]))
    assert op == "Lt", op
    return Req(True, lt=int(vals[0]))


def within(value, gt, lt):
    if gt is None and lt is None:
        return True
    try:
        v = int(value)
    except ValueError:
        return False
    return not (gt is not None and gt >= v) and not (lt is not None and lt <= v)


def intersect(a, b):
    """Requirement.Intersection (requirement.go:150-185)."""
    gt = max([x for x in (a.gt, b.gt) if x is not None], default=None)
    lt = min([x for x in (a.lt, b.lt) if x is not None], default=None)
    if gt is not None and lt is not None and gt >= lt:
        return Req(False)
    if a.complement and b.complement:
        vals = a.values | b.values
    elif a.complement:
        vals = b.values - a.values
    elif b.complement:
        vals = a.values - b.values
    else:
        vals = a.values & b.values
    vals = {v for v in vals if within(v, gt, lt)}
    both = a.complement and b.complement
    return Req(both, vals, gt if both else None, lt if both else None)


def has(r, value):
    """Requirement.Has (requirement.go:214-220)."""
    return ((value not in r.values) if r.complement else (value in r.values)) and within(value, r.gt, r.lt)


def operator(r):
    if r.complement:
        return "NotIn" if r.values else "Exists"
    return "In" if r.values else "DoesNotExist"


def reqs_of(exprs):
    """Requirements.Add over a list of node selector requirements (requirements.go:120-130)."""
    out = {}
    for e in exprs:
        r = req_of(e)
        out[e["key"]] = intersect(out[e["key"]], r) if e["key"] in out else r
    return out


def tolerates_taint(tol, taint):
    """v1.Toleration.ToleratesTaint."""
    if tol.get("effect") and tol["effect"] != taint.get("effect", ""):
        return False
    if tol.get("key") and tol["key"] != taint["key"]:
        return False
    if tol.get("operator", "Equal") in ("", "Equal"):
        return tol.get("value", "") == taint.get("value", "")
    return tol["operator"] == "Exists"


def tolerates(taints, tols):
    return all(any(tolerates_taint(t, x) for t in tols) for x in taints)


# --- the states the reference covers ---------------------------------------------------------------------

def _node_affinity(pod):
    return pod["spec"].get("affinity", {}).get("nodeAffinity", {})


def pod_exprs(pod):
    """newPodRequirements of the unrelaxed pod (requirements.go:64-100): the node selector, the heaviest
    preferred term and the first required term, as one operand list."""
    out = [{"key": k, "operator": "In", "values": [v]} for k, v in sorted(pod["spec"].get("nodeSelector", {}).items())]
    na = _node_affinity(pod)
    pref = na.get("preferredDuringSchedulingIgnoredDuringExecution") or []
    if pref:
        top = max(p["weight"] for p in pref)
        heaviest = [p for p in pref if p["weight"] == top]
        assert len(heaviest) == 1, "tied preferred weights: sort.Slice decides, not modelled here"
        out += heaviest[0]["preference"].get("matchExpressions", [])
    terms = (na.get("requiredDuringSchedulingIgnoredDuringExecution") or {}).get("nodeSelectorTerms") or []
    if terms:
        out += terms[0].get("matchExpressions", [])
    return out


def simple_chain(pod):
    """The chain's states differ by the PreferNoSchedule toleration alone."""
    na = _node_affinity(pod)
    aff = pod["spec"].get("affinity", {})
    terms = (na.get("requiredDuringSchedulingIgnoredDuringExecution") or {}).get("nodeSelectorTerms") or []
    return (not na.get("preferredDuringSchedulingIgnoredDuringExecution") and len(terms) <= 1 and
            not aff.get("podAffinity") and not aff.get("podAntiAffinity") and
            not pod["spec"].get("topologySpreadConstraints"))


def relaxes_tolerations(snapshot):
    """Preferences.ToleratePreferNoSchedule: some NodePool carries a PreferNoSchedule taint (scheduler.go:66-73)."""
    return any(t.get("effect") == "PreferNoSchedule"
               for np_ in snapshot["nodePools"] for t in np_["spec"]["template"]["spec"].get("taints", []))


def covered_states(snapshot, pod):
    """[(operand list, tolerations)] of the states the reference covers, in chain order, and whether that is the
    pod's whole chain."""
    tols = list(pod["spec"].get("tolerations", []))
    states = [(pod_exprs(pod), tols)]
    if not simple_chain(pod):
        return states, False
    have = any(not t.get("key") and t.get("operator") == "Exists" and not t.get("value") and
               t.get("effect") == "PreferNoSchedule" for t in tols)
    if relaxes_tolerations(snapshot) and not have:
        states.append((states[0][0], tols + [TOL_PNS]))
    return states, True


# --- the node table --------------------------------------------------------------------------------------

def node_labels(node):
    lab = dict(node["labels"])
    lab[synth.HOSTNAME] = node.get("hostName", node["name"])
    return lab


def node_bit(node, X, tols):
    if not tolerates(node.get("taints", []), tols):
        return 0
    lab = node_labels(node)
    for key, r in X.items():
        if key not in lab:
            if operator(r) not in ("NotIn", "DoesNotExist"):
                return 0
        elif not has(r, lab[key]):
            return 0
    return 1


def node_rows(snapshot, node_names=None):
    """{(pod index, chain position): [bit per node]} for the covered states that hold a label requirement, nodes
    in `node_names` order (default: the snapshot's)."""
    by_name = {n["name"]: n for n in snapshot["stateNodes"]}
    assert len(by_name) == len(snapshot["stateNodes"])
    order = [by_name[n] for n in (node_names if node_names is not None else [n["name"] for n in snapshot["stateNodes"]])]
    out = {}
    for pi, pod in enumerate(snapshot["pods"]):
        for j, (exprs, tols) in enumerate(covered_states(snapshot, pod)[0]):
            X = reqs_of(exprs)
            if X:
                out[(pi, j)] = [node_bit(n, X, tols) for n in order]
    return out


# --- the instance-type table -----------------------------------------------------------------------------

def covered_keys(snapshot):
    keys, multi = {synth.ZONE, synth.CT}, set()
    for it in snapshot["instanceTypes"]:
        for e in it["requirements"]:
            keys.add(e["key"])
            if e["operator"] == "In" and len(set(e.get("values") or [])) > 1:
                multi.add(e["key"])
    return keys - multi


def template_exprs(tpl):
    """NewNodeClaimTemplate's requirements (nodeclaimtemplate.go:43-53): the NodePool's requirement list, its
    labels and the nodepool label."""
    t = tpl["spec"]["template"]
    labels = dict(t.get("metadata", {}).get("labels", {}))
    labels[synth.NODEPOOL] = tpl["metadata"]["name"]
    return list(t["spec"].get("requirements", [])) + \
        [{"key": k, "operator": "In", "values": [v]} for k, v in sorted(labels.items())]


def it_key_exprs(it, key):
    return [e for e in it["requirements"] if e["key"] == key]


def it_term(it, key, xr):
    """One key's term at one position (module docstring)."""
    mine = it_key_exprs(it, key)
    if not mine:
        return 1
    assert len(mine) == 1
    if mine[0]["operator"] in COMPLEMENT_OPS:
        return 0  # irregular position: in none of the key's position tables
    vals = mine[0].get("values") or []
    if mine[0]["operator"] == "DoesNotExist" or not vals:
        return 1
    assert len(vals) == 1
    return 1 if has(xr, vals[0]) else 0


def template_lists(snapshot):
    """Per template, its instance types in the snapshot's instanceTypesByNodePool order."""
    its = snapshot["instanceTypes"]
    return [[its[i]["name"] for i in snapshot["instanceTypesByNodePool"].get(t["metadata"]["name"], [])]
            for t in snapshot["nodeClaimTemplates"]]


def irregular_names(snapshot):
    return {it["name"] for it in snapshot["instanceTypes"]
            if any(e["operator"] in COMPLEMENT_OPS for e in it["requirements"])}


def it_rows(snapshot, lists=None):
    """{(pod index, chain position): [per template: None (taints not tolerated: a zero row) or [bit per position]]},
    positions in `lists` order (default: template_lists)."""
    lists = lists if lists is not None else template_lists(snapshot)
    by_name = {it["name"]: it for it in snapshot["instanceTypes"]}
    cov = covered_keys(snapshot)
    tpls = snapshot["nodeClaimTemplates"]
    tfac = []
    for t, names in zip(tpls, lists):  # the template's own factor, once per template
        T = {k: r for k, r in reqs_of(template_exprs(t)).items() if k in cov}
        tfac.append([all(it_term(by_name[n], k, r) for k, r in T.items()) for n in names])
    out, memo = {}, {}
    for pi, pod in enumerate(snapshot["pods"]):
        for j, (exprs, tols) in enumerate(covered_states(snapshot, pod)[0]):
            X = {k: r for k, r in reqs_of(exprs).items() if k in cov}
            sig = repr(sorted((k, repr(r)) for k, r in X.items()))
            row = []
            for ti, (t, names) in enumerate(zip(tpls, lists)):
                if not tolerates(t["spec"]["template"]["spec"].get("taints", []), tols):
                    row.append(None)
                    continue
                if (sig, ti) not in memo:
                    memo[(sig, ti)] = [1 if tf and all(it_term(by_name[n], k, r) for k, r in X.items()) else 0
                                       for tf, n in zip(tfac[ti], names)]
                row.append(memo[(sig, ti)])
            out[(pi, j)] = row
    return out


def pack(bits):
    """Bits as little-endian 32-bit words (bit i of the list is bit i & 31 of word i >> 5)."""
    words = [0] * ((len(bits) + 31) // 32)
    for i, b in enumerate(bits):
        if b:
            words[i >> 5] |= 1 << (i & 31)
    return words


# --- case builders ---------------------------------------------------------------------------------------

def _snapshot(its, by_pool, templates, nodes, pods):
    return {"wellKnownLabels": synth.FAKE_WELL_KNOWN + [SLOT], "instanceTypes": its, "instanceTypesByNodePool": by_pool,
            "nodeClaimTemplates": templates, "nodePools": templates, "stateNodes": nodes, "daemonSetPods": [],
            "pods": pods, "clusterPods": [], "volumeDrivers": {}}


def _affinity(exprs):
    return {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
        {"matchExpressions": exprs}]}}}


def make_its(n, V, irregular=True):
    """n fake instance types: unique names (the instance-type label has n values), `integer` = cpu cycling over V
    values, small types (cpu <= 4) hold `special` as DoesNotExist.  irregular: every 37th type (from the 6th)
    holds `size` as a complement, and -- where every integer value still occurs on another type -- every 41st
    (from the 8th) holds `integer` as one."""
    its = []
    for i in range(n):
        cpu = 1 + i % V
        it = synth.fake_instance_type("it-%04d" % i, cpu, 2 * cpu + (i // V) % 3, pods=110, arch=ARCHS[(i // 3) % 2])
        if irregular and i % 37 == 5:
            for e in it["requirements"]:
                if e["key"] == "size":
                    e.update(operator="NotIn", values=["tiny"])
        if irregular and n >= 2 * V and i % 41 == 7:
            for e in it["requirements"]:
                if e["key"] == INT:
                    e.update(operator="Gt", values=["0"])
        its.append(it)
    return its


def _int_values(its):
    return sorted({e["values"][0] for it in its for e in it["requirements"] if e["key"] == INT and e["operator"] == "In"},
                  key=int)


def it_pods(rng, n_pods, its, key):
    """Pods whose rows differ from their neighbours': kinds alternate between an In selector, NotIn with few and
    with nearly all values excluded, Exists / DoesNotExist, Gt, Lt, no requirement, and a pod that does not
    tolerate the tainted template (a zero row).  `key`: the key the In / NotIn terms name (the instance-type label
    or `integer`); Gt / Lt are always on `integer`.  No state names a key twice."""
    names = [it["name"] for it in its]
    ints = _int_values(its)
    vals = names if key == synth.IT_LABEL else ints
    pods = []
    for i in range(n_pods):
        kind = i % 8
        tols = [TOL_GOLD] if (i // 8) % 2 == 0 else [TOL_ALL]
        sel, exprs = {}, []
        pick = lambda k: [vals[int(x)] for x in sorted(rng.choice(len(vals), size=min(k, len(vals)), replace=False))]
        if kind == 0:
            # the last, the first or a random value: the In row's bits sit in the last and the first word too
            sel[key] = vals[-1] if i % 24 == 0 else vals[0] if i % 24 == 8 else pick(1)[0]
        elif kind == 1:
            exprs.append({"key": key, "operator": "NotIn", "values": pick(2)})
            if i % 16 == 1:
                sel[synth.ARCH] = ARCHS[(i // 16) % 2]
        elif kind == 2:
            exprs.append({"key": key, "operator": "NotIn", "values": pick(max(1, len(vals) - 1 - int(rng.integers(1, 4))))})
        elif kind == 3:
            exprs.append({"key": "special", "operator": ["Exists", "DoesNotExist", "NotIn"][(i // 8) % 3],
                          **({"values": ["optional"]} if (i // 8) % 3 == 2 else {})})
            exprs.append({"key": INT, "operator": "Exists"})
        elif kind == 4:
            exprs.append({"key": INT, "operator": "Gt", "values": [ints[int(rng.integers(len(ints)))]]})
            if i % 16 == 4:
                exprs.append({"key": "size", "operator": "In", "values": ["large"]})
        elif kind == 5:
            exprs.append({"key": INT, "operator": "Lt", "values": [ints[int(rng.integers(len(ints)))]]})
            if i % 16 == 5:
                exprs.append({"key": "size", "operator": "Exists"})
        elif kind == 7:
            tols = []
            sel[key] = pick(1)[0]
        p = synth.pod(i, cpu="100m", mem="64Mi", node_selector=sel or None, affinity=_affinity(exprs) if exprs else None,
                      tolerations=tols or None)
        pods.append(p)
    return pods


def it_case(n_its, V, n_pods, seed, key=INT):
    """One tainted template over n_its instance types; the NodePool holds a NotIn term on `integer` (three values
    spread over its universe, not the first or the last) and an Exists on `special`, so the template factor takes the complement branches
    the pods' factor takes."""
    rng = np.random.default_rng(seed)
    its = make_its(n_its, V)
    ints = _int_values(its)
    # (a single type: exclude a value no type holds, or the template factor would be all zero)
    excl = sorted({ints[2], ints[len(ints) // 2], ints[-4]}, key=int) if len(ints) > 8 else ["99"]
    reqs = [{"key": INT, "operator": "NotIn", "values": excl}]
    if n_its > 1:
        reqs.append({"key": "special", "operator": "Exists"})
    pool = synth.node_pool("pool-0", requirements=reqs, taints=[GOLD])
    return _snapshot(its, {"pool-0": list(range(n_its))}, [pool], [], it_pods(rng, n_pods, its, key))


def three_template_case(seed, n_pods=21):
    """Three templates over lists of 40, 33 and 7 instance types (TW = 2: the shorter lists leave zero tails), one
    tainted NoSchedule, one PreferNoSchedule (every pod but one then has two states: S = 2 * n_pods - 1, so
    S * NTPL is odd and the last wave step of k_feasibility<32> has a dead half), one untainted."""
    rng = np.random.default_rng(seed)
    its = make_its(40, 40)
    ints = _int_values(its)
    pools = [synth.node_pool("pool-a", weight=30, requirements=[{"key": INT, "operator": "Gt", "values": [ints[4]]}],
                             taints=[GOLD]),
             synth.node_pool("pool-b", weight=20, requirements=[{"key": INT, "operator": "NotIn", "values": ints[30:36]}],
                             taints=[{"key": "spotty", "value": "", "effect": "PreferNoSchedule"}]),
             synth.node_pool("pool-c", weight=10, requirements=[{"key": synth.IT_LABEL, "operator": "NotIn",
                                                                 "values": [its[11]["name"], its[14]["name"]]}])]
    by_pool = {"pool-a": list(range(40)), "pool-b": list(range(7, 40)), "pool-c": list(range(10, 17))}
    pods = it_pods(rng, n_pods, its, INT)
    pods[6]["spec"]["tolerations"] = [TOL_GOLD, TOL_PNS]  # the one single-state pod
    return _snapshot(its, by_pool, pools, [], pods)


def make_nodes(rng, n, cpu=("4",), pool="pool-0"):
    """n existing nodes: a unique `slot` label each, zone / team / integer labels that some nodes lack, a third
    tainted dedicated=gold."""
    nodes = []
    for i in range(n):
        name = "node-%04d" % i
        labels = {synth.ARCH: ARCHS[int(rng.integers(2))], synth.CT: "on-demand", synth.NODEPOOL: pool,
                  synth.HOSTNAME: name, SLOT: "s%d" % i}
        if rng.random() < 0.85:
            labels[synth.ZONE] = ZONES[int(rng.integers(3))]
        if rng.random() < 0.75:
            labels["team"] = TEAMS[int(rng.integers(3))]
        if rng.random() < 0.8:
            labels[INT] = str(int(rng.integers(1, 41)))
        c = cpu[i % len(cpu)]
        nodes.append({"name": name, "hostName": name, "labels": labels,
                      "taints": [GOLD] if rng.random() < 1 / 3 else [],
                      "available": {"cpu": c, "memory": "%sGi" % (4 * int(c)), "pods": "20"},
                      "capacity": {"cpu": c, "memory": "%sGi" % (4 * int(c)), "pods": "110"},
                      "daemonSetRequests": {}, "initialized": True})
    return nodes


def node_pod(rng, i, n_nodes, cpu="100m"):
    """Pod i of the node cases: the kinds of it_pods on the nodes' labels, with and without the toleration."""
    kind = i % 8
    tols = [TOL_GOLD] if (i // 8) % 2 == 0 else []
    sel, exprs = {}, []
    slots = lambda k: ["s%d" % int(x) for x in sorted(rng.choice(n_nodes, size=max(1, min(k, n_nodes)), replace=False))]
    if kind == 0:
        sel[synth.ZONE] = ZONES[int(rng.integers(3))]
    elif kind == 1:
        exprs.append({"key": "team", "operator": "NotIn", "values": [TEAMS[int(rng.integers(3))]]})
    elif kind == 2:
        exprs.append({"key": "team", "operator": ["Exists", "DoesNotExist"][(i // 8) % 2]})
        tols = [TOL_GOLD] if (i // 16) % 2 == 0 else []
    elif kind == 3:
        exprs.append({"key": INT, "operator": ["Gt", "Lt"][(i // 8) % 2], "values": [str(int(rng.integers(5, 36)))]})
        tols = [TOL_GOLD] if (i // 16) % 2 == 0 else []
    elif kind == 5:
        sel[synth.ARCH] = ARCHS[(i // 8) % 2]
        tols = []
    elif kind == 6:
        exprs.append({"key": SLOT, "operator": "NotIn", "values": slots(n_nodes // 2)})
        tols = [TOL_ALL]
    elif kind == 7:
        exprs.append({"key": SLOT, "operator": "In", "values": slots(max(3, n_nodes // 4))})
        exprs.append({"key": synth.ZONE, "operator": "NotIn", "values": [ZONES[int(rng.integers(3))]]})
        tols = [TOL_GOLD]
    return synth.pod(i, cpu=cpu, mem="64Mi", node_selector=sel or None, affinity=_affinity(exprs) if exprs else None,
                     tolerations=tols or None)


def node_case(n_nodes, seed, n_pods=64):
    rng = np.random.default_rng(seed)
    its = make_its(4, 4, irregular=False)
    pool = synth.node_pool("pool-0")
    nodes = make_nodes(rng, n_nodes)
    return _snapshot(its, {"pool-0": [0, 1, 2, 3]}, [pool], nodes, [node_pod(rng, i, n_nodes) for i in range(n_pods)])


# --- end-to-end cases at the same edges ------------------------------------------------------------------

def node_solve_case(n_nodes, seed):
    """Existing nodes with room for one or two pods each and, per selector set, one pod more than the nodes it
    admits have room for: first fit walks every word of the pods' rows, the later pods of a set past nodes an
    earlier commit filled."""
    rng = np.random.default_rng(seed)
    its = make_its(8, 8, irregular=False)
    pool = synth.node_pool("pool-0", taints=[GOLD])
    nodes = make_nodes(rng, n_nodes, cpu=("1", "2"))
    protos = [node_pod(rng, i, n_nodes, cpu="900m") for i in (0, 1, 2, 3, 5, 6, 7, 10, 11, 15)]
    pods = []
    for proto in protos:
        exprs, tols = pod_exprs(proto), proto["spec"].get("tolerations", [])
        X = reqs_of(exprs)
        room = sum(int(n["available"]["cpu"]) for n in nodes if node_bit(n, X, tols))
        for _ in range(room + 1):
            p = synth.pod(len(pods), cpu="900m", mem="64Mi")
            p["spec"].update({k: v for k, v in proto["spec"].items() if k in ("nodeSelector", "affinity", "tolerations")})
            pods.append(p)
    return _snapshot(its, {"pool-0": list(range(8))}, [pool], nodes, pods)


def it_solve_case(n_its, seed, n_pods=64):
    """The pods of it_case with requests that differ, so the Solve opens several NodeClaims whose instance-type
    options come from rows of TW words."""
    snap = it_case(n_its, 50, n_pods, seed, key=synth.IT_LABEL)
    rng = np.random.default_rng(seed + 1)
    for p in snap["pods"]:
        p["spec"]["containers"][0]["resources"]["requests"] = {
            "cpu": ["500m", "1", "2500m", "7"][int(rng.integers(4))], "memory": ["256Mi", "1Gi", "5Gi"][int(rng.integers(3))]}
    return snap


# --- the case lists (seeds chosen by tests/test_feasibility_reference.py's non-degeneracy checks) -----------------

NODE_SIZES = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300)
NODE_SEEDS = {n: 100 + n for n in NODE_SIZES}

# instance-type rows, shape: list length -> (pods, seed); the In / NotIn terms name the instance-type label, whose
# universe is the list (one value per type), so the pods' complement loops run ceil(n / GW) chunks
SHAPE_SIZES = (1, 31, 32, 33, 1024, 1025, 2048, 2049)
SHAPE_CASES = {n: (64 if n < 1024 else 16, 200 + n) for n in SHAPE_SIZES}

# instance-type rows, value chunks: (values of `integer`, instantiation) -> (instance types, pods, seed); GW = 32
# runs on a list of V types (TW <= 4), GW = 64 on 1056 types (TW = 33) whose `integer` cycles over the V values
VALUE_SIZES = (31, 32, 33, 63, 64, 65, 100)
VALUE_CASES = {(v, gw): (v if gw == 32 else 1056, 64 if gw == 32 else 32, 300 + v + gw) for v in VALUE_SIZES for gw in (32, 64)}
THREE_TEMPLATE_SEED = 7


def node_snapshot(n):
    return node_case(n, NODE_SEEDS[n])


def shape_snapshot(n):
    pods, seed = SHAPE_CASES[n]
    return it_case(n, min(n, 50), pods, seed, key=synth.IT_LABEL)


def value_snapshot(v, gw):
    n, pods, seed = VALUE_CASES[(v, gw)]
    return it_case(n, v, pods, seed, key=INT)


def three_template_snapshot():
    return three_template_case(THREE_TEMPLATE_SEED)
