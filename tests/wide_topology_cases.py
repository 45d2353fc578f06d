"""Constructed inputs that take the topology kernels (topo_pop, topo_node_state1/K, topo_apply, topo_record, tcnt_at /
tcnt_inc, tdom; ks_solve.hip as ks_solve_topo.hip and ks_sim_topo.hip instantiate it) to the shape edges no random
generator of the suite reaches: more than 64 non-hostname domains (a second stride of a wave's domain scan), domains past
a 32-bit requirement word, a custom topology key, a fifth topology key slot and nodes past index 256 in a simulation,
count words outside the LDS-resident small prefix, and the Solve plans that keep the whole count table, only the small
prefix, or no node-domain table in LDS.

Nothing is drawn at random.  Each case states the cell it targets and what must be true of the answer; the CPU test
(test_wide_topology_preconditions.py) proves both with the inspectors and the oracle, the GPU test
(test_wide_topology_gpu.py) compares the kernels with the oracle bit for bit.

Domains are named <prefix>-000 ... <prefix>-NNN, so that a domain's position in the sorted-name order (its value id, the
bit `pos & 31` of requirement word `pos >> 5`, lane `pos & 63` of stride `pos >> 6`) is the number in its name."""
import copy
import functools
import json
import re

from karpenter_amd import synth

ZONE, HOST = synth.ZONE, synth.HOSTNAME
RACK = "example.com/rack"  # custom (not well-known): the final Compatible does not allow it undefined
MORE_KEYS = ["example.com/row", "example.com/room", "example.com/cage", "example.com/pdu"]
FULL_BUDGET = 160 * 1024 - 256
GI = synth.GI

NVS = (33, 64, 65, 129)
TYPES = ("spread", "affinity", "anti")
TG_SPREAD, TG_AFFINITY, TG_ANTI = 0, 1, 2


def names(key, nv):
    prefix = "zone" if key == ZONE else key.split("/")[-1]
    return ["%s-%03d" % (prefix, i) for i in range(nv)]


def positions(nv):
    """The deciding domain's positions: first, both sides of the word boundary, both sides of the lane boundary, last."""
    return sorted({p for p in (0, 31, 32, 63, 64, nv - 1) if p < nv})


def instance_types(zones, n=6):
    its = []
    for i in range(n):
        cpu, mem = 2 << i, 4 << i
        price = synth.price_from_resources(cpu, mem * GI)
        offers = [{"capacityType": "on-demand", "zone": z, "price": price, "available": True} for z in zones]
        its.append(synth.fake_instance_type("wide-it-%d" % i, cpu, mem, pods=110, offerings=offers))
    return its


def state_node(name, labels, cpu=16):
    lab = {synth.NODEPOOL: "default", synth.IT_LABEL: "wide-it-3", synth.ARCH: "amd64", synth.OS: "linux",
           synth.CT: "on-demand", HOST: name, "testing/cluster": "unspecified"}
    lab.update(labels)
    return {"name": name, "hostName": name, "labels": lab, "taints": [],
            "available": {"cpu": "%d" % (cpu - 1), "memory": "%dGi" % (2 * cpu - 2), "pods": "100"},
            "capacity": {"cpu": str(cpu), "memory": "%dGi" % (2 * cpu), "pods": "110"},
            "daemonSetRequests": {}, "initialized": True}


class Builder:
    """One pool over 6 instance types offered in every zone; cluster pods bound to label-only nodes (clusterNodes) seed
    the counts, so a 129-domain case needs no 129 existing nodes."""

    def __init__(self, nz=3, pool_keys=None):
        self.zones = names(ZONE, nz)
        self.pool_keys = dict(pool_keys or {})  # custom key -> its values, a pool `In` requirement
        self.pods, self.nodes, self.cluster, self.cnodes = [], [], [], {}
        self.pid = 0

    def domains(self, key):
        return self.zones if key == ZONE else self.pool_keys[key]

    def labels_at(self, key, dom):
        """Node labels that put a node in domain `dom` of `key` (and in the first domain of every other key)."""
        lab = {ZONE: self.zones[0]}
        for k, vals in self.pool_keys.items():
            lab[k] = vals[0]
        lab[key] = dom
        return lab

    def seed(self, key, dom, app, n=1, anti=None):
        """n bound cluster pods of `app` in domain `dom` (anti: with required anti-affinity to that app on `key`)."""
        name = "seed-%s" % dom
        self.cnodes.setdefault(name, {HOST: name, **self.labels_at(key, dom)})
        for _ in range(n):
            p = synth.pod(900000 + len(self.cluster), cpu="100m", mem="64Mi", labels={"app": app})
            p["spec"]["nodeName"] = name
            p["status"] = {"phase": "Running"}
            if anti:
                p["spec"]["affinity"] = {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
                    {"labelSelector": {"matchLabels": {"app": anti}}, "topologyKey": key}]}}
            self.cluster.append(p)

    def pod(self, cpu, app, extra=None, affinity=None, selector=None, not_in=None):
        p = synth.pod(self.pid, cpu=cpu, mem="128Mi", labels={"app": app}, node_selector=selector, affinity=affinity,
                      extra=extra)
        if not_in:
            key, vals = not_in
            p["spec"].setdefault("affinity", {})["nodeAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": {
                "nodeSelectorTerms": [{"matchExpressions": [{"key": key, "operator": "NotIn", "values": list(vals)}]}]}}
        self.pods.append(p)
        self.pid += 1
        return self.pid - 1

    def node(self, name, labels):
        self.nodes.append(state_node(name, labels))

    def snapshot(self):
        reqs = [{"key": k, "operator": "In", "values": list(v)} for k, v in self.pool_keys.items()]
        pool = synth.node_pool("default", requirements=reqs)
        its = instance_types(self.zones)
        return {"wellKnownLabels": synth.FAKE_WELL_KNOWN, "instanceTypes": its,
                "instanceTypesByNodePool": {"default": list(range(len(its)))}, "nodeClaimTemplates": [pool],
                "nodePools": [pool], "stateNodes": self.nodes, "daemonSetPods": [], "pods": self.pods,
                "clusterPods": self.cluster,
                "clusterNodes": [{"name": n, "labels": lab} for n, lab in sorted(self.cnodes.items())]}


def spread(key, app, skew=1, min_domains=None):
    c = {"topologyKey": key, "maxSkew": skew, "whenUnsatisfiable": "DoNotSchedule",
         "labelSelector": {"matchLabels": {"app": app}}}
    if min_domains is not None:
        c["minDomains"] = min_domains
    return {"topologySpreadConstraints": [c]}


def pod_affinity(key, app, anti=False):
    return {"podAntiAffinity" if anti else "podAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
        {"labelSelector": {"matchLabels": {"app": app}}, "topologyKey": key}]}}


def _builder(key, nv):
    return Builder(nz=nv) if key == ZONE else Builder(pool_keys={key: names(key, nv)})


def _constrained(b, key, gtype, pos, error=False, not_in=None, cpu="1"):
    """Seed the counts so that domain `pos` alone decides for a pod of group type `gtype`, and add that pod.
    error: no domain is left (the deciding domain holds 2 where the others hold 1, so the message names it).
    not_in: a domain the pod's strict requirements exclude.  Returns the pod's index."""
    dom = b.domains(key)
    nv = len(dom)
    if gtype in ("spread", "spread-tie", "spread-notin"):
        # every other domain at min + maxSkew: only the domain at the minimum passes the skew test
        hold = {pos}
        if gtype == "spread-tie":  # the last domain ties with it: the smaller name wins, (count << 32) | v
            hold.add(nv - 1)
        if gtype == "spread-notin":  # the domain before it is at the minimum too, but the pod excludes it
            hold.add(pos - 1)
            not_in = (key, [dom[pos - 1]])
        for v in range(nv):
            if error:
                b.seed(key, dom[v], "s", 2 if v == pos else 1)
            elif v not in hold:
                b.seed(key, dom[v], "s")
        # error: minDomains above the domain count makes the minimum 0, and every domain holds maxSkew already
        return b.pod(cpu, "s", extra=spread(key, "s", min_domains=nv + 1 if error else None), not_in=not_in)
    if gtype == "affinity":  # the only domain with a selected pod
        if error:  # the only domain with selected pods is one the pod's strict requirements exclude
            b.seed(key, dom[pos], "a-target", 2)
            return b.pod(cpu, "a-client", affinity=pod_affinity(key, "a-target"), not_in=(key, [dom[pos]]))
        b.seed(key, dom[pos], "a-target")
        return b.pod(cpu, "a-client", affinity=pod_affinity(key, "a-target"), not_in=not_in)
    if gtype == "affinity-bootstrap":  # a self-selecting pod and no selected pod: the first domain it allows
        assert pos < nv - 1 and not error
        p = b.pod(cpu, "b", affinity=pod_affinity(key, "b"))
        b.pods[p]["spec"]["affinity"]["nodeAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": {
            "nodeSelectorTerms": [{"matchExpressions": [{"key": key, "operator": "In",
                                                         "values": [dom[pos], dom[nv - 1]]}]}]}}
        return p
    if gtype == "anti":  # the only registered zero-count domain
        for v in range(nv):
            if error:
                b.seed(key, dom[v], "x-target", 2 if v == pos else 1)
            elif v != pos:
                b.seed(key, dom[v], "x-target")
        return b.pod(cpu, "x-client", affinity=pod_affinity(key, "x-target", anti=True), not_in=not_in)
    assert gtype == "inverse", gtype  # bound pods that refuse the pending pod's app everywhere else
    for v in range(nv):
        if error:
            b.seed(key, dom[v], "i-owner", 2 if v == pos else 1, anti="i-victim")
        elif v != pos:
            b.seed(key, dom[v], "i-owner", anti="i-victim")
    return b.pod(cpu, "i-victim", not_in=not_in)


TARGETS = ("claim", "open", "node", "unlabelled", "error")


def solve_case(key, nv, gtype, pos, target="claim"):
    """One pod of group type `gtype` over `nv` domains of `key` whose only admissible domain is the one at `pos`, placed
    on a fresh NodeClaim, an open NodeClaim (a larger unconstrained pod opened it; this pod narrows it), an existing
    node in that domain (among nodes in the other edge domains), an existing node lacking the key's label (node_slow;
    probe pods with a node selector per edge domain then show which domain the node took), or nowhere."""
    b = _builder(key, nv)
    dom = b.domains(key)
    probes = {}
    if target == "open":
        b.pod("2", "generic")
    if target == "node":
        for v in sorted(set(positions(nv)) | {1, pos}):
            b.node("node-at-%s" % dom[v], b.labels_at(key, dom[v]))
    not_in = None
    if target == "unlabelled":
        lab = b.labels_at(key, dom[0])
        del lab[key]
        b.node("node-unlabelled", lab)
        # a NotIn on the key admits the node (existingnode.go:97-115); the excluded domain is not the deciding one
        not_in = (key, [dom[(pos + 2) % nv]])
    p = _constrained(b, key, gtype, pos, error=target == "error", not_in=not_in, cpu="1")
    if target == "unlabelled":
        for v in sorted(set(positions(nv)) | {1, pos}):
            probes[b.pod("500m", "probe", selector={key: dom[v]})] = dom[v]
    return {"kind": "solve", "snapshot": b.snapshot(), "key": key, "nv": nv, "type": gtype, "pos": pos, "target": target,
            "pod": p, "domain": dom[pos], "probes": probes, "budget": 0}


def _base_type(gtype):
    return {"spread": TG_SPREAD, "spread-tie": TG_SPREAD, "spread-notin": TG_SPREAD, "affinity": TG_AFFINITY,
            "affinity-bootstrap": TG_AFFINITY, "anti": TG_ANTI, "inverse": TG_ANTI}[gtype]


def min_domains_case(m, nv=65):
    """Spread with minDomains m over nv = 65 eligible domains, each holding maxSkew = 1 pod already: with m <= 65 the
    minimum is 1 and the pod lands in the first domain; with m = 66 the minimum drops to 0 (topologygroup.go:204-207)
    and no domain passes.  The eligible-domain count is a sum over two strides of the wave."""
    b = _builder(ZONE, nv)
    for z in b.zones:
        b.seed(ZONE, z, "s")
    p = b.pod("1", "s", extra=spread(ZONE, "s", min_domains=m))
    return {"kind": "solve", "snapshot": b.snapshot(), "key": ZONE, "nv": nv, "type": "spread", "pos": 0,
            "target": "claim" if m <= nv else "error", "pod": p, "domain": b.zones[0] if m <= nv else [], "probes": {},
            "budget": 0, "minDomains": m}


def closed_form_case(kind, nv):
    """No nodes, no seeds, 2 * nv identical pods (the answer is known without the oracle):
    even      maxSkew 1 over nv zones: every zone ends with exactly 2 pods;
    mindom    the same with minDomains nv + 1: the minimum stays 0, so each zone holds at most maxSkew = 1 pod;
    anti      zonal anti-affinity to their own app, pod i pinned to zone i % nv by a node selector: one pod per zone,
              the other nv fail.  (Unpinned, the first pod's NodeClaim keeps every zero-count zone and Topology.Record
              blocks them all, topology.go:130-133, so one pod is placed and 2 nv - 1 fail: the oracle does just that.)"""
    b = _builder(ZONE, nv)
    for i in range(2 * nv):
        if kind == "anti":
            b.pod("1", "c", affinity=pod_affinity(ZONE, "c", anti=True), selector={ZONE: b.zones[i % nv]})
        else:
            b.pod("1", "c", extra=spread(ZONE, "c", min_domains=nv + 1 if kind == "mindom" else None))
    return {"kind": "solve", "snapshot": b.snapshot(), "key": ZONE, "nv": nv, "type": kind, "budget": 0}


# ---- the Solve plan cells: one wide problem, three budgets -------------------------------------------------------
PLAN_APPS = 18
PLAN_NV = 129


PLAN_FULL_NODES = 88


def plan_problem():
    """18 zonal spread apps over 129 zones (2322 count words: the 16th group on leaves the 2048-word small prefix),
    a rack spread app (70 racks), a hostname spread app, 8 existing nodes with room and 88 without.  App a's only
    admissible zone is zone 7 a + 3 (every other zone holds a pod of the app), so every zone group, small or not,
    decides a placement; apps 0-7 find an existing node in their zone, the others open NodeClaims.

    The 88 full nodes are what the `tdl == 0` cell costs: make_plan keeps the node-domain table (TK x N words) in
    LDS while 16 bytes per word fit in what the count table leaves, and the smallest inspected budget that still
    holds this problem's small prefix and its 22 claims (14000) leaves about 3.4 KiB, so TK x N must exceed ~215
    words: 3 keys x 96 nodes."""
    b = Builder(nz=PLAN_NV, pool_keys={RACK: names(RACK, 70)})
    want = {}
    for a in range(PLAN_APPS):
        app, at = "plan-%02d" % a, 7 * a + 3
        for v in range(PLAN_NV):
            if v != at:
                b.seed(ZONE, b.zones[v], app)
        want[b.pod("1", app, extra=spread(ZONE, app))] = b.zones[at]
    for a in range(8):
        b.node("node-%02d" % a, b.labels_at(ZONE, b.zones[7 * a + 3]))
    for j in range(PLAN_FULL_NODES):
        b.node("node-full-%02d" % j, b.labels_at(ZONE, b.zones[(5 * j) % PLAN_NV]))
        b.nodes[-1]["available"] = {"cpu": "0", "memory": "0", "pods": "0"}
    racks = b.pool_keys[RACK]
    for v in range(70):
        if v != 66:
            b.seed(RACK, racks[v], "plan-rack")
    rack_pod = b.pod("3", "plan-rack", extra=spread(RACK, "plan-rack"))
    for _ in range(3):
        b.pod("500m", "plan-host", extra=spread(HOST, "plan-host"))
    return b.snapshot(), want, (rack_pod, racks[66])


PLAN_CELLS = ("whole-table", "small-prefix", "no-node-domains")


def plan_case(cell):
    snap, want, rack = plan_problem()
    return {"kind": "solve-plan", "snapshot": snap, "cell": cell, "zones": want, "rack": rack}


def plan_budget(dims, cell):
    """The first of the inspected budgets (largest first) whose level-0 plan is in the cell."""
    for budget, pl in sorted(((int(k), v) for k, v in dims["plans"].items()), reverse=True):
        ok = {"whole-table": pl["tcl"] == dims["tgCntWords"] and pl["tdl"] > 0,
              "small-prefix": pl["tcl"] == dims["tgSmall"] < dims["tgCntWords"] and pl["tdl"] > 0,
              "no-node-domains": pl["tdl"] == 0 and pl["KO"] >= dims["pods"]}[cell]
        if ok:
            return budget, pl
    return None, None


# ---- simulations -------------------------------------------------------------------------------------------------
def wide_cluster(n_nodes, ppn, nz, apps, seed, keys=(), n_its=60, it_range=(8, 30), candidates=None, n_pending=2):
    """synth.cluster_snapshot widened: `nz` zones (offerings, pool requirement, node labels round-robin), the custom
    keys `keys` on the pool and the nodes, and the app specs `apps` (a list of functions app name -> pod spec update)
    dealt to the bound and pending pods in turn.  candidates: node indices listed as candidates (default: all)."""
    snap = synth.cluster_snapshot(n_nodes, ppn, n_its=n_its, it_range=it_range, seed=seed, n_pending=n_pending,
                                  spot_frac=0.0)
    zones = names(ZONE, nz)
    for i, it in enumerate(snap["instanceTypes"]):
        price = it["offerings"][0]["price"]
        offers = [{"capacityType": "on-demand", "zone": z, "price": price, "available": True} for z in zones]
        snap["instanceTypes"][i] = synth.fake_instance_type(it["name"], i + 1, 2 * (i + 1), pods=10 * (i + 1),
                                                            offerings=offers)
    key_vals = {k: names(k, nv) for k, nv in keys}
    pool = snap["nodePools"][0]
    pool["spec"]["template"]["spec"]["requirements"] = (
        [{"key": ZONE, "operator": "In", "values": zones}] +
        [{"key": k, "operator": "In", "values": v} for k, v in key_vals.items()])
    snap["nodeClaimTemplates"] = [pool]
    cluster = []
    k = 0
    # NewTopology creates the groups in pod order, pending pods first (then the nodes' pods, node by node): dealing
    # the apps in that order makes app a's first group the a-th owned group of the encoding
    for p in snap["pendingPods"]:
        app = "wide-%02d" % (k % len(apps))
        p["metadata"]["labels"]["app"] = app
        p["spec"].update(apps[k % len(apps)](app))
        k += 1
    for j, n in enumerate(snap["stateNodes"]):
        # zones and custom domains walk at different paces, from the far end, so every edge domain is populated
        n["labels"][ZONE] = zones[(nz - 1 - 7 * j) % nz]
        n["labels"][synth.CT] = "on-demand"
        for q, (key, vals) in enumerate(key_vals.items()):
            n["labels"][key] = vals[(len(vals) - 1 - (3 + 2 * q) * j) % len(vals)]
        for p in n["pods"]:
            app = "wide-%02d" % (k % len(apps))
            p["metadata"]["labels"]["app"] = app
            p["spec"].update(apps[k % len(apps)](app))
            cluster.append(p)
            k += 1
    snap["clusterPods"] = cluster
    if candidates is not None:
        snap["candidates"] = [snap["stateNodes"][j]["name"] for j in candidates]
    return snap


def _apps(zone_keys, n_spread=2):
    """Spread (DoNotSchedule), affinity and anti-affinity apps per key, to their own app."""
    out = []
    for key in zone_keys:
        for s in range(n_spread):
            out.append(functools.partial(lambda app, key, s: spread(key, app, skew=1 + s), key=key, s=s))
        out.append(functools.partial(lambda app, key: {"affinity": pod_affinity(key, app)}, key=key))
        out.append(functools.partial(lambda app, key: {"affinity": pod_affinity(key, app, anti=True)}, key=key))
    return out


ROOM = {"cpu": "8", "memory": "16Gi", "pods": "50"}


def _anchor_and_mover(snap, r, m, key, alone=False):
    """An anchor pod on node r and, on node m, a pod that requires pod affinity to the anchor's app on `key`
    (alone: in place of node m's other pods).  With r alone in its domain of `key`, r is the one existing node the pod
    fits: node m's simulation ends without a NodeClaim exactly when r has room and its domain is read right."""
    nodes = snap["stateNodes"]
    pid = 700000 + 2 * r
    anchor = synth.pod(pid, cpu="100m", mem="64Mi", labels={"app": "anchor-%d" % r})
    mover = synth.pod(pid + 1, cpu="200m", mem="64Mi", labels={"app": "mover-%d" % r},
                      affinity=pod_affinity(key, "anchor-%d" % r))
    for p, at in ((anchor, r), (mover, m)):
        p["spec"]["nodeName"] = nodes[at]["name"]
        p["status"] = {"phase": "Running", "conditions": [{"type": "PodScheduled", "status": "True"}]}
        p["metadata"]["annotations"] = {"controller.kubernetes.io/pod-deletion-cost": str(10 * at)}
    if alone:
        gone = {q["metadata"]["uid"] for q in nodes[m]["pods"]}
        snap["clusterPods"] = [q for q in snap["clusterPods"] if q["metadata"]["uid"] not in gone]
        nodes[m]["pods"] = []
    snap["clusterPods"] = snap["clusterPods"] + [anchor, mover]
    nodes[m]["pods"] = nodes[m]["pods"] + [mover]
    nodes[r]["pods"] = nodes[r]["pods"] + [anchor]


def sim_wide_zones():
    """(a) 70 zones: spread / affinity / anti-affinity apps over a 10-node cluster."""
    return {"kind": "cons", "snapshot": wide_cluster(10, 4, 70, _apps([ZONE]), seed=501), "cell": "wide-zones"}


# (receiver, mover, key): the keys of slots 4 and 5; the movers sit on late nodes, after every app created its groups
SLOT_PAIRS = ((8, 6, MORE_KEYS[2]), (9, 7, MORE_KEYS[3]))


def sim_key_slots(full=()):
    """(b) six topology keys (zone, rack and four more custom keys, 65-70 values each); the apps on the fifth and
    sixth key take key slots 4 and 5, which tdom serves from HBM.  Besides the widened cluster's apps, nodes 6 and 7
    each carry a pod that must join an anchor pod in node 8's cage / node 9's pdu domain (no other node shares it):
    their simulations need no NodeClaim exactly when that node's domain in slot 4 / 5 is read right.
    full: receivers without room (the dependence check)."""
    keys = [(RACK, 70)] + [(k, 65 + i) for i, k in enumerate(MORE_KEYS)]
    apps = _apps([ZONE, RACK] + MORE_KEYS, n_spread=1)
    snap = wide_cluster(10, 6, 66, apps, seed=502, keys=keys)
    for r, m, key in SLOT_PAIRS:
        snap["stateNodes"][r]["available"] = {k: "0" for k in ROOM} if r in full else dict(ROOM)
        _anchor_and_mover(snap, r, m, key)
    return {"kind": "cons", "snapshot": snap, "cell": "key-slots", "keys": [ZONE, RACK] + MORE_KEYS,
            "movers": {snap["stateNodes"][m]["name"]: (snap["stateNodes"][r]["name"], key) for r, m, key in SLOT_PAIRS}}


def sim_non_small():
    """(c) 130 zones x 20 zonal apps (2600 count words): the groups past the 2048-word prefix are read and written
    through the simulations' copy-on-write bitmap."""
    apps = _apps([ZONE], n_spread=3) * 4
    return {"kind": "cons", "snapshot": wide_cluster(10, 8, 130, apps, seed=503), "cell": "non-small"}


def strip_apps(snap, drop):
    """The cluster with the topology constraints of the pods `drop(app index, spec)` selects taken off (the pods stay,
    unconstrained): what the answer is without those groups.  App index: NN of a widened cluster's wide-NN, else None."""
    s = copy.deepcopy(snap)
    pods = s["pendingPods"] + [p for n in s["stateNodes"] for p in n["pods"]] + s.get("clusterPods", [])
    for p in pods:
        app = p["metadata"]["labels"].get("app", "")
        if drop(int(app[5:]) if app.startswith("wide-") else None, p["spec"]):
            p["spec"].pop("topologySpreadConstraints", None)
            p["spec"].pop("affinity", None)
    return s


def spec_keys(spec):
    """The topology keys a pod spec's constraints name."""
    keys = {c["topologyKey"] for c in spec.get("topologySpreadConstraints", [])}
    for kind in ("podAffinity", "podAntiAffinity"):
        for t in spec.get("affinity", {}).get(kind, {}).get("requiredDuringSchedulingIgnoredDuringExecution", []):
            keys.add(t["topologyKey"])
    return keys


MANY_NODES = 260
RECEIVERS = (255, 256, 258)  # the only nodes with room: the last of the LDS window, the first past it, one beyond
MOVERS = (3, 130, 257)       # candidates whose one pod must join the anchor pod on receiver 255 / 256 / 258


def sim_many_nodes(full=()):
    """(d) 260 nodes x 1 pod over 69 zones and 73 racks.  Every node is full but the three receivers, each alone in a
    zone and a rack of its own and running an anchor pod.  Mover m's single pod requires pod affinity to anchor m's
    app (zone for receivers 255 and 258, rack for 256): it fits receiver m alone, so the mover's simulation is a
    delete exactly when the kernel reads that node's domain right, and needs a NodeClaim otherwise.  The other
    candidates (20 in all, two of them past index 256) carry the widened cluster's spread / affinity / anti-affinity
    pods.  full: receivers made full as well (the dependence check).  The oracle's pass with every simulation takes
    0.4 s (measured; 39 simulations)."""
    cands = sorted(set(range(5, 200, 13)) | {254, 259} | set(MOVERS))
    apps = _apps([ZONE, RACK], n_spread=1)
    snap = wide_cluster(MANY_NODES, 1, 69, apps, seed=504, keys=[(RACK, 73)], candidates=cands, it_range=(3, 12),
                        n_pending=0)
    zones, racks = names(ZONE, 69), names(RACK, 73)
    nodes = snap["stateNodes"]
    for j, n in enumerate(nodes):  # the last three zones and racks are the receivers' own
        if n["labels"][ZONE] in zones[66:]:
            n["labels"][ZONE] = zones[j % 66]
        if n["labels"][RACK] in racks[70:]:
            n["labels"][RACK] = racks[j % 70]
        if j not in RECEIVERS or j in full:
            n["available"] = {k: "0" for k in n["available"]}
    for i, (r, m) in enumerate(zip(RECEIVERS, MOVERS)):
        nodes[r]["labels"][ZONE], nodes[r]["labels"][RACK] = zones[66 + i], racks[70 + i]
        if r not in full:
            nodes[r]["available"] = dict(ROOM)
        _anchor_and_mover(snap, r, m, RACK if r == 256 else ZONE, alone=True)
    return {"kind": "cons", "snapshot": snap, "cell": "many-nodes", "candidates": cands,
            "movers": {nodes[m]["name"]: nodes[r]["name"] for r, m in zip(RECEIVERS, MOVERS)}}


DRIFT_ZONES = (10, 69, 0, 40, 64, 31)  # the six nodes' zones


def drift_wide_zones():
    """A Drift command over six full nodes in 70 zones, all drifted, node 0 first.  Its two pods cannot share an
    instance type (40 and 39 of at most 60 cpu), so the command has two replacements whose requirements the pick
    exports: one pod refuses the zones of app d-x (zones 0 and 40 hold it), leaving a zone set of 68 values over three
    requirement words; the other follows its anchor into zone 69, a single bit of the third word."""
    import disrupt_cases as dc

    snap = wide_cluster(6, 0, 70, [lambda app: {}], seed=505, n_pending=0)
    zones = names(ZONE, 70)
    nodes = snap["stateNodes"]
    for n, z in zip(nodes, DRIFT_ZONES):
        n["labels"][ZONE] = zones[z]
        dc.fill(n)

    def bind(i, at, cpu, app, affinity=None):
        p = dc.bound_pod(600000 + i, nodes[at]["name"], cpu)
        p["metadata"]["labels"]["app"] = app
        if affinity:
            p["spec"]["affinity"] = affinity
        nodes[at]["pods"].append(p)
        snap["clusterPods"].append(p)

    bind(0, 0, "40", "d-anti", pod_affinity(ZONE, "d-x", anti=True))
    bind(1, 0, "39", "d-aff", pod_affinity(ZONE, "d-anchor"))
    bind(2, 1, "100m", "d-anchor")
    bind(3, 2, "100m", "d-x")
    bind(4, 3, "100m", "d-x")
    bind(5, 4, "100m", "d-fill")  # (a drifted node without pods would be deleted before any simulation)
    bind(6, 5, "100m", "d-fill")
    dc.mark(snap, "drift", seed=5)
    first = min(nodes, key=lambda n: n["nodeClaimConditions"][1]["lastTransitionTime"])
    first["nodeClaimConditions"], nodes[0]["nodeClaimConditions"] = nodes[0]["nodeClaimConditions"], first["nodeClaimConditions"]
    return {"kind": "disrupt", "snapshot": snap, "cell": "drift-wide-zones", "candidate": nodes[0]["name"],
            "refused": [zones[0], zones[40]], "anchor": zones[69]}


# ---- the case table ----------------------------------------------------------------------------------------------
def _grid():
    cases = {}

    def add(name, fn, *args, **kw):
        assert name not in cases, name
        cases[name] = functools.partial(fn, *args, **kw)

    for nv in NVS:
        for gtype in TYPES:
            for pos in positions(nv):
                add("zone-%d-%s-p%d" % (nv, gtype, pos), solve_case, ZONE, nv, gtype, pos)
    for gtype in TYPES + ("inverse",):  # the custom key, two strides
        for pos in positions(65):
            add("rack-65-%s-p%d" % (gtype, pos), solve_case, RACK, 65, gtype, pos)
    for nv in (65, 129):
        for pos in positions(nv):
            add("zone-%d-inverse-p%d" % (nv, pos), solve_case, ZONE, nv, "inverse", pos)
    for pos in (0, 31, 32, 63, 64):  # ties, exclusions and the bootstrap minima across words and strides
        add("zone-129-spread-tie-p%d" % pos, solve_case, ZONE, 129, "spread-tie", pos)
        add("zone-129-affinity-bootstrap-p%d" % pos, solve_case, ZONE, 129, "affinity-bootstrap", pos)
    for pos in (32, 33, 64, 65, 128):
        add("zone-129-spread-notin-p%d" % pos, solve_case, ZONE, 129, "spread-notin", pos)
    for gtype in TYPES + ("inverse",):  # every placement target per type, the deciding domain in the second stride
        for target in TARGETS[1:]:
            add("zone-65-%s-%s" % (gtype, target), solve_case, ZONE, 65, gtype, 64, target)
    for target in ("open", "unlabelled", "error"):
        add("rack-65-spread-%s" % target, solve_case, RACK, 65, "spread", 64, target)
    for m in (64, 65, 66):
        add("zone-65-minDomains-%d" % m, min_domains_case, m)
    return cases


SOLVE_CASES = _grid()
CLOSED_FORM = [(kind, nv) for kind in ("even", "mindom", "anti") for nv in (65, 129)]
CONS_CASES = {"wide-zones": sim_wide_zones, "key-slots": sim_key_slots, "non-small": sim_non_small,
              "many-nodes": sim_many_nodes}


@functools.lru_cache(maxsize=None)
def solve(name):
    return SOLVE_CASES[name]()


@functools.lru_cache(maxsize=None)
def oracle_solve(name):
    """The oracle's canonical Results of a Solve case, computed once."""
    from oracle import bridge

    doc, _ = bridge.solve(json.dumps(solve(name)["snapshot"]))
    doc.pop("stats", None)
    return doc


@functools.lru_cache(maxsize=None)
def cons(name):
    return CONS_CASES[name]()


@functools.lru_cache(maxsize=None)
def oracle_cons(name, all_sims):
    """The oracle's consolidation document of a simulation case, computed once per all_sims."""
    from oracle import bridge

    return bridge.consolidate(json.dumps(cons(name)["snapshot"]), all_sims=all_sims)[0]


def moved(name):
    """The case rebuilt with the deciding domain at position 1 (for the dependence check)."""
    fn = SOLVE_CASES[name]
    if fn.func is not solve_case:
        return None
    key, nv, gtype, pos = fn.args[:4]
    at = 1 if gtype != "spread-notin" else 2  # (the excluded domain sits before it)
    return solve_case(key, nv, gtype, at, *fn.args[4:])


# ---- reading an answer -------------------------------------------------------------------------------------------
def claim_values(claim, key):
    """The values of `key In [...]` among a NodeClaim's requirements (None: the key is not restricted to a set)."""
    for r in claim["requirements"]:
        m = re.match(r"^(\S+) In \[(.*)\]$", r)
        if m and m.group(1) == key:
            return m.group(2).split()
    return None


def where(results, pod):
    """("claim", index) / ("node", name) / ("error", text) for a pod of a canonical Results."""
    for i, c in enumerate(results["newNodeClaims"]):
        if pod in c["pods"]:
            return "claim", i
    for n in results["existingNodes"]:
        if pod in n["pods"]:
            return "node", n["name"]
    return "error", results["podErrors"][str(pod)]


def deciding_domain(case, results):
    """The domain the case's pod ended in, as the answer shows it; for an error, the domain the message singles out."""
    kind, at = where(results, case["pod"])
    key = case["key"]
    if kind == "claim":
        vals = claim_values(results["newNodeClaims"][at], key)
        return kind, vals[0] if vals and len(vals) == 1 else vals
    if kind == "node":
        node = next(n for n in case["snapshot"]["stateNodes"] if n["name"] == at)
        if key in node["labels"]:
            return kind, node["labels"][key]
        # an unlabelled node: the probes it then admitted name the domain it took
        took = sorted(d for p, d in case["probes"].items() if where(results, p) == ("node", at))
        return "unlabelled", took[0] if len(took) == 1 else took
    m = re.findall(r"([\w.-]+):2\b", at[at.find("counts = map["):]) if "counts = map[" in at else []
    return kind, m[0] if len(m) == 1 else m
