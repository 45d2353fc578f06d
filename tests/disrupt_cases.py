"""Snapshots for the Drift / Expiration tests (ks_cons_disrupt, ks_cons_inspect_disrupt): small clusters whose
shapes are the smallest at which the candidate selection, the pick or the export can go wrong."""
import copy
import random

from karpenter_amd import synth

KIND = {"drift": "Drifted", "expiration": "Expired"}


def mark(snap, method="drift", names=None, status="True", seed=1, tie=False):
    """Give the nodes (all, or `names`) the method's condition, with distinct transition times in an order unlike
    the node order (tie: one shared time)."""
    nodes = [n for n in snap["stateNodes"] if names is None or n["name"] in names]
    offs = list(range(len(nodes)))
    random.Random(seed).shuffle(offs)
    for n, k in zip(nodes, offs):
        at = synth.NOW - 100000 + (0 if tie else 61 * k)
        n["nodeClaimConditions"] = [{"type": "Ready", "status": "True", "lastTransitionTime": synth._fmt_time(synth.NOW - 5)},
                                    {"type": KIND[method], "status": status, "lastTransitionTime": synth._fmt_time(at)}]
    return snap


def small(seed=3, n=14, ppn=6, **kw):
    return synth.cluster_snapshot(n, ppn, n_its=40, it_range=(4, 20), seed=seed, **kw)


def fill(node):
    """No room left on the node."""
    node["available"] = {k: "0" for k in node["available"]}


def bound_pod(i, node, cpu, mem="64Mi", selector=None):
    p = synth.pod(i, cpu=cpu, mem=mem, node_selector=selector)
    p["spec"]["nodeName"] = node
    p["status"] = {"phase": "Running", "conditions": [{"type": "PodScheduled", "status": "True"}]}
    return p


def lean(n_nodes, n_its=40, pods_of=None, full=True, extra=None, type_cpu=None):
    """A resource-only (LEAN) cluster over fake.InstanceTypes(n_its) (i + 1 cpu each): node j holds the pods
    pods_of(j) returns ([(cpu, selector)]); every node has no room left (full) so a candidate's pods need new
    NodeClaims.  extra: {resource: capacity} every instance type also offers (more resource names)."""
    its = synth.fake_instance_types(n_its)
    if extra:
        its = [synth.fake_instance_type(t["name"], i + 1, 2 * (i + 1), pods=10 * (i + 1), extra_capacity=extra)
               for i, t in enumerate(its)]
    snap = synth.cluster_snapshot(n_nodes, 0, n_its=n_its, it_range=(min(4, n_its - 1), n_its), seed=11)
    snap["instanceTypes"] = its
    pid = 0
    for j, n in enumerate(snap["stateNodes"]):
        n["pods"] = []
        for cpu, sel, req in (pods_of(j) if pods_of else []):
            p = bound_pod(pid, n["name"], cpu, selector=sel)
            p["spec"]["containers"][0]["resources"]["requests"].update(req or {})
            n["pods"].append(p)
            pid += 1
        if full:
            fill(n)
    return snap


def claims_case(k):
    """The first drifted node's simulation needs k NodeClaims (0, 1, 2 or 70)."""
    if k == 0:  # room elsewhere
        snap = lean(4, pods_of=lambda j: [("500m", None, None)] * 2, full=False)
    elif k == 1:
        snap = lean(4, pods_of=lambda j: [("500m", None, None)] * 3)
    elif k == 2:  # 2 x 30 cpu: no type of 40 cpu holds both
        snap = lean(4, pods_of=lambda j: [("30", None, None)] * 2)
    else:  # 70 pods of 3 cpu, types of at most 4 cpu
        snap = lean(3, n_its=4, pods_of=lambda j: [("3", None, None)] * (70 if j == 0 else 1))
    mark(snap, "drift", seed=2)
    # the node with the most pods drifted first
    nodes = snap["stateNodes"]
    heavy = max(nodes, key=lambda n: len(n["pods"]))
    first = min(nodes, key=lambda n: n["nodeClaimConditions"][1]["lastTransitionTime"])
    heavy["nodeClaimConditions"], first["nodeClaimConditions"] = first["nodeClaimConditions"], heavy["nodeClaimConditions"]
    return snap


def types_case(n_its):
    """One replacement whose instance-type list spans more than one 32-bit word (33 types: 2 words, 65: 3)."""
    return mark(lean(3, n_its=n_its, pods_of=lambda j: [("100m", None, None)] * 2), "drift", seed=3)


def resources_case(extra):
    """3 resource names (cpu, memory, pods) or 5 (two extended resources every pod requests)."""
    ext = {"example.com/a": "64", "example.com/b": "64"} if extra else None
    req = {"example.com/a": "1", "example.com/b": "2"} if extra else None
    return mark(lean(3, pods_of=lambda j: [("500m", None, req)] * 3, extra=ext), "drift", seed=4)


NOWHERE = {"example.com/nowhere": "x"}  # a node selector no template or node offers


def count_case(n, schedulable):
    """n drifted candidates of one pod each; only `schedulable` ("last", "first", "none": positions of the
    method's order) can move its pod, the others' pod carries a node selector nothing offers."""
    snap = lean(n, n_its=8, pods_of=lambda j: [("500m", None, None)])
    mark(snap, "drift", seed=5)
    order = sorted(snap["stateNodes"], key=lambda x: x["nodeClaimConditions"][1]["lastTransitionTime"])
    keep = {"last": order[-1]["name"], "first": order[0]["name"], "none": None}[schedulable]
    for nd in snap["stateNodes"]:
        if nd["name"] != keep:
            nd["pods"][0]["spec"]["nodeSelector"] = dict(NOWHERE)
    return snap


def selectors_case():
    """Pods with node selectors: requirement-carrying simulations."""
    return mark(small(seed=21, n=12, pod_selectors=True, n_pending=2), "drift", seed=6)


def topology_case():
    """Topology spread / affinity apps, pending pods, uninitialized and not-ready nodes."""
    return mark(small(seed=22, n=16, topology=6, n_pending=3, uninitialized_frac=0.2, not_ready_frac=0.2),
                "drift", seed=7)


def never_pool(snap):
    """The same snapshot with the pool's consolidateAfter Never."""
    s = copy.deepcopy(snap)
    for key in ("nodePools", "nodeClaimTemplates"):
        for p in s[key]:
            p["spec"]["disruption"]["consolidateAfter"] = "Never"
    return s
