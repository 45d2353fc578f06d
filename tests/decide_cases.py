"""Clusters, virtual clocks and oracle-side need lists for the decision-replay route tests
(tests/test_decide_routes_gpu.py, tests/test_decide_preconditions.py, the C client's consolidate mode and the
multi-process leg).

A "shift" cluster is one where a clock cuts the multi-node search short of probes that have NodeClaims: the
requirement table a caller builds in ks_cons_needed_sims order (no clock) then holds rows the clocked replay never
reads, in front of rows it does read.  A "carry" cluster has probes re-run from pod objects earlier probes
relaxed."""
import functools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from karpenter_amd import synth  # noqa: E402
from oracle import bridge  # noqa: E402

SHIFT_FAMILY = dict(n_nodes=16, pods_per_node=8, n_its=40, it_range=(6, 30), topology=3, pod_selectors=True)
# TOPO_CASES seed 24 of test_cons_gpu.py (test_consolidation_timeouts_parity runs it at world 1, inline route)
TOPO24 = dict(n_nodes=25, pods_per_node=10, n_its=60, it_range=(8, 30), seed=24, pod_selectors=True, topology=3)

# name -> the clocks under which the clocked need list pairs other simulations than the clockless one
SHIFT = {
    "shift-305": [(0.0, 1000.0, 1.0)],
    "shift-326": [(2.0, 1000.0, 1.0)],
    "shift-303": [(0.0, 1000.0, 1.0)],
    "topo-24": [(60.0, 180.0, 25.0)],
}
# (the issue's seed 322 shifts at (2.0, 1000.0, 1.0) too; the CPU precondition test covers it, the GPU tests do not)
SHIFT_CPU_ONLY = {"shift-322": [(2.0, 1000.0, 1.0)]}
CARRY = ["carry-1", "carry-4", "carry-23", "carry-38", "late-carry"]
CLUSTERS = list(SHIFT) + CARRY + ["replace"]


@functools.lru_cache(maxsize=None)
def snapshot(name):
    """The cluster snapshot `name` as a JSON string."""
    if name.startswith("shift-"):
        return json.dumps(synth.cluster_snapshot(seed=int(name[6:]), **SHIFT_FAMILY))
    if name == "topo-24":
        return json.dumps(synth.cluster_snapshot(**TOPO24))
    if name == "replace":  # test_dist_cons_gpu._snapshot("replace"): spot/on-demand mix, replacements and deletes
        return json.dumps(synth.cluster_snapshot(40, 8, n_its=60, it_range=(6, 30), seed=11, spot_frac=0.5))
    import carry_scenarios as cs

    if name == "late-carry":
        return json.dumps(cs.make("late-carry", 0))
    s = int(name[6:])
    return json.dumps(cs.random_cluster(s, topology=s % 2 == 0))


@functools.lru_cache(maxsize=None)
def oracle(name, clock=None, all_sims=False):
    """The oracle's document (cached; callers must not change it)."""
    if clock is None:
        return bridge.consolidate(snapshot(name), all_sims=all_sims)[0]
    return bridge.consolidate_clock(snapshot(name), *clock, all_sims=all_sims)


def clocks(name):
    """None, then every cut of the multi-node search (k + 1 probes for k in 0..L-1, L the clockless path's length),
    then the fixed clocks.  (multi_timeout_s, single_timeout_s, sim_seconds); the reference's check is
    clock.Now().After(timeout), strict, made before each simulation, and the clock is advanced by repeated addition."""
    n = len(oracle(name)["multi"]["path"])
    return ([None] + [(float(k), 1000.0, 1.0) for k in range(n)] +
            [(0.25, 0.75, 0.125),   # exact in binary: 0.25 > 0.25 is false, so 3 probes run
             (0.3, 0.9, 0.1),       # 0.1 + 0.1 + 0.1 = 0.30000000000000004 > 0.3: 3 probes, not 4
             (1000.0, 4.0, 1.0),    # the single-node scan is abandoned with no command
             (60.0, 180.0, 25.0)])  # the existing timeout test's clock


def need_rows(doc):
    """The requirement-table rows a decision document renders, as (simulation, requirementsString): the non-carried
    probes of the multi-node path, then the single-node simulations, those with a NodeClaim.  (A carried probe's
    requirements come from its re-run, not from the table.)  Without all_sims ks_cons_needed_sims lists exactly
    these simulations in this order."""
    rows = []
    for p in doc["multi"]["path"]:
        if not p["carried"] and p["newNodeClaims"] > 0:
            rows.append((("multi", p["mid"]), p["claim0"]["requirementsString"]))
    for i, x in enumerate(doc["single"]["sims"]):
        if x["newNodeClaims"] > 0:
            rows.append((("single", i), x["claim0"]["requirementsString"]))
    return rows


def shifted_positions(clockless, clocked):
    """Positions of the clocked need list that pair, in the clockless list, another simulation whose requirement
    record differs: a table mapped by the wrong list renders these rows wrong."""
    a, b = need_rows(clockless), need_rows(clocked)
    return [i for i, (x, y) in enumerate(zip(a, b)) if x[0] != y[0] and x[1] != y[1]]


def _explain(a, b, path=""):
    if type(a) != type(b):
        return "%s: %r vs %r" % (path, a, b)
    if isinstance(a, dict):
        for k in sorted(set(a) | set(b)):
            if a.get(k) != b.get(k):
                return _explain(a.get(k), b.get(k), path + "." + k)
    elif isinstance(a, list):
        if len(a) != len(b):
            return "%s: len %d vs %d" % (path, len(a), len(b))
        for i, (x, y) in enumerate(zip(a, b)):
            if x != y:
                return _explain(x, y, "%s[%d]" % (path, i))
    return "%s: %r vs %r" % (path, a, b)


def first_diff(want, got):
    """None when the documents are equal, else the first differing field as "path: want vs got"."""
    return None if want == got else _explain(want, got)
