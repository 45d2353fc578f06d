"""The templates' Pareto fronts the LEAN Solve's run capacity reads (ks_host.cpp pareto_fronts, KS_RUN_FRONT):
template position q is dropped when another position's Allocatable is >= q's in every resource, the lowest
position of equal vectors stays, and a front of more than 64 positions is given up (an empty list: the kernel then
scans every option).  Host only: ks_problem_inspect reports the lists; the reference is the definition itself,
on Allocatable = capacity - kubeReserved in exact integers."""
import random

import run_front_cases as cases
from karpenter_amd import synth
from karpenter_amd.scheduler import inspect

GI = 1 << 30


def _alloc(it):
    cap, ov = it["capacity"], it["overhead"]["kubeReserved"]
    assert ov == {"cpu": "100m", "memory": "10Mi"} and cap["memory"].endswith("Gi")
    return (int(cap["cpu"]) * 1000 - 100, int(cap["memory"][:-2]) * GI - (10 << 20), int(cap["pods"]))


def _front(vecs):
    keep = []
    for q, x in enumerate(vecs):
        dominated = any(all(a >= b for a, b in zip(y, x)) and (y != x or p < q) for p, y in enumerate(vecs) if p != q)
        if not dominated:
            keep.append(q)
    return keep if len(keep) <= 64 else []


def _snapshot(types, order=None):
    snap = synth.benchmark_snapshot(4, 1, 1, diverse=False)
    snap["instanceTypes"] = types
    snap["instanceTypesByNodePool"] = {"default-pool": list(order if order is not None else range(len(types)))}
    return snap


def _check(snap):
    types = snap["instanceTypes"]
    got = inspect(snap)["paretoFronts"]
    want = [_front([_alloc(types[i]) for i in snap["instanceTypesByNodePool"][t["metadata"]["name"]]])
            for t in snap["nodeClaimTemplates"]]
    assert got == want
    return got


def test_chain_catalogue_has_a_front_of_one():
    assert _check(synth.config2(10)) == [[399]]
    assert _check(cases.chain()) == [[19]]


def test_non_chain_catalogue_and_the_tie():
    """fake-it-11, cpu-big, mem-big and pods-big; cpu-big-twin (position 15) ties with cpu-big (12) and goes."""
    assert _check(cases.non_chain(1, 1, 1)) == [[11, 12, 13, 14]]


def test_positions_are_the_template_s_not_the_catalogue_s():
    types = cases.non_chain(1, 1, 1)["instanceTypes"]
    order = list(reversed(range(len(types))))  # cpu-big-twin now stands before cpu-big
    assert _check(_snapshot(types, order)) == [[0, 1, 2, 4]]
    snap = _snapshot(types, [3, 15, 7])
    assert _check(snap) == [[1, 2]]  # fake-it-7 holds more pods than the twin
    # two templates over different lists
    snap = synth.benchmark_snapshot(4, 14, 1, diverse=False)
    snap["nodeClaimTemplates"] = [synth.node_pool("a-pool"), synth.node_pool("b-pool")]
    snap["instanceTypesByNodePool"] = {"a-pool": list(range(8)), "b-pool": list(range(13, 3, -1))}
    assert _check(snap) == [[7], [0]]


def test_random_catalogues_against_the_definition():
    rng = random.Random(10)
    for n in (1, 2, 3, 17, 64, 65, 130):
        for spread in (2, 5, 40):  # few distinct values: many ties and dominated types; many: wide fronts
            types = [synth.fake_instance_type("t-%d" % i, rng.randint(1, spread), rng.randint(1, spread),
                                              pods=rng.randint(1, spread)) for i in range(n)]
            _check(_snapshot(types))


def test_a_front_of_64_is_kept_and_one_of_65_given_up():
    def anti(n):
        return [synth.fake_instance_type("t-%d" % i, i + 1, 100 - i, pods=10) for i in range(n)]
    assert _check(_snapshot(anti(64))) == [list(range(64))]
    assert _check(_snapshot(anti(65))) == [[]]
    # 65 on the front and a type that dominates them all: a front of one again
    assert _check(_snapshot(anti(65) + [synth.fake_instance_type("top", 200, 200, pods=10)])) == [[65]]
