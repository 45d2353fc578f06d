"""Oracle versus GPU, whole canonical documents, on problems whose pods carry creation times: the generators of
tests/test_solve_gpu.py and tests/test_cons_gpu.py with their pods stamped (a few distinct seconds, many pods per
second, the stamps falling while the uids rise), so the queue's third key component decides among pods equal in cpu and
memory; and the prefix probe of tests/test_queue_reference.py, whose scheduled set is the queue's first k pods."""
import json

import pytest

import problems
import queue_cases as qc
from karpenter_amd import Consolidator, Scheduler, queue_inputs, synth
from oracle import bridge

pytestmark = pytest.mark.gpu


def _solve_both(snap):
    s = json.dumps(snap)
    want, _ = bridge.solve(s)
    want.pop("stats", None)
    sch = Scheduler(s)
    try:
        got = sch.solve()
    finally:
        sch.close()
    return want, got


def _stamped(snap):
    qc.stamp_pods(snap["pods"])
    inp = queue_inputs(snap)
    assert inp["skBits"][2] > 0, "the pods must differ in their creation second"
    return snap


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_random_problem_with_stamps(seed):
    want, got = _solve_both(_stamped(problems.random_problem(seed, n_pods=200)))
    assert got.canonical() == want


@pytest.mark.parametrize("seed", [460, 461])
def test_lean_problem_with_stamps(seed):
    snap = _stamped(synth.benchmark_snapshot(3000, 60, seed, diverse=False))
    want, got = _solve_both(snap)
    assert got.stats["route"]["lean"] == 1
    assert got.canonical() == want


@pytest.mark.parametrize("kind", ["stamps-oppose-uids", "equal-stamps"])
def test_prefix_probe_on_the_gpu(kind):
    import test_queue_reference as ref

    pairs = ref._probe_pods(kind)
    order = ref._probe_reference(pairs)
    for k in (1, 4, len(pairs) - 1):
        snap = qc.prefix_probe(pairs, k)
        want, got = _solve_both(snap)
        assert got.canonical() == want
        assert qc.scheduled_uids(got.doc, snap) == set(order[:k])


@pytest.mark.parametrize("case", [dict(n_nodes=12, pods_per_node=6, n_its=40, it_range=(8, 24), seed=1),
                                  dict(n_nodes=30, pods_per_node=12, n_its=80, it_range=(10, 40), seed=3, n_pending=5)],
                         ids=["c1", "c3"])
def test_cluster_with_stamps(case):
    snap = synth.cluster_snapshot(**case)
    qc.stamp_pods([p for node in snap["stateNodes"] for p in node["pods"]] + snap["pendingPods"])
    s = json.dumps(snap)
    for all_sims in (True, False):
        want, _ = bridge.consolidate(s, all_sims=all_sims)
        c = Consolidator(s)
        try:
            got = c.consolidate(all_sims=all_sims)
        finally:
            c.close()
        got.pop("kernel_ms")
        assert got == want
