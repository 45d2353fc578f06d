"""k_static_templates and k_static_nodes (ks_problem_static_feasibility, where = 0) against the same definitions on
the host (where = 1, checked against the oracle by tests/test_static_feasibility_host.py), word for word on all five
arrays, on the problems of tests/static_feasibility_cases.py.  Shapes pinned: TW 1, 1, 1, 2, 2, 3; row counts that
are no multiple of a block's four waves (the last block has idle waves); NWN with a ragged last word at N = 33, 65
and 257; a second block of k_static_nodes at N = 257.  The output buffers are pre-filled with 0xA5 bytes, so a word a
kernel fails to store shows as 0xA5A5A5A5: a failing row must be all zero.

Then the bound against the Solve on three random problems without topology, one problem compared with the oracle
protocol directly, and the timing accessor."""
import json

import numpy as np
import pytest

import static_feasibility_cases as sc
from karpenter_amd import Scheduler
from oracle import bridge

pytestmark = pytest.mark.gpu

ARRAYS = ("tpl_code", "tpl_count", "tpl_options", "node_bits", "node_count")


def _both(snap):
    sch = Scheduler(json.dumps(snap))
    try:
        return sch.static_feasibility(where="device"), sch.static_feasibility(where="host")
    finally:
        sch.close()


@pytest.mark.parametrize("name", sc.ALL_PROBLEMS)
def test_device_equals_host(name):
    dev, host = _both(sc.problem(name))
    assert dev.meta == host.meta
    for a in ARRAYS:
        g, w = getattr(dev, a), getattr(host, a)
        assert g.shape == w.shape and g.dtype == w.dtype, a
        bad = np.argwhere(g != w)
        assert not len(bad), "%s differs first at %s: device %#x, host %#x" % (a, bad[0], int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))
    sc.check_shape(dev)
    assert not (dev.tpl_options[dev.tpl_count == 0] != 0).any()
    for a in ("tpl_code", "tpl_options", "node_bits"):
        assert not (getattr(dev, a) == 0xA5A5A5A5).any(), a
    assert dev.kernel_ms > 0 and dev.templates_ms > 0 and (dev.nodes_ms > 0 or dev.meta["N"] == 0)
    assert dev.bytes_written == sum(getattr(dev, a).nbytes for a in ARRAYS)
    assert dev.bytes_read == host.bytes_read > 0


def test_pinned_shapes():
    tw = [_both(sc.problem("list-%d" % n))[0].meta["TW"] for n in sc.LIST_SIZES]
    assert tw == [1, 1, 1, 2, 2, 3]
    rows = []
    for name in sc.TEMPLATE_PROBLEMS:
        m = _both(sc.problem(name))[0].meta
        rows.append(m["S"] * m["NTPL"])
    assert any(r % 4 for r in rows), rows  # a last block with idle waves
    for n in (33, 65, 257):
        m = _both(sc.problem("nodes-%d" % n))[0].meta
        assert m["NWN"] == n // 32 + 1 and n % 32 == 1


@pytest.mark.parametrize("seed", sc.SOLVE_SEEDS)
def test_bounds_the_solve(seed):
    """A clear bit means never: every placement of the GPU Solve lies inside the matrix (sc.check_bounds_solve: for
    every pod without a state in meta["undefinedKeyStates"], where a clear bit holds for a fresh target only)."""
    snap = sc.solve_problem(seed)
    sch = Scheduler(json.dumps(snap))
    try:
        f = sch.static_feasibility(where="device")
        h = sch.static_feasibility(where="host")
        res = sch.solve(device=0)
    finally:
        sch.close()
    for a in ARRAYS:
        assert (getattr(f, a) == getattr(h, a)).all(), a
    checked, _ = sc.check_bounds_solve(f, res.existing_nodes, res.new_nodeclaims, res.pod_errors)
    assert checked > 50


def test_device_matches_oracle():
    """One problem straight against the oracle protocol: three templates (TW = 2, relaxing chains) plus 33 nodes."""
    snap = dict(sc.problem("three-templates"))
    sch = Scheduler(json.dumps(snap))
    try:
        f = sch.static_feasibility(where="device")
    finally:
        sch.close()
    assert sc.check_against_oracle(bridge, snap, f) == len(snap["pods"]) * 3
    nodes = sc.problem("nodes-33")
    sch = Scheduler(json.dumps(nodes))
    try:
        f = sch.static_feasibility(where="device")
    finally:
        sch.close()
    assert sc.check_against_oracle(bridge, nodes, f) == len(nodes["pods"]) * (1 + 33)


def test_c_client_on_the_device(tmp_path):
    snap = sc.problem("three-templates")
    doc = sc.c_client("device", snap, tmp_path)
    sc.c_client_agrees(doc, _both(snap)[1])
    assert doc["timed"] is True
