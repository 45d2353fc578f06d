"""The static feasibility matrix on the host (ks_problem_static_feasibility, where = 1) against the oracle protocol
of tests/static_feasibility_cases.py, on every (pod, template) and (pod, node) pair of its problems: instance-type
lists of 1 .. 65 (TW 1 .. 3), three templates, R = 3 and R = 5, requests that decide Fits by one milli-CPU, NodePool
limits that keep one, none and some of the candidates, unavailable and partial offerings, every operator on a
single-valued key, In / NotIn on zone and capacity type, taints with and without the toleration, chains that relax;
1 .. 257 nodes with exact and one-unit-short room, taints, missing labels and held host ports.  No pair is skipped.
Then the argument checks, the refusal of negative requests and the meta document.  No device is used."""
import ctypes
import json

import pytest

import static_feasibility_cases as sc
from karpenter_amd import KsError, Scheduler, lib
from oracle import bridge


def _host(snap):
    sch = Scheduler.host_only(json.dumps(snap))
    try:
        return sch.static_feasibility(where="host")
    finally:
        sch.close()


@pytest.mark.parametrize("name", sc.ALL_PROBLEMS)
def test_host_matches_oracle(name):
    snap = sc.problem(name)
    assert len(snap["pods"]) <= 24
    f = _host(snap)
    sc.check_shape(f)
    pairs = sc.check_against_oracle(bridge, snap, f)
    assert pairs == len(snap["pods"]) * (len(snap["nodeClaimTemplates"]) + len(snap["stateNodes"]))


def test_problems_cover_what_they_claim():
    """The cases decide what their names say (so the oracle comparison above exercises those paths)."""
    c = None
    tw = []
    for n in sc.LIST_SIZES:
        f = _host(sc.problem("list-%d" % n))
        c = f.codes
        tw.append(f.meta["TW"])
        codes = {int(x) & 0xff for x in f.tpl_code.ravel()}
        assert {c["FC_NONE"], c["FC_TAINTS"]} <= codes, (n, codes)
        # the last two pods: one milli-CPU too many for the largest type, then a fit by exactly zero
        over, exact = f.meta["podState0"][-2], f.meta["podState0"][-1]
        assert f.tpl_count[over, 0] == 0 and int(f.tpl_code[over, 0]) & 0xff == c["FC_NO_IT"]
        assert not (int(f.tpl_code[over, 0]) >> 8) & c["FF_REQ_FITS"] and (int(f.tpl_code[over, 0]) >> 8) & c["FF_REQ_OFF"]
        assert f.tpl_count[exact, 0] >= 1
    assert tw == [1, 1, 1, 2, 2, 3]
    f = _host(sc.problem("list-65"))
    assert {c["FC_NONE"], c["FC_TAINTS"], c["FC_COMPAT"], c["FC_NO_IT"]} <= {int(x) & 0xff for x in f.tpl_code.ravel()}
    full = len(f.meta["templates"][0]["instanceTypes"])
    assert f.meta["TW"] == 3 and any(0 < int(x) < full for x in f.tpl_count.ravel())
    one, none, some = (_host(sc.problem(k)) for k in ("limit-one", "limit-none", "limit-subset"))
    assert (none.tpl_code == c["FC_LIMITS"]).all() and not none.tpl_options.any()
    assert 0 < one.tpl_count.max() <= 1 and 1 < some.tpl_count.max() <= 8
    assert none.unschedulable().keys() == set(range(len(sc.problem("limit-none")["pods"])))
    f = _host(sc.problem("three-templates"))
    assert f.meta["TW"] == 2 and [len(t["instanceTypes"]) for t in f.meta["templates"]] == [40, 33, 7]
    assert max(f.meta["podNState"]) >= 3 and 1 in f.meta["podNState"]
    f = _host(sc.problem("five-resources"))
    assert 0 < f.tpl_count[f.meta["podState0"][1], 0] < f.tpl_count[f.meta["podState0"][0], 0]
    for n in sc.NODE_SIZES:
        f = _host(sc.problem("nodes-%d" % n))
        assert f.meta["N"] == n and f.meta["NWN"] == (n + 31) // 32
        if n >= 4:  # the exact-fit pod lands on node 0 and on none of the three nodes one unit short
            names = f.nodes(len(f.meta["podState0"]) - 2, 0)
            assert "node-0000" in names and not {"node-0001", "node-0002", "node-0003"} & set(names)
            assert 0 < f.node_count.max() < n


def test_arguments_and_refusals():
    l = lib()
    snap = sc.problem("list-31")
    sch = Scheduler.host_only(json.dumps(snap))
    try:
        with pytest.raises(KsError) as e:
            sch.static_feasibility(where="nowhere")
        assert e.value.code == -6
        f = sch.static_feasibility(where="host")
        assert f.kernel_ms == 0 and f.bytes_read > 0
        assert f.bytes_written == sum(a.nbytes for a in (f.tpl_code, f.tpl_count, f.tpl_options, f.node_bits, f.node_count))
        with pytest.raises(IndexError):
            f.options(len(snap["pods"]), 0, 0)
        with pytest.raises(IndexError):
            f.nodes(0, f.meta["podNState"][0])
        # the C entries: out-of-range arguments are KS_ERR_ARG; freeing NULL is a no-op
        vp = ctypes.c_void_p
        l.ks_problem_static_feasibility.argtypes = [vp, vp, ctypes.c_int, ctypes.POINTER(vp)]
        h = vp()
        assert l.ks_problem_static_feasibility(sch._h, None, 2, ctypes.byref(h)) == -6
        assert l.ks_problem_static_feasibility(sch._h, None, -1, ctypes.byref(h)) == -6
        assert l.ks_problem_static_feasibility(None, None, 1, ctypes.byref(h)) == -6
        assert l.ks_problem_static_feasibility(sch._h, None, 1, None) == -6
        assert l.ks_problem_static_feasibility(sch._h, None, 0, ctypes.byref(h)) == -6  # no device behind this problem
        assert l.ks_problem_static_feasibility(sch._h, None, 1, ctypes.byref(h)) == 0
        l.ks_feasibility_template_row.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
        l.ks_feasibility_node_row.argtypes = [vp, ctypes.c_int, vp, vp, vp]
        S, NTPL = f.meta["S"], f.meta["NTPL"]
        code, cnt, words, nw = ctypes.c_uint32(), ctypes.c_int32(), vp(), ctypes.c_int()
        for s, t in ((-1, 0), (S, 0), (0, -1), (0, NTPL)):
            assert l.ks_feasibility_template_row(h, s, t, None, None, None, None) == -6
        for s in (-1, S):
            assert l.ks_feasibility_node_row(h, s, None, None, None) == -6
        assert l.ks_feasibility_template_row(h, S - 1, NTPL - 1, ctypes.byref(code), ctypes.byref(cnt), ctypes.byref(words),
                                             ctypes.byref(nw)) == 0
        assert (code.value, cnt.value, nw.value) == (int(f.tpl_code[S - 1, NTPL - 1]), int(f.tpl_count[S - 1, NTPL - 1]), f.meta["TW"])
        got = list((ctypes.c_uint32 * nw.value).from_address(words.value))
        assert got == [int(x) for x in f.tpl_options[S - 1, NTPL - 1]]
        assert l.ks_feasibility_node_row(h, 0, ctypes.byref(cnt), ctypes.byref(words), ctypes.byref(nw)) == 0
        assert (cnt.value, nw.value) == (int(f.node_count[0]), f.meta["NWN"])
        l.ks_feasibility_meta.argtypes = [vp, vp]
        assert l.ks_feasibility_meta(h, None) == -6
        l.ks_feasibility_free.argtypes = [vp]
        l.ks_feasibility_free(h)
        l.ks_feasibility_free(None)
    finally:
        sch.close()


def test_negative_requests_are_refused():
    sch = Scheduler.host_only(json.dumps(sc.negative_request_case()))
    try:
        with pytest.raises(KsError) as e:
            sch.static_feasibility(where="host")
        assert e.value.code == -2 and "negative" in str(e.value)
    finally:
        sch.close()


def test_host_only_problem_does_not_solve():
    sch = Scheduler.host_only(json.dumps(sc.problem("list-1")))
    try:
        with pytest.raises(KsError) as e:
            sch.solve()
        assert e.value.code == -4
        assert len(sch.save()) > 0
    finally:
        sch.close()


def test_bound_on_the_oracle_solve_and_its_exception():
    """The matrix bounds the reference's own Solve for every pod it claims to (sc.check_bounds_solve), and the pods
    it does not claim to are a real exception: in seed 14's Solve one of them shares a NodeClaim that its own rows
    refuse (another pod defined the label key first)."""
    outside = {}
    for seed in sc.SOLVE_SEEDS:
        snap = sc.solve_problem(seed)
        f = _host(snap)
        res, _ = bridge.solve(json.dumps(snap))
        checked, outside[seed] = sc.check_bounds_solve(f, res["existingNodes"], res["newNodeClaims"], res["podErrors"])
        assert checked > 50 and f.meta["undefinedKeyStates"]
    assert outside[14] >= 1


def test_c_client_on_the_host(tmp_path):
    """tests/c/feasibility_check.c: the row accessors from plain C99 give the Python binding's arrays."""
    for name in ("three-templates", "nodes-33"):
        doc = sc.c_client("host", sc.problem(name), tmp_path)
        sc.c_client_agrees(doc, _host(sc.problem(name)))
        assert doc["timed"] is False


def test_meta_indexes_every_array():
    snap = sc.problem("three-templates")
    f = _host(snap)
    m = f.meta
    assert m["ignores"] == ["topology", "volumeLimits"] and m["topologyStates"] == [] and m["volAny"] == 0
    assert m["undefinedKeyStates"] == []  # every key these pods name is well-known or on every template
    assert [t["nodePool"] for t in m["templates"]] == [t["metadata"]["name"] for t in snap["nodeClaimTemplates"]]
    its = snap["instanceTypes"]
    for t, tpl in zip(m["templates"], snap["nodeClaimTemplates"]):
        assert t["instanceTypes"] == [its[i]["name"] for i in snap["instanceTypesByNodePool"][tpl["metadata"]["name"]]]
    assert set(m["codes"]) == {"FC_NONE", "FC_LIMITS", "FC_TAINTS", "FC_COMPAT", "FC_NO_IT", "FF_REQ", "FF_FITS", "FF_OFF",
                               "FF_REQ_FITS", "FF_REQ_OFF", "FF_FITS_OFF"}
    assert len(m["podState0"]) == len(snap["pods"]) == len(m["podNState"])
    nodes = _host(sc.problem("nodes-33")).meta
    assert sorted(nodes["nodes"]) == sorted(n["name"] for n in sc.problem("nodes-33")["stateNodes"])
    # a problem with spread constraints names the states that own the groups the matrix ignores
    import problems
    tf = _host(problems.random_problem(11, n_pods=40, n_nodes=6, topology=True))
    assert tf.meta["topologyStates"] and all(0 <= s < tf.meta["S"] for s in tf.meta["topologyStates"])
