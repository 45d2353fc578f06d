"""k_feasibility and k_feasibility_nodes read back word for word (ks_problem_feasibility_rows) and compared, by exact
equality, with the plain reference of tests/feasibility_cases.py (checked against the oracle on the CPU by
tests/test_feasibility_reference.py) at the shapes where the kernels have structure:

  node rows         N = 1 .. 300: a partial word, the second word of a wave's ballot (the lane-32 store), the
                    other waves of a block, a second block, and the `w < NWN` / `w + 1 < NWN` guards at a ragged end;
  instance types    lists of 1 .. 2049 types: a partly filled and a full half-wave of k_feasibility<32>, the first
                    <64> shape, the full wave, its second pass, the clamped lanes past TW; three templates with
                    lists of unequal length and an odd row count (zero tails, the dead second half);
  value chunks      a single-valued key with 31 .. 100 values under NotIn (few and many values), Exists, Gt and Lt
                    from the pods and a NotIn from the NodePool, in both instantiations: the second chunk of the
                    complement ballots, and in <32> two rows with different keys, operators and trip counts in
                    the halves of one wave, an intolerant (zero) row beside a live one.

Words past a template's list and bits past N are compared too (the reference packs them as zero).  The consumers
run at the same edges end to end: rows on, rows off (KS_NO_NODE_ROWS / KS_NO_FEASIBILITY) and the oracle, whole
canonical documents."""
import json
import os

import pytest

import feasibility_cases as fc
from karpenter_amd import Scheduler, synth
from oracle import bridge

pytestmark = pytest.mark.gpu


def _read(snap, which):
    sch = Scheduler(json.dumps(snap))
    try:
        return sch.feasibility_rows(which)
    finally:
        sch.close()


def _first_diff(got, want):
    for w, (g, x) in enumerate(zip(got, want)):
        if int(g) != x:
            d = int(g) ^ x
            return 32 * w + (d & -d).bit_length() - 1
    return None


def _pod_text(snap, pi):
    spec = snap["pods"][pi]["spec"]
    return "pod %d %s tolerations=%s" % (pi, json.dumps(fc.pod_exprs(snap["pods"][pi])), json.dumps(spec.get("tolerations", [])))


def check_node_rows(snap):
    meta, words = _read(snap, 1)
    n = meta["N"]
    nwn = (n + 31) // 32
    assert n == len(snap["stateNodes"]) and sorted(meta["nodes"]) == sorted(x["name"] for x in snap["stateNodes"])
    ref = fc.node_rows(snap, meta["nodes"])
    assert words.size == meta["FNR"] * nwn
    seen = 0
    for pi, pod in enumerate(snap["pods"]):
        states, whole = fc.covered_states(snap, pod)
        if whole:
            assert meta["podNState"][pi] == len(states)
        for j in range(len(states)):
            s = meta["podState0"][pi] + j
            row = meta["stateNodeRow"][s]
            if (pi, j) not in ref:
                assert row == -1, "a state without label requirements has a node row"
                continue
            assert 0 <= row < meta["FNR"]
            seen += 1
            got, want = words[row * nwn:(row + 1) * nwn], fc.pack(ref[(pi, j)])
            if [int(x) for x in got] != want:
                b = _first_diff(got, want)
                node = meta["nodes"][b] if b < n else "(past N)"
                pytest.fail("node rows differ first at state %d (chain position %d), node %d %s: got %d; %s; got words %s, "
                            "want %s" % (s, j, b, node, (int(got[b >> 5]) >> (b & 31)) & 1, _pod_text(snap, pi),
                                         [hex(int(x)) for x in got], [hex(x) for x in want]))
    assert seen == meta["FNR"], "rows the reference does not cover"


def check_it_rows(snap):
    meta, words = _read(snap, 0)
    tw, ntpl = meta["TW"], meta["NTPL"]
    lists = [t["instanceTypes"] for t in meta["templates"]]
    assert [sorted(x) for x in lists] == [sorted(x) for x in fc.template_lists(snap)]
    assert set(meta["coveredKeys"]) == fc.covered_keys(snap)
    irr = fc.irregular_names(snap)
    for t, names in zip(meta["templates"], lists):
        assert t["irregular"] == (fc.pack([1 if x in irr else 0 for x in names]) + [0] * tw)[:tw]
    ref = fc.it_rows(snap, lists)
    assert words.size == meta["S"] * ntpl * tw
    seen = 0
    for pi, pod in enumerate(snap["pods"]):
        states, whole = fc.covered_states(snap, pod)
        if whole:
            assert meta["podNState"][pi] == len(states)
        for j in range(len(states)):
            s = meta["podState0"][pi] + j
            seen += 1
            for t in range(ntpl):
                bits = ref[(pi, j)][t]
                assert ((meta["stateTolTpl"][s] >> t) & 1) == (0 if bits is None else 1)
                want = (fc.pack(bits or []) + [0] * tw)[:tw]
                got = words[(s * ntpl + t) * tw:(s * ntpl + t + 1) * tw]
                if [int(x) for x in got] != want:
                    b = _first_diff(got, want)
                    name = lists[t][b] if b < len(lists[t]) else "(past the template's list of %d)" % len(lists[t])
                    pytest.fail("instance-type rows differ first at state %d (chain position %d), template %d %s, position "
                                "%d %s: got %d; %s; got word %s, want %s" % (
                                    s, j, t, snap["nodeClaimTemplates"][t]["metadata"]["name"], b, name,
                                    (int(got[b >> 5]) >> (b & 31)) & 1, _pod_text(snap, pi), hex(int(got[b >> 5])),
                                    hex(want[b >> 5])))
    assert seen == meta["S"], "states the reference does not cover"


@pytest.mark.parametrize("n", fc.NODE_SIZES)
def test_node_rows(n):
    check_node_rows(fc.node_snapshot(n))


@pytest.mark.parametrize("n", fc.SHAPE_SIZES)
def test_instance_type_rows_shape(n):
    check_it_rows(fc.shape_snapshot(n))


def test_instance_type_rows_three_templates():
    check_it_rows(fc.three_template_snapshot())


@pytest.mark.parametrize("v,gw", sorted(fc.VALUE_CASES))
def test_instance_type_rows_value_chunks(v, gw):
    check_it_rows(fc.value_snapshot(v, gw))


def test_rows_off_is_unsupported():
    from karpenter_amd import KsError
    snap = fc.node_snapshot(33)
    for which, var in ((0, "KS_NO_FEASIBILITY"), (1, "KS_NO_NODE_ROWS")):
        os.environ[var] = "1"
        try:
            with pytest.raises(KsError) as e:
                _read(snap, which)
        finally:
            os.environ.pop(var, None)
        assert e.value.code == -2


# --- the consumers at the same edges ---------------------------------------------------------------------

def _solve(snap_json, var, off):
    saved = os.environ.pop(var, None)
    if off:
        os.environ[var] = "1"
    try:
        sch = Scheduler(snap_json)
        r = sch.solve()
        sch.close()
        return r
    finally:
        os.environ.pop(var, None)
        if saved is not None:
            os.environ[var] = saved


def _on_off_oracle(snap, var):
    s = json.dumps(snap)
    on, off = _solve(s, var, False), _solve(s, var, True)
    assert on.canonical() == off.canonical()
    want, _ = bridge.solve(s)
    want.pop("stats", None)
    assert on.canonical() == want
    return on, off


@pytest.mark.parametrize("n", (33, 65, 257, 300))
def test_node_scan_reads_every_word(n):
    """node_compat's fnp[n >> 5] read past the first word, and the exact test after a commit narrowed a node: nodes
    with room for one or two pods, one pod more per selector set than its nodes hold."""
    on, off = _on_off_oracle(fc.node_solve_case(n, 400 + n), "KS_NO_NODE_ROWS")
    assert on.node_feasibility_ms > 0 and off.node_feasibility_ms == 0


@pytest.mark.parametrize("n,tw", ((1024, 32), (1056, 33), (2080, 65)))
def test_feas_masks_and_every_word(n, tw):
    """feas_masks' AND of a row of TW words: NodeClaims whose instance-type options lie in the first and the last word."""
    on, off = _on_off_oracle(fc.it_solve_case(n, 500 + tw), "KS_NO_FEASIBILITY")
    assert on.feasibility_ms > 0 and off.feasibility_ms == 0


def test_node_rows_in_consolidation_70_nodes():
    """Simulations over 70 existing nodes (three words of node bits) and pods with node selectors: rows on, off, oracle."""
    from karpenter_amd import Consolidator
    snap = synth.cluster_snapshot(n_nodes=70, pods_per_node=6, n_its=60, it_range=(8, 30), seed=11, pod_selectors=True)
    s = json.dumps(snap)
    want, _ = bridge.consolidate(s, all_sims=True)
    outs = []
    for off in (False, True):
        saved = os.environ.pop("KS_NO_NODE_ROWS", None)
        if off:
            os.environ["KS_NO_NODE_ROWS"] = "1"
        try:
            got = Consolidator(s).consolidate(all_sims=True)
        finally:
            os.environ.pop("KS_NO_NODE_ROWS", None)
            if saved is not None:
                os.environ["KS_NO_NODE_ROWS"] = saved
        got.pop("kernel_ms")
        outs.append(got)
    assert outs[0] == outs[1]
    assert outs[0] == want
