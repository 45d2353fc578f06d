"""What tests/test_feasibility_rows_gpu.py relies on, checked without a GPU: the plain reference of
tests/feasibility_cases.py agrees with the oracle's requirement algebra on every operand pair the cases hold, each
case has the shape it is named for (through the host-only inspector), and no compared table is degenerate.

The reference (sets and ints, feasibility_cases.py) and the oracle (oracle/cpu_ref.cpp Compatible / Intersection)
are two statements of requirements.go written apart; every node bit's label part is compared with the oracle's
strict `compatible`, every per-key term of the instance-type rows with its `intersection`.  The seeds of the case
lists are chosen here: a seed whose table fails a non-degeneracy check below is replaced in feasibility_cases.py."""
import json

import pytest

import feasibility_cases as fc
from karpenter_amd import inspect, synth
from oracle import bridge

WELL_KNOWN = synth.FAKE_WELL_KNOWN + [fc.SLOT]


def _dims(snap):
    d = inspect(snap)
    d["values"] = dict(zip(d["keyNames"], d["keyValues"]))
    return d


def _states(snap):
    """[(pod index, chain position, operand list, tolerations)]; every pod of these cases has a simple chain."""
    out = []
    for pi, pod in enumerate(snap["pods"]):
        sts, whole = fc.covered_states(snap, pod)
        assert whole, "a case pod with a chain the reference does not cover"
        keys = [e["key"] for e in sts[0][0]]
        assert len(keys) == len(set(keys)), "a state names a key twice: the oracle comparison takes one operand per key"
        out += [(pi, j, e, t) for j, (e, t) in enumerate(sts)]
    return out


# --- node rows -------------------------------------------------------------------------------------------

def _both(bits, what):
    assert set(bits) == {0, 1}, "%s: only %s" % (what, sorted(set(bits)))


def _check_node_table(snap, n):
    d = _dims(snap)
    states = _states(snap)
    rows = fc.node_rows(snap)
    assert d["nodes"] == n and d["states"] == len(states) and d["FNR"] == len(rows) and d["pods"] <= 64
    assert d["FNR"] > 8
    # label part against the oracle's strict Compatible, taint part against a second spelling of Tolerates
    ops, want = [], []
    tolerant = [fc.TOL_ALL]
    for pi, j, exprs, tols in states:
        if (pi, j) not in rows:
            assert not exprs
            continue
        X = fc.reqs_of(exprs)
        for ni, node in enumerate(snap["stateNodes"]):
            lab = [{"key": k, "operator": "In", "values": [v]} for k, v in sorted(fc.node_labels(node).items())]
            ops.append({"op": "compatible", "a": lab, "b": exprs, "allowUndefinedWellKnown": False})
            want.append(fc.node_bit(node, X, tolerant))
            untolerated = [t for t in node["taints"] if not any(fc.tolerates_taint(x, t) for x in tols)]
            assert rows[(pi, j)][ni] == (want[-1] if not untolerated else 0)
    got = bridge.eval_ops(ops, WELL_KNOWN)
    bad = [(o["a"], o["b"], g, w) for o, g, w in zip(ops, got, want) if g["ok"] != bool(w)]
    assert not bad, bad[:3]
    # non-degenerate: both values in the table, in its first and last word, and in the two columns at every
    # multiple of 32 (the 64-node wave and 256-node block boundaries among them) the case crosses
    table = list(rows.values())
    _both([b for r in table for b in r], "table")
    if n > 1:
        _both([b for r in table for b in r[:32]], "first word")
        _both([b for r in table for b in r[(n - 1) // 32 * 32:]], "last word")
    for edge in range(32, n, 32):
        _both([r[edge - 1] for r in table], "node %d" % (edge - 1))
        _both([r[edge] for r in table], "node %d" % edge)
    assert any(t for node in snap["stateNodes"] for t in node["taints"]) or n < 4
    assert any(not node["taints"] for node in snap["stateNodes"]) or n < 4


@pytest.mark.parametrize("n", fc.NODE_SIZES)
def test_node_case(n):
    _check_node_table(fc.node_snapshot(n), n)


# --- instance-type rows ----------------------------------------------------------------------------------

def _check_it_table(snap, tw, named_key=None, named_values=None, gw=None, odd_rows=None):
    d = _dims(snap)
    states = _states(snap)
    rows = fc.it_rows(snap)
    lists = fc.template_lists(snap)
    assert d["TW"] == tw and d["templates"] == len(lists) and d["states"] == len(states) == len(rows) and d["pods"] <= 64
    assert (31 + max(len(x) for x in lists)) // 32 == tw
    if gw is not None:
        assert (gw == 32) == (tw <= 32)
    if named_key is not None:
        assert d["values"][named_key] == named_values
    if odd_rows is not None:
        assert (d["states"] * d["templates"]) % 2 == (1 if odd_rows else 0)
    cov = fc.covered_keys(snap)
    assert set(d["coveredKeys"]) == cov and {fc.INT, synth.IT_LABEL, "special", "size"} <= cov
    # every per-key term against the oracle's Intersection, one op per distinct operand pair
    sides = [e for _, _, e, _ in states] + [fc.template_exprs(t) for t in snap["nodeClaimTemplates"]]
    pairs = {}
    for exprs in sides:
        keys = [e["key"] for e in exprs]
        assert len(keys) == len(set(keys))
        for e in exprs:
            if e["key"] not in cov:
                continue
            for it in snap["instanceTypes"]:
                mine = fc.it_key_exprs(it, e["key"])
                if mine and mine[0]["operator"] == "In":
                    pairs.setdefault((tuple(mine[0]["values"]), id(e)), (it, e))
    assert pairs
    ops = [{"op": "intersection", "a": fc.it_key_exprs(it, e["key"])[0], "b": e} for it, e in pairs.values()]
    got = bridge.eval_ops(ops, WELL_KNOWN)
    terms = set()
    for (it, e), g in zip(pairs.values(), got):
        nonempty = g["complement"] or len(g["values"]) > 0
        term = fc.it_term(it, e["key"], fc.req_of(e))
        assert term == (1 if nonempty else 0), (it["name"], e, g)
        terms.add(term)
    assert terms == {0, 1}
    # the pinned positions occur: DoesNotExist types and irregular ones, the latter at most a tenth of any list
    irr = fc.irregular_names(snap)
    for names in lists:
        assert 10 * len([n for n in names if n in irr]) <= len(names)
    if max(len(x) for x in lists) > 5:
        assert irr
        assert any(e["operator"] == "DoesNotExist" for it in snap["instanceTypes"] for e in it["requirements"])
    # non-degenerate: both values in the table and in the first and last word of the rows; a zero (intolerant)
    # row beside a live one; in a GW = 32 case no two adjacent rows equal
    flat = [(r if r is not None else [0] * len(names)) for row in rows.values() for r, names in zip(row, lists)]
    live = [r for row in rows.values() for r in row if r is not None]
    assert len(live) < len(flat), "no intolerant row"
    _both([b for r in live for b in r], "table")
    longest = max(len(x) for x in lists)
    if longest > 1:
        _both([b for r in live for b in r[:32]], "first word")
        _both([b for r in live if len(r) == longest for b in r[(longest - 1) // 32 * 32:]], "last word")
    if tw <= 32:
        same = [i for i in range(1, len(flat)) if flat[i] == flat[i - 1] and len(flat[i]) > 1]
        assert not same, "adjacent equal rows %s" % same[:5]


@pytest.mark.parametrize("n", fc.SHAPE_SIZES)
def test_shape_case(n):
    snap = fc.shape_snapshot(n)
    _check_it_table(snap, {1: 1, 31: 1, 32: 1, 33: 2, 1024: 32, 1025: 33, 2048: 64, 2049: 65}[n],
                    named_key=synth.IT_LABEL, named_values=n, odd_rows=False)


@pytest.mark.parametrize("v,gw", sorted(fc.VALUE_CASES))
def test_value_case(v, gw):
    snap = fc.value_snapshot(v, gw)
    n = fc.VALUE_CASES[(v, gw)][0]
    _check_it_table(snap, (n + 31) // 32, named_key=fc.INT, named_values=v, gw=gw, odd_rows=False)
    # the pods' terms on the named key: In, NotIn with few and with many values, Exists, Gt, Lt
    ops = {(e["operator"], len(e.get("values", [])) > 2) for p in snap["pods"] for e in fc.pod_exprs(p) if e["key"] == fc.INT}
    assert {("In", False), ("NotIn", False), ("NotIn", True), ("Exists", False), ("Gt", False), ("Lt", False)} <= ops
    assert any(e["key"] == fc.INT and e["operator"] == "NotIn" for e in fc.template_exprs(snap["nodeClaimTemplates"][0]))
    if gw == 32:
        # rows 2k and 2k + 1 are the halves of one wave step: an In row beside a complement row on the same key,
        # and an intolerant (zero) row beside a live one
        def named_op(i):
            return [e["operator"] for e in fc.pod_exprs(snap["pods"][i]) if e["key"] == fc.INT]
        assert any(named_op(i) == ["In"] and named_op(i + 1) == ["NotIn"] for i in range(0, len(snap["pods"]) - 1, 2))
        rows = fc.it_rows(snap)
        assert any((rows[(i, 0)][0] is None) != (rows[(i + 1, 0)][0] is None) for i in range(0, len(snap["pods"]) - 1, 2))


def test_three_template_case():
    snap = fc.three_template_snapshot()
    _check_it_table(snap, 2, odd_rows=True)
    assert sorted(len(x) for x in fc.template_lists(snap)) == [7, 33, 40]
    assert fc.relaxes_tolerations(snap)
    assert any(len(fc.covered_states(snap, p)[0]) == 2 for p in snap["pods"])


# --- the end-to-end cases --------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (33, 65, 257, 300))
def test_node_solve_case(n):
    """First fit walks deep: the oracle fills existing nodes in every word of the rows and still turns pods away."""
    snap = fc.node_solve_case(n, 400 + n)
    d = _dims(snap)
    assert d["nodes"] == n and d["FNR"] > 0
    want, _ = bridge.solve(json.dumps(snap))
    order = [x["name"] for x in want["existingNodes"]]
    used = {i // 32 for i, x in enumerate(want["existingNodes"]) if x["pods"]}
    assert used == set(range((n + 31) // 32)), used
    assert len(order) == n
    assert want["newNodeClaims"] or want["podErrors"]


@pytest.mark.parametrize("n,tw", ((1024, 32), (1056, 33), (2080, 65)))
def test_it_solve_case(n, tw):
    snap = fc.it_solve_case(n, 500 + tw)
    assert _dims(snap)["TW"] == tw
    want, _ = bridge.solve(json.dumps(snap))
    assert len(want["newNodeClaims"]) > 1
    opts = {o for c in want["newNodeClaims"] for o in c["instanceTypeOptions"]}
    words = {int(o.split("-")[1]) // 32 for o in opts}
    assert 0 in words and tw - 1 in words
