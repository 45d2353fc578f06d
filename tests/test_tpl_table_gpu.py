"""LEAN Solve: the fresh-NodeClaim table (KS_TPL_TABLE).  k_fresh_claims derives, once per handle and one wave
per (request class, template), what a NewNodeClaim that misses the memo would derive on the Solve's one-wave chain; the
Solve copies the record instead.  Every case is bit-exact parity of the canonical Results -- pod errors with their
failure flags included -- with the oracle, and the counters say which route ran:

  tplMemoHits   opens that found their key in the memo (unchanged by the table)
  tplTableHits  opens that missed it and took a record

On a build with the table (ks_problem_inspect's "tplTableBuild") every open from a template without a NodePool limit
is one or the other; on a build without it tplTableHits is 0.  The shapes are tests/tpl_table_cases.py's, each proven
to be in its cell by tests/test_tpl_table_preconditions.py."""
import json

import pytest

import tpl_table_cases as tc
from karpenter_amd import Scheduler, inspect, synth


def _assert_parity(want, got):
    g = got.canonical()
    for key in ("newNodeClaims", "existingNodes", "podErrors"):
        if want[key] != g[key] and isinstance(want[key], list):
            for i, (a, b) in enumerate(zip(want[key], g[key])):
                assert a == b, "%s[%d]: want %s\n got %s" % (key, i, json.dumps(a)[:1500], json.dumps(b)[:1500])
        assert want[key] == g[key], key
    assert want == g


def _lean(got):
    r = got.stats["route"]
    return r["family"] == "solve" and r["lean"] == 1


def _built():
    return inspect(synth.benchmark_snapshot(1, 1, 1, diverse=False))["tplTableBuild"] == 1


def _check_route(got, want, exp, table=True):
    """The counters against the oracle's NodeClaims: `table` whether this handle should hold one."""
    st = got.stats
    claims = len(want["newNodeClaims"])
    limited = exp.get("pools", {}).get("limited-pool", 0) if exp.get("limited") else 0
    print("claims %d limited %d tplMemoHits %d tplTableHits %d tplTable %d tplClasses %d tplTableMs %.4f" % (
        claims, limited, st["tplMemoHits"], st["tplTableHits"], st["tplTable"], st["tplClasses"], st["tplTableMs"]))
    assert st["nclaims"] == claims
    assert _lean(got) == exp["lean"]
    if not exp["lean"]:
        assert (st["tplTable"], st["tplTableHits"], st["tplMemoHits"]) == (0, 0, 0)
        return
    if _built() and table:
        assert st["tplTable"] == 1 and st["tplClasses"] > 0
        assert st["tplTableHits"] + st["tplMemoHits"] == claims - limited
        if exp.get("alternate"):
            assert st["tplMemoHits"] == 0
    else:
        assert (st["tplTable"], st["tplTableHits"]) == (0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", tc.NAMES)
def test_parity_and_route(name):
    exp = tc.CASES[name][1]
    want = tc.oracle(name)
    got = Scheduler(tc.snapshot_json(name)).solve()
    _assert_parity(want, got)
    _check_route(got, want, exp)
    if name == "front_no_offering":  # the record's front flag is false: a run's capacity scans the options
        assert got.stats["runCapFull"] > 0
    if "memo" in exp:  # both kinds of open occur; the memo's hits are the recorded ones (lean_step_counters.json)
        assert got.stats["tplMemoHits"] == exp["memo"]
        assert got.stats["tplTableHits"] == (exp["claims"] - exp["memo"] if _built() else 0)


@pytest.mark.gpu
def test_second_solve_of_a_handle_reads_the_same_table():
    """The table is built by the first Solve and kept: a second Solve gives the same Results and counters."""
    sch = Scheduler(tc.snapshot_json("no_fit"))
    first, again = sch.solve(), sch.solve()
    _assert_parity(tc.oracle("no_fit"), again)
    for k in ("tplTableHits", "tplMemoHits", "tplTable", "tplClasses", "algBytes"):
        assert first.stats[k] == again.stats[k], k


@pytest.mark.gpu
def test_claims_past_the_lds_resident_ones():
    """More NodeClaims than the plan keeps in LDS: the opens past KL store the record's values to HBM."""
    budget = tc.NONINLINE_BUDGET
    plan = inspect(tc.non_inline_shape())["plans"][str(budget)]
    snap = json.dumps(tc.non_inline(plan))
    import problems
    from oracle import bridge

    want = problems.canonical(bridge.solve(snap)[0])
    got = Scheduler(snap).solve(lds_budget=budget)
    _assert_parity(want, got)
    assert plan["KL"] < len(want["newNodeClaims"]) <= plan["KO"]
    assert got.stats["plan"]["KL"] == plan["KL"] and got.stats["plan"]["wide"] == 0
    _check_route(got, want, dict(lean=True))


@pytest.mark.gpu
def test_cap_exceeded(monkeypatch):
    """40 request classes and a cap of 64 bytes: no table, every NewNodeClaim derives as before."""
    monkeypatch.setenv(tc.CAP_ENV, "64")
    want = tc.oracle("all_distinct")
    got = Scheduler(tc.snapshot_json("all_distinct")).solve()
    _assert_parity(want, got)
    _check_route(got, want, tc.CASES["all_distinct"][1], table=False)
    assert got.stats["tplClasses"] == 40


@pytest.mark.gpu
def test_binary_round_trip():
    """The snapshot format holds no classes: a handle created from the binary recomputes them from the requests."""
    name = "three_classes"
    a = Scheduler(tc.snapshot_json(name))
    b = Scheduler.from_binary(a.save())
    ra, rb = a.solve(), b.solve()
    _assert_parity(tc.oracle(name), rb)
    assert ra.canonical() == rb.canonical()
    for k in ("tplTableHits", "tplMemoHits", "tplTable", "tplClasses"):
        assert ra.stats[k] == rb.stats[k], k
    _check_route(rb, tc.oracle(name), tc.CASES[name][1])
