"""Launch lists on the GPU (k_launch_lists, ks_results_nodeclaim_launch): NodeClaimTemplate.ToNodeClaim's OrderByPrice
and its cut to 100 instance types, per NewNodeClaim of a Solve.

Every case compares, for every claim of the Results: the names with the oracle's "launchInstanceTypes" (oracle/
cpu_ref.cpp: std::sort over (price, name)) and with "launchInstanceTypes" of the same Results' ks_results_json (the
host renderer, which this path does not share code with); n_options with the oracle's option count; the prices with
launch_cases.claim_prices (the minimum over the snapshot's available offerings that the claim's structured zone and
capacity-type requirements allow).  The snapshots are tests/launch_cases.py's; prices are multiples of 1/8."""
import ctypes

import pytest

import launch_cases as lc
from karpenter_amd import Scheduler, lib
from karpenter_amd.scheduler import KsError, _bind_accessors, _Opts

pytestmark = pytest.mark.gpu


def _check(key, snap, **kw):
    """Solve with launch lists and compare every claim; returns the structured Results."""
    want = lc.oracle(key, snap)
    got = Scheduler(snap).solve_structured(launch_lists=True, with_json=True, **kw)
    wc, gc, jc = want["newNodeClaims"], got.new_nodeclaims, got.doc["newNodeClaims"]
    assert len(gc) == len(wc) == len(jc) and len(wc) > 0
    for i, (w, g, j) in enumerate(zip(wc, gc, jc)):
        assert g["launch"] == w["launchInstanceTypes"], (key, i)
        assert g["launch"] == j["launchInstanceTypes"], (key, i)
        assert g["n_options"] == len(w["instanceTypeOptions"]) == len(g["instance_types"]), (key, i)
        assert len(g["launch"]) == min(g["n_options"], lc.CUT), (key, i)
        assert g["launch_prices"] == lc.claim_prices(snap, g), (key, i)
        assert g["launch_prices"] == sorted(g["launch_prices"]), (key, i)
    assert got.launch_ms > 0
    return got


@pytest.mark.parametrize("prices", ["desc", "shuffle"])
@pytest.mark.parametrize("n", lc.CUT_SIZES)
def test_cut_edges(n, prices):
    got = _check(("cut", n, prices), lc.cut_case(n, prices))
    (c,) = got.new_nodeclaims
    assert c["n_options"] == n  # nothing is filtered


def test_fits_removes_a_prefix():
    (c,) = _check("fits", lc.fits_prefix_case()).new_nodeclaims
    assert c["n_options"] == 130 and c["launch"][0] == "fake-it-149"


def test_tie_group_straddles_the_cut():
    snap = lc.tie_groups_case()
    (c,) = _check("tie-groups", snap).new_nodeclaims
    p = c["launch_prices"]
    assert c["n_options"] == 120 and p[97] < p[98] == p[99]  # positions 98 .. 104 share a price: two of seven stay
    group = sorted(it["name"] for it in snap["instanceTypes"] if it["offerings"][0]["price"] == p[99])
    assert len(group) == 7 and c["launch"][98:] == group[:2]


def test_all_equal_prices_order_by_name():
    snap = lc.all_equal_case()
    (c,) = _check("all-equal", snap).new_nodeclaims
    names = sorted(it["name"] for it in snap["instanceTypes"])  # bytewise: "It-..." before "it-...", it-10 before it-9
    assert c["launch"] == names[:lc.CUT] and names[0].startswith("It-") and names.index("it-10") < names.index("it-9")


def test_price_signs():
    (c,) = _check("signs", lc.signs_case()).new_nodeclaims
    assert c["launch"] == ["sign-" + x for x in "eiabcdhjgf"]  # -1.5 twice, the five zeros of either sign by name, 0.125, 1e300


@pytest.mark.parametrize("name", sorted(lc.REQUIREMENT_CASES))
def test_requirements_decide_the_price(name):
    snap = lc.REQUIREMENT_CASES[name]()
    (c,) = _check(("req", name), snap).new_nodeclaims
    keys = {k for k, _, _, _, _ in c["requirements"]}
    if name.startswith("neither"):  # the claim's record holds neither key
        assert lc.synth.ZONE not in keys and lc.synth.CT not in keys
    for case, base in lc.REQUIREMENT_DIFFERS:
        if case == name:  # a kernel that ignores the record (or availability) gives the unrestricted order
            other = lc.oracle(("req", base), lc.REQUIREMENT_CASES[base]())["newNodeClaims"][0]["launchInstanceTypes"]
            assert c["launch"] != other, (name, base)


def _residences(got):
    plan = got.doc["stats"]["plan"]
    return len(got.new_nodeclaims), plan["KL"]


def test_many_claims_two_templates():
    snap = lc.many_claims_case()
    got = _check("many", snap)
    n, kl = _residences(got)
    assert n >= 140 and n <= kl  # every claim LDS-resident during the Solve
    assert {c["template"] for c in got.new_nodeclaims} == {0, 1}


def test_many_claims_past_the_lds_claims():
    got = _check("many", lc.many_claims_case(), lds_budget=14000)
    n, kl = _residences(got)
    assert kl < n  # claims past KL lived in HBM


def test_many_claims_lean_uneven_lists():
    got = _check("many-lean", lc.many_claims_lean_case())
    assert got.doc["stats"]["route"]["lean"] == 1 and len(got.new_nodeclaims) >= 140
    assert {c["template"] for c in got.new_nodeclaims} == {0, 1}


def test_lean_solve():
    got = _check("lean", lc.lean_case())
    assert got.doc["stats"]["route"]["lean"] == 1 and len(got.new_nodeclaims) == 40


def test_replanned_solve():
    snap, budget = lc.replan_case()
    got = _check("replan", snap, lds_budget=budget)
    assert len(got.doc["stats"]["route"]["launches"]) == 2 and got.doc["stats"]["plan"]["wide"] == 1


def test_flag_off():
    snap = lc.many_claims_case()
    sch = Scheduler(snap)
    off = sch.solve_structured()
    assert off.launch_ms == 0 and len(off.new_nodeclaims) > 0
    assert all("launch" not in c and "launch_prices" not in c and "n_options" not in c for c in off.new_nodeclaims)
    on = sch.solve_structured(launch_lists=True, with_json=True)
    doc_off = sch.solve()
    assert on.doc["newNodeClaims"] == doc_off.doc["newNodeClaims"]
    assert on.doc["existingNodes"] == doc_off.doc["existingNodes"] and on.doc["podErrors"] == doc_off.doc["podErrors"]
    # the accessor on a Results whose Solve did not set the flag, and out of range on one that did
    l = lib()
    _bind_accessors(l)
    n, nopt = ctypes.c_int(), ctypes.c_int()
    its, prices = ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.c_double)()
    for flag, index, want in ((0, 0, -6), (1, 0, 0), (1, -1, -6), (1, len(off.new_nodeclaims), -6)):
        r = ctypes.c_void_p()
        o = _Opts(-1, 1, 1, 0, 0, flag)
        assert l.ks_solve(sch._h, ctypes.byref(o), ctypes.byref(r)) == 0
        try:
            rc = l.ks_results_nodeclaim_launch(r, index, ctypes.byref(its), ctypes.byref(prices), ctypes.byref(n),
                                               ctypes.byref(nopt))
            assert rc == want, (flag, index, rc)
            assert (l.ks_results_launch_ms(r) > 0) == bool(flag)
        finally:
            l.ks_results_free(r)


def test_duplicate_names_are_refused():
    snap = lc.duplicate_names_case()
    sch = Scheduler(snap)
    with pytest.raises(KsError) as e:
        sch.solve_structured(launch_lists=True)
    assert e.value.code == -2 and 'template 0 (nodepool "default-pool")' in str(e.value) and '"dup-a"' in str(e.value)
    want = lc.oracle("dup", snap)
    got = sch.solve()  # with the flag off the Solve works as before
    assert got.doc["newNodeClaims"][0]["instanceTypeOptions"] == want["newNodeClaims"][0]["instanceTypeOptions"]
    assert len(sch.solve_structured().new_nodeclaims) == 1


def test_random_set_is_not_hollow():
    """Over the 16 random problems the oracle alone gives at least 3 claims with more than 100 options and at least 3
    with two options at one price, and every problem has NodeClaims."""
    docs = [(lc.random_case(c), lc.oracle(("random", c), lc.random_case(c))) for c in lc.RANDOM_CASES]
    stats = [lc.oracle_claim_stats(snap, doc) for snap, doc in docs]
    assert len(docs) == 16 and all(doc["newNodeClaims"] for _, doc in docs)
    assert sum(w for w, _ in stats) >= 3 and sum(t for _, t in stats) >= 3, stats


@pytest.mark.parametrize("case", lc.RANDOM_CASES, ids=lc.RANDOM_IDS)
def test_random_problems(case):
    _check(("random", case), lc.random_case(case))
