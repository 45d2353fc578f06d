"""The host side of the launch lists (no device): the name-rank table k_launch_lists orders equal prices by, its
place in the binary snapshot, the duplicate-name refusal and the ks_solve_opts layout."""
import ctypes

import launch_cases as lc
import problems
from karpenter_amd import encode_binary, inspect, inspect_binary
from karpenter_amd.scheduler import _Opts


def _expected_ranks(snap):
    """Per template, per list position: the rank of the instance type's name in bytewise order among all types."""
    names = [it["name"] for it in snap["instanceTypes"]]
    order = sorted(range(len(names)), key=lambda i: (names[i].encode(), i))
    rank = {i: r for r, i in enumerate(order)}
    return [[rank[i] for i in snap["instanceTypesByNodePool"][t["metadata"]["name"]]] for t in snap["nodeClaimTemplates"]]


def test_name_rank_is_bytewise():
    snap = lc.all_equal_case()  # It-2 < it-1, it-10 < it-9, list order reversed
    doc = inspect(snap)
    assert doc["nameRank"] == _expected_ranks(snap)
    names = [it["name"] for it in snap["instanceTypes"]]
    (ranks,) = doc["nameRank"]
    assert sorted(ranks) == list(range(len(names)))
    assert ranks[names.index("It-2")] < ranks[names.index("it-1")] < ranks[names.index("it-10")] < ranks[names.index("it-9")]
    assert doc["launchListsRefusal"] == ""


def test_name_rank_two_templates():
    snap = lc.many_claims_case()
    doc = inspect(snap)
    assert doc["nameRank"] == _expected_ranks(snap) and [len(r) for r in doc["nameRank"]] == [32, 64]
    snap = lc.many_claims_lean_case()
    doc = inspect(snap)
    assert doc["nameRank"] == _expected_ranks(snap) and [len(r) for r in doc["nameRank"]] == [40, 70] and doc["lean"] == 1
    snap = problems.random_problem(5)
    assert inspect(snap)["nameRank"] == _expected_ranks(snap)


def test_name_rank_survives_the_binary_snapshot():
    snap = lc.tie_groups_case()
    blob = encode_binary(snap)
    assert inspect_binary(blob)["nameRank"] == inspect(snap)["nameRank"] == _expected_ranks(snap)
    assert inspect_binary(blob) == inspect(snap)


def test_duplicate_names_message():
    doc = inspect(lc.duplicate_names_case())
    assert doc["launchListsRefusal"] == ('launch lists: template 0 (nodepool "default-pool") lists two instance types named '
                                         '"dup-a"; OrderByPrice has no defined order for them')
    # the same name in two templates' lists is no duplicate within either
    snap = lc.many_claims_case()
    assert set(snap["instanceTypesByNodePool"]["pool-a"]) & set(snap["instanceTypesByNodePool"]["pool-b"])
    assert inspect(snap)["launchListsRefusal"] == ""


def test_opts_keep_their_size():
    assert ctypes.sizeof(_Opts) == 8 * ctypes.sizeof(ctypes.c_int)
    assert _Opts.launch_lists.offset == 5 * ctypes.sizeof(ctypes.c_int)
    assert _Opts.reserved.offset == 6 * ctypes.sizeof(ctypes.c_int) and _Opts.reserved.size == 2 * ctypes.sizeof(ctypes.c_int)
    o = _Opts(-1, 1, 1, 0, 0)
    assert o.launch_lists == 0  # the default call leaves the flag clear


def test_random_set_is_not_hollow():
    """The condition test_launch_gpu.py's random set rests on, from the oracle alone."""
    docs = [(lc.random_case(c), lc.oracle(("random", c), lc.random_case(c))) for c in lc.RANDOM_CASES]
    stats = [lc.oracle_claim_stats(snap, doc) for snap, doc in docs]
    assert len(docs) == 16 and all(doc["newNodeClaims"] for _, doc in docs)
    assert sum(w for w, _ in stats) >= 3 and sum(t for _, t in stats) >= 3, stats


def test_requirement_cases_differ_on_the_oracle():
    """Each restricted case orders its options differently from the unrestricted one (on the oracle, so a kernel that
    ignored the claim's record could not pass test_launch_gpu.py)."""
    lists = {k: lc.oracle(("req", k), f())["newNodeClaims"][0]["launchInstanceTypes"] for k, f in lc.REQUIREMENT_CASES.items()}
    for case, base in lc.REQUIREMENT_DIFFERS:
        assert lists[case] != lists[base] and sorted(lists[case]) == sorted(lists[base]), (case, base)
