"""What tests/test_queue_readback_gpu.py relies on, checked without a GPU: the encoded sort keys against values the
test computes itself (creation times through calendar.timegm, never through the library's or the oracle's own date
code), skMin / skBits at the span edges, the oracle's queue order with timestamps (a problem whose scheduled set is a
prefix of the queue, so a mistake shared by the library's and the oracle's date parsing shows), the plain references of
tests/queue_cases.py against closed forms, every case's precondition, and the Python record check against the host's
check_record."""
import json

import pytest

import queue_cases as qc
from karpenter_amd import queue_inputs, rec_headers_meta, rec_headers_verdicts
from oracle import bridge

DATES = [
    "2024-02-29T12:34:56Z",  # 29 Feb of a leap year
    "2023-03-01T00:00:00Z",  # 1 Mar of a non-leap year
    "2024-03-01T00:00:00Z",
    "2000-02-29T23:59:59Z",  # a leap century
    "2100-03-01T00:00:00Z",  # a non-leap century, after 2038
    "2025-12-31T23:59:59Z", "2026-01-01T00:00:00Z",  # adjacent years
    "1999-12-31T23:59:59Z", "2000-01-01T00:00:00Z",
    "2038-01-19T03:14:08Z",  # 2^31
    "2262-04-11T23:47:16Z",
    "1970-01-01T00:00:01Z",
]


def test_date_helper_is_calendar_timegm():
    assert qc.seconds("1970-01-01T00:00:01Z") == 1
    assert qc.seconds("2024-02-29T00:00:00Z") + 86400 == qc.seconds("2024-03-01T00:00:00Z")
    assert qc.seconds("2023-02-28T00:00:00Z") + 86400 == qc.seconds("2023-03-01T00:00:00Z")
    assert qc.seconds("2100-02-28T00:00:00Z") + 86400 == qc.seconds("2100-03-01T00:00:00Z")
    assert qc.seconds("2025-12-31T23:59:59Z") + 1 == qc.seconds("2026-01-01T00:00:00Z")
    assert qc.seconds("2038-01-19T03:14:08Z") == 2 ** 31
    for d in DATES:
        assert qc.stamp(qc.seconds(d)) == d


def test_sort_keys_against_the_snapshot():
    """Every component from literal values: -cpu and -memory in the exported device units, the creation second (0
    without a stamp: Go's zero Time sorts first), the uid's rank among the sorted uids."""
    cpus = [100, 250, 1, 1500, 64000, 999]
    mems = ["64Mi", "1Gi", "3Mi", "2048Gi", "512Mi"]
    stamps = DATES + [None, None]
    uids = ["b", "a", "Z", "zz", "z", "~", "0", "10", "9", "u1", "u02", "A", "-", "_", "aa", "ab"]
    n = len(uids)
    pods = [qc.qpod(uids[i], cpus[i % len(cpus)], mem=mems[i % len(mems)], created=stamps[i % len(stamps)])
            for i in range(n)]
    inp = queue_inputs(qc.snapshot(pods))
    assert inp["P"] == n and inp["uids"] == uids and inp["hostOrder"] is None and not inp["dupUids"]
    cpu_col, mem_col = inp["resources"].index("cpu"), inp["resources"].index("memory")
    rank = {u: r for r, u in enumerate(sorted(uids, key=lambda u: u.encode()))}
    unit = {"Mi": 1 << 20, "Gi": 1 << 30}
    for i in range(n):
        key = inp["sortKeys"][i]
        cpu_nano = cpus[i % len(cpus)] * 10 ** 6
        m = mems[i % len(mems)]
        mem_nano = int(m[:-2]) * unit[m[-2:]] * 10 ** 9
        assert -key[0] * 10 ** inp["resShift"][cpu_col] == cpu_nano, (i, key)
        assert -key[1] * 10 ** inp["resShift"][mem_col] == mem_nano, (i, key)
        s = stamps[i % len(stamps)]
        assert key[2] == (0 if s is None else qc.seconds(s)), (i, s, key)
        assert key[3] == rank[uids[i]], (i, key)
        assert inp["podReq"][i][cpu_col] == -key[0] and inp["podReq"][i][mem_col] == -key[1]
    assert min(k[2] for k in inp["sortKeys"]) == 0 < qc.seconds("1970-01-01T00:00:01Z")  # a missing stamp sorts first
    for c in range(4):
        col = [k[c] for k in inp["sortKeys"]]
        assert inp["skMin"][c] == min(col) and inp["skBits"][c] == (max(col) - min(col)).bit_length()


def test_missing_stamp_sorts_first():
    pods = [qc.qpod("a", 100, 64, created="1970-01-01T00:00:01Z"), qc.qpod("b", 100, 64),
            qc.qpod("c", 100, 64, created="2100-03-01T00:00:00Z"), qc.qpod("d", 100, 64)]
    inp = queue_inputs(qc.snapshot(pods))
    assert [inp["uids"][p] for p in qc.order_reference(inp["sortKeys"])] == ["b", "d", "a", "c"]


# --- the oracle sees the same order, timestamps included --------------------------------------------------------------

def _probe_pods(kind):
    n = 9
    if kind == "stamps-oppose-uids":
        dates = ["2024-02-29T00:00:00Z", "2024-03-01T00:00:00Z", "2025-12-31T23:59:59Z", "2026-01-01T00:00:00Z",
                 "2038-01-19T03:14:08Z", "2100-02-28T23:59:59Z", "2100-03-01T00:00:00Z", "2101-01-01T00:00:00Z", None]
        # uid order a..i, stamp order its reverse; the pod without a stamp has the largest uid and comes first
        return [(dates[n - 2 - i] if i < n - 1 else None, "abcdefghi"[i]) for i in range(n)]
    return [("2026-03-01T12:00:00Z", "ihgfedcba"[i]) for i in range(n)]  # equal stamps: the uid decides


def _probe_reference(pairs):
    """The queue order from the literal values alone: (creation second, uid)."""
    return [u for _, u in sorted(pairs, key=lambda tu: (0 if tu[0] is None else qc.seconds(tu[0]), tu[1].encode()))]


@pytest.mark.parametrize("kind", ["stamps-oppose-uids", "equal-stamps"])
def test_oracle_schedules_the_queue_prefix(kind):
    pairs = _probe_pods(kind)
    want = _probe_reference(pairs)
    if kind == "stamps-oppose-uids":
        assert want == ["i"] + list("hgfedcba"), "the case must oppose uid order"
    seen = []
    for k in (1, 4, len(pairs) - 1):
        snap = qc.prefix_probe(pairs, k)
        inp = queue_inputs(snap)
        assert [inp["uids"][p] for p in qc.order_reference(inp["sortKeys"])] == want
        res, _ = bridge.solve(json.dumps(snap))
        assert len(res["newNodeClaims"]) == 1, "the NodePool limit must allow one node"
        got = qc.scheduled_uids(res, snap)
        assert got == set(want[:k]), "k = %d: the oracle scheduled %s, the queue's first k are %s" % (k, sorted(got), want[:k])
        assert len(res["podErrors"]) == len(pairs) - k
        seen.append(got)
    assert seen[0] < seen[1] < seen[2]  # nested prefixes


# --- skBits edges -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("comp", qc.SPAN_COMPONENTS)
@pytest.mark.parametrize("span", qc.SPANS)
def test_sk_bits_at_span_edges(comp, span):
    snap, pre = qc.span_case(comp, span)
    inp = queue_inputs(snap)
    pre(inp)
    col = [k[comp] for k in inp["sortKeys"]]
    assert inp["skBits"][comp] == span.bit_length() and inp["skMin"][comp] == min(col) and max(col) - min(col) == span
    if comp == 2:
        assert min(col) == qc.T2026
    else:
        assert sorted(-x for x in col) == [1, 1 + span // 2, 1 + span]  # "Nm" at a 1m unit


def test_sk_bits_memory_span():
    snap, pre = qc.memory_span_case()
    inp = queue_inputs(snap)
    pre(inp)
    assert max(k[1] for k in inp["sortKeys"]) - inp["skMin"][1] >= 2 ** 40


# --- every GPU case takes the path it is named for ----------------------------------------------------------------------

@pytest.mark.parametrize("n", [n for n in qc.ORDER_SIZES if n <= 4097])
def test_size_cases(n):
    snap, pre = qc.size_case(n)
    inp = queue_inputs(snap)
    pre(inp)
    assert qc.is_sorted_permutation(qc.expected_order(inp), inp["sortKeys"])


@pytest.mark.parametrize("subset", qc.SUBSETS, ids=["".join(map(str, s)) for s in qc.SUBSETS])
def test_subset_cases(subset):
    snap, pre = qc.subset_case(subset)
    inp = queue_inputs(snap)
    pre(inp)
    order = qc.order_reference(inp["sortKeys"])  # strict keys
    assert order != list(range(inp["P"])), "the input order must not already be the queue order"


def test_other_order_cases():
    for snap, pre in (qc.stable_case(), qc.late_second_case(), qc.tie_case(True), qc.tie_case(False)):
        inp = queue_inputs(snap)
        pre(inp)
        assert qc.is_sorted_permutation(qc.expected_order(inp), inp["sortKeys"])
    # the stable case: each lower component runs against the one above it
    inp = queue_inputs(qc.stable_case()[0])
    order = qc.order_reference(inp["sortKeys"])
    assert order != sorted(order) and order != sorted(order, reverse=True)


# --- run lengths --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(qc.RUN_LISTS))
def test_run_length_reference_against_the_run_list(name):
    runs = qc.RUN_LISTS[name]
    inp = queue_inputs(qc.runs_case(runs))
    assert inp["lean"] == 1 and inp["hostOrder"] is None
    order = qc.order_reference(inp["sortKeys"])
    assert order == list(range(sum(runs))), "the runs must follow each other in the queue"
    assert qc.run_lengths(order, inp, True) == qc.run_lengths_of(runs)
    assert qc.run_lengths(order, inp, False) == qc.run_lengths_of(runs)


def test_run_lists_hit_the_word_and_block_edges():
    ends = set()  # the last entry of every run
    at = 0
    for length in qc.RUN_LISTS["ends-at-63-64-255-256"]:
        at += length
        ends.add(at - 1)
    assert {63, 64, 255, 256} <= ends
    first, long, _ = qc.RUN_LISTS["three-zero-words"]
    # the break words of entries 64 .. 255 (words 1, 2, 3) hold no run start
    assert first < 64 and first + long >= 256 and long >= 200
    assert qc.RUN_LISTS["run-of-64-from-0"][0] == 64 and qc.RUN_LISTS["break-at-last-entry"][-1] == 1
    assert [sum(qc.RUN_LISTS["one-run-%d" % n]) for n in (64, 65, 128, 256, 257, 320)] == [64, 65, 128, 256, 257, 64 * 5]


@pytest.mark.parametrize("kind", ["resource", "tolerations", "templates", "flags"])
def test_criterion_cases_differ_in_one_criterion(kind):
    """Neighbours differ in the named criterion alone, and the strict comparison is what "flags" tests: without
    pod_s0 words 2..3 nothing breaks there.  The template-toleration set (word 2) is computed from the toleration
    words (0..1) and the templates' taints, so no snapshot makes it differ alone: "templates" differs in both, and
    the non-strict reference breaks there too."""
    snap = qc.criterion_case(kind)
    inp = queue_inputs(snap)
    n = inp["P"]
    assert inp["lean"] == 1 and inp["hostOrder"] is None
    order = qc.order_reference(inp["sortKeys"])
    assert order == list(range(n))
    for i in range(1, n):
        p, q = order[i], order[i - 1]
        req_diff = [c for c in range(inp["R"]) if inp["podReq"][p][c] != inp["podReq"][q][c]]
        s0_diff = [w for w in range(4) if inp["podS0"][p][w] != inp["podS0"][q][w]]
        assert inp["podFlags"][p] == inp["podFlags"][q]
        if kind == "resource":
            assert inp["resources"][-1] == qc.LAST_RESOURCE and req_diff == [inp["R"] - 1] and s0_diff == []
        else:
            assert req_diff == [] and s0_diff == {"tolerations": [0], "templates": [0, 2], "flags": [3]}[kind]
    assert qc.run_lengths(order, inp, True) == [1] * n
    assert qc.run_lengths(order, inp, False) == (qc.run_lengths_of([n]) if kind == "flags" else [1] * n)


def test_run_length_reference_with_simulations():
    """A change of simulation starts a run between identical pods."""
    inp = queue_inputs(qc.runs_case([6]))
    assert qc.run_lengths([0, 1, 2, 3, 4, 5], inp, False, entry_sim=[0, 0, 1, 1, 1, 2]) == [2, 1, 3, 2, 1, 1]
    assert qc.sim_queues([5, 4, 3, 2, 1, 0], [0, 0, 1, 1, 1, 2], qc.inverse([0, 1, 2, 3, 4, 5])) == [4, 5, 1, 2, 3, 0]


# --- the Python record check against the host's ---------------------------------------------------------------------------

def crafted_records(meta, tw, tpl_beg):
    """[(name, record, both_fail_only)]: every record the GPU test of k_rec_headers crafts, at this shape."""
    out = [("good-%d" % t, qc.good_record(meta, tw, tpl_beg, t), False) for t in range(10)]
    for code, rec in sorted(qc.failing_records(meta, tw, tpl_beg).items()):
        out.append(("code-%d" % code, rec, False))
    nit = tpl_beg[1] - tpl_beg[0]
    full = list(range(nit))
    out.append(("all-options", qc.make_record(meta, tw, 2000, "REPLACE", 1, tpl=0, options=full), False))
    out.append(("no-claims-garbage-words", qc.make_record(meta, tw, 2001, "NOOP", 0, raw_words=[-1, 0x5A5A5A5A, 7] * tw), False))
    out.append(("noop-two-claims", qc.make_record(meta, tw, 2002, "NOOP", 2, hostincr=2, tpl=1,
                                                  options=[0]), False))
    out.append(("tpl-minus-1", qc.make_record(meta, tw, 2003, "REPLACE", 1, tpl=-1, options=[0]), False))
    out.append(("tpl-ntpl", qc.make_record(meta, tw, 2004, "REPLACE", 1, tpl=len(tpl_beg) - 1, options=[0]), False))
    out.append(("no-options", qc.make_record(meta, tw, 2005, "REPLACE", 1, tpl=0, options=[]), False))
    if nit > 1:
        out.append(("same-not-in-price", qc.make_record(meta, tw, 2006, "REPLACE", 1, tpl=0, options=full, price=[0],
                                                        same=[0, nit - 1]), False))
    # several rules at once: host and reference may name different ones
    out.append(("error-and-check", qc.make_record(meta, tw, 2007, "DELETE", 1, tpl=0, options=[0], error="ITER_CAP"), True))
    if nit < 32 * tw and nit > 1:
        out.append(("beyond-and-subset", qc.make_record(meta, tw, 2008, "REPLACE", 1, tpl=0, options=[0, nit],
                                                        price=[nit - 1]), True))
    return out


@pytest.mark.parametrize("tw,nits", qc.REC_SHAPES)
def test_record_reference_against_the_host_check(tw, nits):
    meta = rec_headers_meta()
    tpl_beg = qc.tpl_beg_for(nits)
    cases = crafted_records(meta, tw, tpl_beg)
    verdicts = rec_headers_verdicts([rec for _, rec, _ in cases], tw, tpl_beg)
    codes = set()
    for (name, rec, both_fail), msg in zip(cases, verdicts):
        code = qc.record_code(rec, tw, tpl_beg, meta)
        codes.add(code)
        if name.startswith("good") or name in ("all-options", "no-claims-garbage-words", "noop-two-claims"):
            assert code == 0 and msg == "", (name, code, msg)
        elif both_fail:
            assert msg != "" and code != 0, (name, code, msg)
        else:
            assert code != 0 and any(msg.endswith("record check: " + m) for m in qc.CODE_MESSAGES[code]), (name, code, msg)
        if name.startswith("code-"):
            assert code == int(name[5:]), (name, code)
    want = set(range(10)) - ({6} if nits[0] == 32 * tw else set()) - ({7} if nits[0] == 1 else set())
    assert want <= codes


def test_record_constants_are_distinct():
    meta = rec_headers_meta()
    assert len(set(meta["RF"].values())) == len(meta["RF"]) and max(meta["RF"].values()) < meta["RF_HDR"]
    assert meta["KE"]["OK"] == 0 and sorted(meta["CA"].values()) == list(range(len(meta["CA"])))
