"""The queue-preparation kernels of csrc/ks_queue.hip read back word for word and compared, by exact equality, with
the plain references of tests/queue_cases.py (checked on the CPU by tests/test_queue_reference.py).  None of these
tests runs a Solve's k_solve except the consolidation pass of the per-simulation queues.

  order         k_qkeys / k_iota / queue_sort (ks_problem_queue_readback): P = 1 .. 70001, every subset of the four
                key components varying alone (the skipped passes, both buffer parities), the span edges of skBits,
                components that run against each other (stable passes), a large skMin, the tie path;
  run lengths   k_sim_run_breaks / k_sim_run_len, strict: runs ending on the 64-entry ballot words and the 256-thread
                blocks, all-zero break words, each break criterion alone;
  simulations   k_rank / k_sim_keys / sim_queue_sort and the non-strict run lengths after one consolidation pass
                (ks_cons_queue_readback);
  records       k_rec_headers through its handle-free driver (ks_rec_headers_run): every check code, the `valid`
                mask at 31 / 32 / 33 options, the minimum across blocks, the publish and reset across passes, the
                staged header copy at a ragged last block.

Each case asserts the path it exists for (queue_cases' preconditions) before it compares."""
import json

import pytest

import queue_cases as qc
from karpenter_amd import Consolidator, Scheduler, queue_inputs, rec_headers_meta, rec_headers_run

pytestmark = pytest.mark.gpu


def _readback(snap):
    s = json.dumps(snap)
    inp = queue_inputs(s)
    sch = Scheduler(s)
    try:
        order, run_len, device = sch.queue_readback()
    finally:
        sch.close()
    return inp, order, run_len, device


def _pod_text(inp, p):
    if not 0 <= p < inp["P"]:
        return "pod %d (out of range)" % p
    return "pod %d uid %s key %s req %s s0 %s" % (p, inp["uids"][p], inp["sortKeys"][p], inp["podReq"][p], inp["podS0"][p])


def _compare(what, got, want, inp, pods):
    """Exact equality; on the first difference the entry, the pod there and both values."""
    assert len(got) == len(want), "%s: %d entries, want %d" % (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            pytest.fail("%s differs first at entry %d: got %s, want %s; the entry's pod: %s%s" % (
                what, i, hex(g & 0xFFFFFFFF) if g == qc.FILL else g, w, _pod_text(inp, pods[i]),
                "" if what != "order" else "; got " + _pod_text(inp, g)))


def check_order(snap, pre, device_sort=True):
    inp, order, run_len, device = _readback(snap)
    pre(inp)
    assert device == device_sort, "the order came from %s" % ("the device sort" if device else "the host")
    want = qc.expected_order(inp)
    _compare("order", order, want, inp, want)
    assert (run_len is not None) == bool(inp["lean"])
    return inp, order, run_len


@pytest.mark.parametrize("n", qc.ORDER_SIZES)
def test_order_sizes(n):
    """The largest case is the one above 65536 entries: its host encode takes a few seconds on a CPU."""
    snap, pre = qc.size_case(n)
    check_order(snap, pre)


@pytest.mark.parametrize("subset", qc.SUBSETS, ids=["".join(map(str, s)) for s in qc.SUBSETS])
def test_order_component_subsets(subset):
    snap, pre = qc.subset_case(subset)
    check_order(snap, pre)


@pytest.mark.parametrize("comp", qc.SPAN_COMPONENTS)
@pytest.mark.parametrize("span", qc.SPANS)
def test_order_span_edges(comp, span):
    snap, pre = qc.span_case(comp, span)
    check_order(snap, pre)


def test_order_memory_span():
    check_order(*qc.memory_span_case())


def test_order_stable_passes():
    check_order(*qc.stable_case())


def test_order_large_minimum_one_second_span():
    inp, _, _ = check_order(*qc.late_second_case())
    assert inp["skMin"][0] < 0 and inp["skMin"][2] > 2 ** 30


def test_tie_path_reads_the_host_order():
    inp, order, _ = check_order(*qc.tie_case(False), device_sort=False)
    assert order == inp["hostOrder"]


def test_shared_uids_with_distinct_stamps_sort_on_the_device():
    check_order(*qc.tie_case(True))


# --- strict run lengths -------------------------------------------------------------------------------------------------

def check_run_lengths(snap):
    inp, order, run_len, device = _readback(snap)
    assert inp["lean"] == 1 and device and run_len is not None
    want_order = qc.expected_order(inp)
    _compare("order", order, want_order, inp, want_order)
    assert qc.FILL not in run_len, "entry %d was never stored" % run_len.index(qc.FILL)
    want = qc.run_lengths(want_order, inp, True)
    _compare("run_len", run_len, want, inp, want_order)
    return inp, want_order, run_len


@pytest.mark.parametrize("name", sorted(qc.RUN_LISTS))
def test_strict_run_lengths(name):
    runs = qc.RUN_LISTS[name]
    _, _, run_len = check_run_lengths(qc.runs_case(runs))
    assert run_len == qc.run_lengths_of(runs)


@pytest.mark.parametrize("kind", ["resource", "tolerations", "templates", "flags"])
def test_strict_run_length_criteria(kind):
    """Neighbours differ in one criterion alone (tests/test_queue_reference.py checks which); every run has length 1.
    "flags" differs only in pod_s0 word 3, where the non-strict comparison would not break.  Word 2 is computed from
    words 0..1, so "templates" differs in both and no case can show word 2 alone."""
    inp, order, run_len = check_run_lengths(qc.criterion_case(kind))
    assert run_len == [1] * inp["P"]
    if kind == "flags":
        assert qc.run_lengths(order, inp, False) == qc.run_lengths_of([inp["P"]])


# --- per-simulation queues ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cons_readback():
    snap = qc.stamped_cluster()
    c = Consolidator(json.dumps(snap))
    try:
        c.run(keep=True)
        return snap, c.queue_readback()
    finally:
        c.close()


def test_simulation_queues(cons_readback):
    snap, rb = cons_readback
    n, sims = rb["n"], rb["sims"]
    esim = rb["lentrySim"]
    assert esim == sorted(esim) and esim[0] == 0 and esim[-1] == sims - 1, "entries are grouped by simulation"
    # the pods carry their stamps
    created = {p["metadata"]["uid"]: qc.seconds(p["metadata"]["creationTimestamp"])
               for node in snap["stateNodes"] for p in node["pods"]}
    assert len(set(created.values())) == 3
    for p in range(rb["P"]):
        assert rb["sortKeys"][p][2] == created[rb["uids"][p]]
    assert rb["skBits"][2] > 0 and rb["hostOrder"] is None
    want_order = qc.order_reference(rb["sortKeys"])
    want_rank = qc.inverse(want_order)
    _compare("rank", rb["rank"], want_rank, rb, list(range(rb["P"])))
    want_map = qc.sim_queues(rb["lentries"], esim, want_rank)
    _compare("lpodmap", rb["lpodmap"], want_map, rb, want_map)
    want_len = qc.run_lengths(want_map, rb, False, entry_sim=esim)
    assert qc.FILL not in rb["lrunlen"]
    _compare("lrunlen", rb["lrunlen"], want_len, rb, want_map)
    # the shapes this cluster exists for
    sizes = [esim.count(s) for s in range(sims)]
    assert n > 256 and 1 in sizes, "entries must cross a block and one simulation must hold a single entry"
    border = [i for i in range(1, n) if esim[i] != esim[i - 1]
              and not qc.pods_differ(rb, want_map[i], want_map[i - 1], False)]
    assert border, "two adjacent simulations must meet in identical pods"
    assert all(want_len[i - 1] == 1 for i in border)
    assert any(i % 64 + want_len[i] > 64 and want_len[i] > 1 for i in range(n)), "a run must cross a 64-entry word"
    assert (1 << rb["rbits"]) >= rb["P"] and (1 << rb["sbits"]) >= sims


# --- k_rec_headers --------------------------------------------------------------------------------------------------------

META = None


def _meta():
    global META
    if META is None:
        META = rec_headers_meta()
    return META


def check_passes(passes, tw, tpl_beg):
    """Every pass's headers equal the records' first RF_HDR words and its status words equal the reference's."""
    meta = _meta()
    h = meta["RF_HDR"]
    out = rec_headers_run(passes, tw, tpl_beg)
    for k, (recs, (hdr, status, verdicts)) in enumerate(zip(passes, out)):
        want_hdr = [w for rec in recs for w in rec[:h]]
        assert len(hdr) == len(want_hdr)
        for i, (g, w) in enumerate(zip(hdr, want_hdr)):
            if g != w:
                pytest.fail("pass %d: header word %d of record %d: got %s, want %s" % (k, i % h, i // h, hex(g & 0xFFFFFFFF), hex(w & 0xFFFFFFFF)))
        want = qc.status_words(recs, tw, tpl_beg, meta)
        for j in range(2):
            if status[j] != want[j]:
                pytest.fail("pass %d: status word %d: got record %d code %d (%s), want record %d code %d (%s)" % (
                    k, j, status[j] >> 32, status[j] & 0xFFFFFFFF, hex(status[j]), want[j] >> 32, want[j] & 0xFFFFFFFF,
                    hex(want[j])))
        for rec, msg in zip(recs, verdicts):  # the host twin agrees on pass / fail
            failing = qc.record_code(rec, tw, tpl_beg, meta) != 0 or rec[meta["RF"]["ERROR"]] != meta["KE"]["OK"]
            assert (msg != "") == failing
    return out


@pytest.mark.parametrize("tw,nits", qc.REC_SHAPES)
@pytest.mark.parametrize("ns", qc.REC_NS)
def test_rec_headers_good_batches(ns, tw, nits):
    tpl_beg = qc.tpl_beg_for(nits)
    (_, status, _), = check_passes([qc.record_batch(_meta(), tw, tpl_beg, ns)], tw, tpl_beg)
    assert status == [qc.ALL_ONES, qc.ALL_ONES]


@pytest.mark.parametrize("tw,nits", qc.REC_SHAPES)
def test_rec_headers_every_code(tw, nits):
    """One failing record per check code among 513 valid ones, each in a pass of its own, at the last position of the
    ragged last block; and the records that are valid at the edges."""
    meta = _meta()
    tpl_beg = qc.tpl_beg_for(nits)
    ns = 513
    bad = qc.failing_records(meta, tw, tpl_beg)
    passes, codes = [], sorted(bad)
    for code in codes:
        passes.append(qc.record_batch(meta, tw, tpl_beg, ns, {ns - 1: bad[code]}))
    out = check_passes(passes, tw, tpl_beg)
    for code, (_, status, _) in zip(codes, out):
        assert status[0] == ((ns - 1) << 32) | code and status[1] == qc.ALL_ONES
    nit = nits[0]
    edge = {
        3: qc.make_record(meta, tw, 3000, "REPLACE", 1, tpl=0, options=range(nit)),  # every option of the list
        260: qc.make_record(meta, tw, 3001, "NOOP", 0, raw_words=[-1, 0x5A5A5A5A, 7] * tw),  # no claims: words unread
        300: qc.make_record(meta, tw, 3002, "NOOP", 2, hostincr=2, tpl=1, options=[0]),
        511: qc.make_record(meta, tw, 3003, "DELETE", 0, raw_words=[-1] * (3 * tw)),
    }
    (_, status, _), = check_passes([qc.record_batch(meta, tw, tpl_beg, ns, edge)], tw, tpl_beg)
    assert status == [qc.ALL_ONES, qc.ALL_ONES]
    for tpl in (-1, len(nits)):
        rec = qc.make_record(meta, tw, 3004, "REPLACE", 1, tpl=tpl, options=[0])
        (_, status, _), = check_passes([qc.record_batch(meta, tw, tpl_beg, 257, {256: rec})], tw, tpl_beg)
        assert status[0] == (256 << 32) | 5


def test_rec_headers_valid_mask_edges():
    """nIT = 31 / 32 / 33: option nIT - 1 is valid, option nIT is beyond the list (where the words hold it)."""
    meta = _meta()
    for tw, nit in ((1, 31), (1, 32), (2, 32), (2, 33), (2, 31), (3, 64), (3, 65)):
        tpl_beg = qc.tpl_beg_for([nit, 1])
        good = qc.make_record(meta, tw, 1, "REPLACE", 1, tpl=0, options=range(nit))
        recs = [good]
        if nit < 32 * tw:
            recs.append(qc.make_record(meta, tw, 2, "REPLACE", 1, tpl=0, options=[nit]))
        (_, status, _), = check_passes([recs], tw, tpl_beg)
        assert status[0] == (qc.ALL_ONES if len(recs) == 1 else (1 << 32) | 6), (tw, nit, hex(status[0]))


def test_rec_headers_minimum_across_blocks():
    """Two failing records in different blocks: the lower simulation wins whichever block finishes first; a kernel
    error on a record that also fails a check fills both words independently."""
    meta = _meta()
    tw, tpl_beg = 2, qc.tpl_beg_for([33, 32])
    bad = qc.failing_records(meta, tw, tpl_beg)
    a = check_passes([qc.record_batch(meta, tw, tpl_beg, 513, {5: bad[8], 512: bad[3]}),
                      qc.record_batch(meta, tw, tpl_beg, 513, {5: bad[3], 512: bad[8]}),
                      qc.record_batch(meta, tw, tpl_beg, 513, {300: bad[9], 511: bad[2]})], tw, tpl_beg)
    assert [s[0] for _, s, _ in a] == [(5 << 32) | 8, (5 << 32) | 3, (300 << 32) | 9]
    both = qc.make_record(meta, tw, 4000, "DELETE", 1, tpl=0, options=[0], error="ITER_CAP")
    err = qc.make_record(meta, tw, 4001, "NOOP", 0, error="CLAIM_CAP")
    (_, status, _), = check_passes([qc.record_batch(meta, tw, tpl_beg, 513, {400: both, 100: err, 2: bad[4]})], tw, tpl_beg)
    assert status == [(2 << 32) | 4, (100 << 32) | meta["KE"]["CLAIM_CAP"]]


def test_rec_headers_status_persists_between_passes():
    """The status words and the block counter are set once: a failing pass, an all-good pass (must publish all-ones in
    both words), the failing pass again (must equal the first), with the grid changing from 3 blocks to 1 and back."""
    meta = _meta()
    tw, tpl_beg = 1, qc.tpl_beg_for([32, 31])
    bad = qc.failing_records(meta, tw, tpl_beg)
    err = qc.make_record(meta, tw, 5000, "NOOP", 0, error="STACK")
    failing = qc.record_batch(meta, tw, tpl_beg, 513, {7: bad[9], 300: err, 512: bad[1]})
    one_bad = [bad[4]]
    out = check_passes([failing, qc.record_batch(meta, tw, tpl_beg, 1), failing, one_bad,
                        qc.record_batch(meta, tw, tpl_beg, 513), failing], tw, tpl_beg)
    status = [s for _, s, _ in out]
    assert status[0] == [(7 << 32) | 9, (300 << 32) | meta["KE"]["STACK"]]
    assert status[1] == [qc.ALL_ONES, qc.ALL_ONES]
    assert status[2] == status[0] and status[5] == status[0]
    assert status[3] == [4, qc.ALL_ONES] and status[4] == [qc.ALL_ONES, qc.ALL_ONES]
