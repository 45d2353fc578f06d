"""NewQueue's order in one sort pass (KS_QUEUE_PACKED, csrc/ks_queue.hip): when the four key components' bit widths
sum to 64 or less the device sorts one packed key per pod; wider keys take the chained per-component passes.  The
order is read back (ks_problem_queue_readback) and compared by exact equality with the host order computed from
ks_problem_queue_inputs' sort keys (tests/queue_cases.py: expected_order).

  widths   key widths summing to exactly 64 (the widest packed key: component 0 ends on bit 63) and to 65 (the
           chained path), the first with each component at its full width at the top and bottom of its span;
  ties     pods tying on the first one, two and three components, so the order rests on the lower fields of the
           packed key, at P in {1, 2, 255, 256, 257, 1025} (k_qkeys_packed's block edge, one pod: no key bits).

Every case asserts the widths it exists for before it compares.  Which path a width of 64 or less takes is the
build's (ks_problem_inspect's "queuePacked"; the shipped build keeps the chain): scripts/variant_check.sh
runs this file on the -DKS_QUEUE_PACKED=1 build, and the expected order is the same for both."""
import json

import pytest

import queue_cases as qc
from karpenter_amd import Scheduler, queue_inputs

pytestmark = pytest.mark.gpu


def check(snap, pre):
    s = json.dumps(snap)
    inp = queue_inputs(s)
    pre(inp)
    sch = Scheduler(s)
    try:
        order, _, device = sch.queue_readback()
    finally:
        sch.close()
    assert device, "the order must come from the device sort"
    want = qc.expected_order(inp)
    assert len(order) == len(want)
    for i, (g, w) in enumerate(zip(order, want)):
        assert g == w, "order differs first at entry %d: got pod %d key %s, want pod %d key %s (skBits %s)" % (
            i, g, inp["sortKeys"][g] if 0 <= g < inp["P"] else None, w, inp["sortKeys"][w], inp["skBits"])
    return inp


def width_case(total):
    """257 pods (9 uid bits), cpu over 10 bits, the stamp over 14, memory over the rest of `total`: every component's
    span is exactly 2^bits - 1, and the pods at both ends of each span are present; the other pods scatter over them
    with the uid order opposing the index."""
    n = 257
    bits = [10, total - 9 - 10 - 14, 14, 9]
    span = [(1 << b) - 1 for b in bits]
    pods = []
    for i in range(n):
        c = (i * 389) % (span[0] + 1) if 1 < i else span[0] * i
        m = (i * 2654435761) % (span[1] + 1) if 3 < i or i < 2 else span[1] * (i - 2)
        t = (i * 7919) % (span[2] + 1) if 5 < i or i < 4 else span[2] * (i - 4)
        pods.append(qc.qpod(qc.uid(n - 1 - i), 1 + c, mem="%d" % (1 + m), created=qc.T2026 + t))

    def pre(inp):
        assert inp["hostOrder"] is None and inp["P"] == n
        assert inp["skBits"] == bits and sum(inp["skBits"]) == total, inp["skBits"]
    return qc.snapshot(pods), pre


def test_key_width_of_exactly_64_bits():
    inp = check(*width_case(64))
    top = max(inp["sortKeys"], key=lambda k: k[0])  # component 0 reaches bit 63 of the packed key
    assert top[0] - inp["skMin"][0] == (1 << inp["skBits"][0]) - 1


def test_key_width_of_65_bits_takes_the_chained_passes():
    check(*width_case(65))


def tie_case(n, depth):
    """Pods in pairs that share the first `depth` components; the next component (or the uid) tells a pair apart, and
    the uid order opposes the index.  One pod: no component varies."""
    pods = []
    for i in range(n):
        shared = (i // 2) % 2
        own = i % 5
        v = [shared if c < depth else (own if c == depth else 0) for c in range(3)]
        pods.append(qc.qpod(qc.uid(n - 1 - i), 100 + v[0], 64 + v[1], created=qc.T2026 + v[2]))

    def pre(inp):
        keys = [tuple(k) for k in inp["sortKeys"]]
        assert inp["P"] == n and inp["hostOrder"] is None and sum(inp["skBits"]) <= 64
        if n > 1:
            assert any(a[:depth] == b[:depth] and a[depth] != b[depth] for a in keys[:4] for b in keys[:4] if a != b)
    return qc.snapshot(pods), pre


@pytest.mark.parametrize("depth", (1, 2, 3))
@pytest.mark.parametrize("n", (1, 2, 255, 256, 257, 1025))
def test_ties_on_the_leading_components(n, depth):
    check(*tie_case(n, depth))
