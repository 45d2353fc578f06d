"""What tests/test_decide_routes_gpu.py relies on, checked on the oracle alone (no GPU): its clusters do reach
the cases the GPU tests are there for.

ks_cons_needed_sims has no clock, so the requirement table a caller hands to ks_cons_decide_clock is in the
clockless need list's order.  When the clock stops the multi-node search early the clocked replay's own need list
is a proper subsequence of it, and a table indexed by the clocked list would render every later simulation with
another simulation's NewNodeClaims[0] requirements.  That is only visible where those records differ: these tests
assert they do, so a change of synth.cluster_snapshot or of the scenarios cannot turn the GPU tests vacuous."""
import pytest

import decide_cases as dc


def _subsequence(short, long):
    it = iter(long)
    return all(x in it for x in short)


def test_seed_305_shifts_the_single_node_command():
    clock = (0.0, 1000.0, 1.0)
    plain, cut = dc.oracle("shift-305"), dc.oracle("shift-305", clock)
    assert [p["action"] for p in plain["multi"]["path"]] == ["no-op"] * 4
    assert all(p["newNodeClaims"] > 0 and not p["carried"] for p in plain["multi"]["path"])
    assert len(cut["multi"]["path"]) == 1
    a, b = dc.need_rows(plain), dc.need_rows(cut)
    assert len(b) < len(a)
    assert _subsequence([x[0] for x in b], [x[0] for x in a])
    assert len({x[1] for x in a}) >= 3
    assert len(dc.shifted_positions(plain, cut)) >= 5  # (9 when this was written)
    # the command's own row is among them
    cmd = cut["single"]["command"]
    assert cmd["action"] == "replace"
    sims = cut["single"]["sims"]
    chosen = [i for i, x in enumerate(sims) if x["action"] != "no-op"][0]
    assert sims[chosen]["action"] == "replace" and sims[chosen]["candidates"] == cmd["candidates"]
    pos = [x[0] for x in b].index(("single", chosen))
    assert pos in dc.shifted_positions(plain, cut)


@pytest.mark.parametrize("name,clock", [(n, c) for fam in (dc.SHIFT, dc.SHIFT_CPU_ONLY) for n, cs in fam.items() for c in cs])
def test_shift_clusters_shift(name, clock):
    plain, cut = dc.oracle(name), dc.oracle(name, clock)
    assert len(cut["multi"]["path"]) < len(plain["multi"]["path"])
    a, b = dc.need_rows(plain), dc.need_rows(cut)
    assert len(b) < len(a) and _subsequence([x[0] for x in b], [x[0] for x in a])
    assert len(dc.shifted_positions(plain, cut)) >= 1
    assert clock in dc.clocks(name)  # the GPU tests do run this clock


@pytest.mark.parametrize("name", dc.CARRY)
def test_cuts_land_on_and_before_carried_probes(name):
    path = dc.oracle(name)["multi"]["path"]
    last, nxt = [], []  # per clock: the last probe run is carried; the first probe not run is carried
    for k in range(len(path)):
        cut = dc.oracle(name, (float(k), 1000.0, 1.0))["multi"]["path"]
        assert cut == path[:k + 1]  # (the carried probes' outcomes included)
        last.append(cut[-1]["carried"])
        if k + 1 < len(path):
            nxt.append(path[k + 1]["carried"])
    assert any(last), "no clock ends the search on a carried probe"
    assert any(nxt), "no cut lands just before a carried probe"


@pytest.mark.parametrize("name", dc.CLUSTERS)
def test_clock_cases_hit_what_they_name(name):
    """The fixed clocks: strict comparison at an exactly representable timeout, the accumulated 0.1s, and the
    abandoned single-node scan."""
    n = len(dc.oracle(name)["multi"]["path"])
    assert n >= 2
    for k in range(n):
        assert len(dc.oracle(name, (float(k), 1000.0, 1.0))["multi"]["path"]) == k + 1
    assert len(dc.oracle(name, (0.25, 0.75, 0.125))["multi"]["path"]) == min(n, 3)
    assert len(dc.oracle(name, (0.3, 0.9, 0.1))["multi"]["path"]) == min(n, 3)
    # the search keeps its last saved command when it is cut, the single-node scan gives its command up
    assert len(dc.oracle(name, (1000.0, 4.0, 1.0))["multi"]["path"]) == n


def test_some_single_node_scan_is_abandoned():
    """(1000, 4, 1): five single-node simulations run, then the scan is abandoned; on the clusters whose command
    comes later the command is lost."""
    lost = 0
    for name in dc.CLUSTERS:
        plain, cut = dc.oracle(name), dc.oracle(name, (1000.0, 4.0, 1.0))
        assert len(cut["single"]["sims"]) == min(5, len(plain["single"]["sims"]))
        if plain["single"]["command"]["action"] != "no-op" and cut["single"]["command"]["action"] == "no-op":
            lost += 1
    assert lost >= 2
