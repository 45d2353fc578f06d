"""The consolidation decision replay (ks_cons_decide / ks_cons_decide_clock) against the oracle on every route a
caller can take to it, under every virtual clock that cuts the multi-node search or the single-node scan.

Routes: world 1 with the requirement records read inline from the handle's launch (records copied out, or kept in
the handle), world 1 with the caller-built requirement table, and worlds 2 and 3 (one handle per rank in this
process, the table gathered from the owners).  The table is built in ks_cons_needed_sims order, which has no clock
(include/karpenter_amd.h); a clock that stops the multi-node search early leaves rows in it the replay never
reads, in front of rows it does (decide_cases.SHIFT; tests/test_decide_preconditions.py keeps those clusters
honest on the CPU).

One test = one cluster on one route: the simulations run once, then decide() is called on the same handles for
every clock and flag set, so the result must not depend on the clock of an earlier call (the multi-node search is
cached per handle, keyed on the clock), and a last clockless decide() must still equal the clockless oracle.
Reference everywhere: oracle.bridge.consolidate / consolidate_clock, full-document equality."""
import pytest

import decide_cases as dc
from karpenter_amd import Consolidator

pytestmark = pytest.mark.gpu

ROUTES = ["inline", "kept", "table", "world2", "world3"]


def _setup(name, route):
    """The handles (handle 0 decides), the records to pass, the world and the fetch callback of a route."""
    snap = dc.snapshot(name)
    if route in ("inline", "kept", "table"):
        c = Consolidator(snap)
        if route == "kept":
            recs, _ = c.run(0, 1, keep=True)
            assert recs is None
        else:
            recs = bytes(c.run(0, 1)[0])
        return [c], recs, 1, (c.claim_requirements if route == "table" else None)
    world = int(route[5:])
    ranks = [Consolidator(snap) for _ in range(world)]  # one handle per "GPU"
    recs = b"".join(bytes(ranks[r].run(r, world)[0]) for r in range(world))
    return ranks, recs, world, lambda s: ranks[s % world].claim_requirements(s)


def _lean(doc):
    """What the sims=False, candidates=False output keeps of a full document."""
    return {"candidates": [],
            "multi": {"command": doc["multi"]["command"], "sims": [],
                      "path": [{k: p[k] for k in ("mid", "carried", "action")} for p in doc["multi"]["path"]]},
            "single": {"command": doc["single"]["command"], "sims": []}}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", dc.CLUSTERS)
def test_decide_equals_oracle(name, route):
    handles, recs, world, fetch = _setup(name, route)
    c = handles[0]
    bad, checked = [], 0  # every clock and flag set is run; the failures are reported together
    for clock in dc.clocks(name) + [None]:  # (the last one: clockless again, after every clocked call)
        for all_sims in (False, True):
            want = dc.oracle(name, clock, all_sims)
            where = "clock=%r all_sims=%r: " % (clock, all_sims)
            got = c.decide(recs, world, all_sims=all_sims, fetch=fetch, clock=clock)
            d = dc.first_diff(want, got)
            if d is not None:
                bad.append(where + d)
            if name in dc.CARRY:
                carried = sum(1 for p in want["multi"]["path"] if p["carried"])
                if c.last_reruns < carried:
                    bad.append(where + "last_reruns %d < %d carried probes" % (c.last_reruns, carried))
            # the bench's flag set: the commands and the search path of the full output, nothing else
            lean = c.decide(recs, world, all_sims=all_sims, fetch=fetch, clock=clock, sims=False, candidates=False)
            d = dc.first_diff(_lean(want), lean)
            if d is not None:
                bad.append(where + "sims=False candidates=False: " + d)
            checked += 1
    for h in handles:
        h.close()
    assert checked == 2 * (len(dc.clocks(name)) + 1)
    assert not bad, "%s %s: %d differences from the oracle\n%s" % (name, route, len(bad), "\n".join(bad))
