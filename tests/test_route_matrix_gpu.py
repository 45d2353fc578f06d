"""Every reachable k_solve instantiation against the oracle, at live-resource counts 1 to 16.

k_solve is instantiated per (family, RT, TL, LEAN) and the host picks one per launch (ks_solve.hip launch_family,
launch_sims_mw, launch_sims_mixed).  Each case here (tests/resource_cases.py, whose inputs
tests/test_route_preconditions.py checks on the CPU) asserts two things: the result equals the oracle's in full (a
Solve's canonical Results; a consolidation's whole document, with all_sims both ways), and the route the library
reports ("stats"."route" of a Solve, Consolidator.last_routes of a pass) is the cell the case names.  A case whose
launch is not its cell fails, so the matrix cannot go vacuous when a generator or the planner changes.

Cell (family, rt, tl, lean) -> test id.  rt = R for R in {3, 4}, else 0 (the generic code); "notl": tl = 0.

  Solve                 rt3 lean  test_solve_case[solve-rt3-lean], [solve-rt3-lean-exit] (lean, then non-lean)
                        rt3 tl    [solve-rt3-tl]           rt3 notl  [solve-rt3-notl]
                        rt4 lean  [solve-rt4-lean], [solve-rt4-lean-exit]
                        rt4 tl    [solve-rt4-tl], [solve-neg-R4]      rt4 notl  [solve-rt4-notl]
                        rt0 tl    [solve-rt0-tl-R5], -R8, -R16, [solve-rt0-R1], -R2, [solve-neg-R5]
                        rt0 notl  [solve-rt0-notl-R5], [solve-rt0-notl-R16]
  Solve + topology      rt3 tl    test_solve_case[topo-rt3-tl]        rt3 notl  [topo-rt3-notl]
                        rt4 tl    [topo-rt4-tl], [topo-neg-R4]        rt4 notl  [topo-rt4-notl]
                        rt0 tl    [topo-rt0-tl-R5], -R8, -R16, [topo-rt0-R1], -R2, [topo-neg-R5]
                        rt0 notl  [topo-rt0-notl-R5], [topo-rt0-notl-R16]
  simulations           rt3 lean  test_cluster_case[sims-rt3-lean]    rt3 tl  [sims-rt3-tl]   rt3 notl  [sims-rt3-notl]
                        rt4 lean  [sims-rt4-lean]  rt4 tl  [sims-rt4-tl], [sims-neg-R4]       rt4 notl  [sims-rt4-notl]
                        rt0 tl    [sims-rt0-tl-R5], -R8, -R16, [sims-rt0-R1], -R2, [sims-neg-R5],
                                  test_sharded_decision_at_five_resources (world 2)
                        rt0 notl  [sims-rt0-notl-R5], [sims-rt0-notl-R16]
  simulations+topology  rt3 tl    test_cluster_case[simstopo-rt3-tl]  rt3 notl  [simstopo-rt3-notl]
                        rt4 tl    [simstopo-rt4-tl], [simstopo-neg-R4]  rt4 notl  [simstopo-rt4-notl]
                        rt0 tl    [simstopo-rt0-tl-R5], -R8, -R16, [simstopo-rt0-R1], -R2, [simstopo-neg-R5],
                                  [simstopo-volumes-R5] (volume limits), [simstopo-carry-R5] (carried-probe re-runs),
                                  test_validate_appends_its_launch
                        rt0 notl  [simstopo-rt0-notl-R5], [simstopo-rt0-notl-R16]
  mixed (4-wave + 1)    rt4       test_cluster_case[mixed-rt4]; rt3: tests/test_cons_mw_gpu.py

Not reachable by any input of test size:
  lean with rt0 or notl, and lean with topology: launch_family runs LEAN only for R in {3, 4} with the tables in
      LDS and no topology groups; those instantiations do not exist.
  sims_mw (k_solve<RT, true, true, false, true, true> launched alone, the second stream of launch_sims_split):
      only when the mixed launch does not fit, 4 x stride > 160 KiB with stride = the plan's LDS bytes, so a plan
      over 40 KiB.  A no-topology pass plans within 40 KiB and re-plans at 160 KiB only when the fixed part alone
      leaves no room (KO < 1); the fixed part's terms that grow are 16 bytes per 32 nodes and 20 bytes per 32
      instance types, so that takes about 80 000 nodes or 64 000 instance types.  The 4-wave body itself is the one
      the mixed launch runs on its first nmw workgroups."""
import json
import os
import socket

import pytest

import resource_cases as rc
from karpenter_amd import Consolidator, Scheduler
from test_cons_gpu import _first_diff
from test_solve_gpu import _diff

pytestmark = pytest.mark.gpu

SOLVE = [c["name"] for c in rc.SOLVE_CASES]
CONS = [c["name"] for c in rc.CONS_CASES]


def _cells(launches):
    return [(l["family"], l["rt"], l["tl"], l["lean"]) for l in launches]


@pytest.mark.parametrize("name", SOLVE)
def test_solve_case(name):
    case = rc.CASES[name]
    got = Scheduler(rc.snapshot(name)).solve(lds_budget=case["budget"])
    d = _diff(rc.oracle(name), got)
    assert d is None, d
    route = got.stats["route"]
    assert _cells(route["launches"]) == case["cells"], route
    assert all(l["n"] == 1 for l in route["launches"])
    assert _cells([route]) == case["cells"][-1:]  # the outer fields are the last launch's


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("name", CONS)
def test_cluster_case(name):
    case = rc.CASES[name]
    cell = case["cells"][0]
    with _Env(case["env"]):
        c = Consolidator(rc.snapshot(name))
        recs, _ = c.run(0, 1)
        recs = bytes(recs)
        launches = c.last_routes
        # the pass: its cell and nothing else, over every simulation
        assert launches and set(_cells(launches)) == {cell}, launches
        assert sum(l["n"] for l in launches) == c.num_sims
        if cell[0] == "sims_mixed":
            assert len(launches) == 1 and 1 <= launches[0]["nmw"] <= c.num_sims
        for all_sims in (True, False):
            got = c.decide(recs, 1, all_sims)
            d = _first_diff(rc.oracle(name, all_sims), got)
            assert d is None, d
        # a carried probe is re-run in a launch of its own (one simulation), reported after the pass's
        reruns = c.last_reruns
        after = c.last_routes
        assert after[:len(launches)] == launches and len(after) >= len(launches) + reruns
        assert all(l["n"] == 1 for l in after[len(launches):])
        assert set(_cells(after[len(launches):])) <= {cell}
        if case["reruns"]:
            assert reruns >= 1
        # the next pass starts a new list (a topology plan launches in two phases only when it is new)
        c.run(0, 1)
        again = c.last_routes
        assert set(_cells(again)) == {cell} and sum(l["n"] for l in again) == c.num_sims and len(again) <= len(launches)


def test_validate_appends_its_launch():
    from oracle import bridge

    name = "simstopo-rt0-tl-R5"
    want = rc.oracle(name, False)
    cmd = want["multi"]["command"] if want["multi"]["command"]["action"] != "no-op" else want["single"]["command"]
    assert cmd["action"] != "no-op"
    c = Consolidator(rc.snapshot(name))
    c.run(0, 1)
    n = len(c.last_routes)
    got = c.validate(cmd)
    assert got == bridge.validate(rc.snapshot(name), cmd)
    after = c.last_routes
    assert len(after) == n + 1 and after[n]["n"] == 1
    assert _cells(after[n:]) == [rc.CASES[name]["cells"][0]]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


SHARDED = "sims-rt0-tl-R5"


def _worker(rank, world, port, q):
    import sys

    import torch.distributed as dist

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import resource_cases as cases
    from karpenter_amd import Consolidator
    from karpenter_amd.sharded import ShardBuffers, sharded_pass

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c = Consolidator(cases.snapshot(SHARDED))
        bufs = ShardBuffers(c, world, "cuda:0")
        _, _, got = sharded_pass(c, rank, world, 0, bufs, all_sims=True, candidates=True, sims=True)
        routes = c.last_routes
        q.put((rank, json.dumps(got, sort_keys=True) if rank == 0 else None, routes, c.num_sims))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_sharded_decision_at_five_resources():
    """World 2 through karpenter_amd.sharded.sharded_pass (the benchmark's exchange) on an R = 5 cluster: rank 0's
    decision is the oracle's, and both ranks launched the generic simulations over their shard."""
    import torch.multiprocessing as mp

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = {}
    for _ in range(world):
        rank, doc, routes, nsims = q.get(timeout=150)
        out[rank] = (doc, routes, nsims)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = rc.oracle(SHARDED, True)
    got = json.loads(out[0][0])
    d = _first_diff(want, got)
    assert d is None, d
    cell = rc.CASES[SHARDED]["cells"][0]
    nsims = out[0][2]
    for rank in range(world):
        routes = out[rank][1]
        assert routes and set(_cells(routes)) == {cell}, routes
        assert routes[0]["n"] == (nsims - rank + world - 1) // world
