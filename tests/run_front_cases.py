"""Problems of the LEAN Solve's run-capacity tests (test_run_front_gpu.py) and of the recorded counters they are
held against (tests/golden/lean_step_counters.json): every NodeClaim count below is the oracle's."""
from karpenter_amd import synth


def non_chain(n_cpu, n_mem, n_small):
    """fake.InstanceTypes(12) is a chain (every type dominates the ones before it); four more types -- most cpu, most
    memory, most pods, and cpu-big again at a higher position (a tie) -- leave a Pareto front of four: the chain's
    last type and the first three of them.  Three pod classes, each ending its NodeClaims on another front member."""
    its = synth.fake_instance_types(12) + [
        synth.fake_instance_type("cpu-big", 32, 16, pods=60),
        synth.fake_instance_type("mem-big", 4, 128, pods=60),
        synth.fake_instance_type("pods-big", 8, 32, pods=200),
        synth.fake_instance_type("cpu-big-twin", 32, 16, pods=60),
    ]
    snap = synth.benchmark_snapshot(0, 1, 1, diverse=False)
    snap["instanceTypes"] = its
    snap["instanceTypesByNodePool"] = {"default-pool": list(range(len(its)))}
    classes = [("2", "256Mi", n_cpu), ("100m", "8Gi", n_mem), ("50m", "64Mi", n_small)]
    pods = []
    for cpu, mem, n in classes:
        pods += [synth.pod(len(pods) + i, cpu=cpu, mem=mem) for i in range(n)]
    snap["pods"] = pods
    return snap


def chain():
    return synth.benchmark_snapshot(1500, 20, 5, diverse=False)


def requirement(pods, its, seed, key, op, values):
    """The template's requirement keeps instance types out of every NodeClaim's options."""
    snap = synth.benchmark_snapshot(pods, its, seed, diverse=False)
    snap["nodeClaimTemplates"] = [synth.node_pool("default-pool", requirements=[
        {"key": key, "operator": op, "values": values}])]
    return snap


def pool_limit(cpu):
    """1500 cpu are 25 NodeClaims of the largest type (60 cpu) to the last one; 1470 leave 30 for the 25th, whose
    options then lack every type above 30 cpu, the front member among them."""
    snap = synth.benchmark_snapshot(3000, 60, 7, diverse=False)
    snap["nodePools"] = [synth.node_pool("default-pool", limits={"cpu": cpu})]
    return snap


# name -> (builder, NodeClaims, pod errors)
CASES = {
    "front3_115": (lambda: non_chain(600, 600, 9000), 115, 0),
    "front3_31": (lambda: non_chain(150, 150, 2500), 31, 0),
    "chain_64": (chain, 64, 0),
    "notin_top_66": (lambda: requirement(1500, 20, 5, "integer", "NotIn", ["20"]), 66, 0),
    "small_only_111": (lambda: requirement(600, 20, 3, "size", "In", ["small"]), 111, 0),
    "pool_limit_25": (lambda: pool_limit("1500"), 25, 1870),
    "pool_limit_part_25": (lambda: pool_limit("1470"), 25, 1900),
    # the shapes of test_claim_run_cross_gpu.py (its SHAPES)
    "cross_11": (lambda: synth.benchmark_snapshot(700, 60, 42, diverse=False), 11, 0),
    "cross_46": (lambda: synth.benchmark_snapshot(3000, 60, 7, diverse=False), 46, 0),
    "cross_56": (lambda: synth.benchmark_snapshot(600, 8, 3, diverse=False), 56, 0),
    "cross_151": (lambda: synth.benchmark_snapshot(2000, 10, 8, diverse=False), 151, 0),
}

# The counters that do not depend on how the run capacity is taken: the kernel must reproduce them
PINNED = ("pops", "ncommits", "nclaims", "runs", "runPods", "sorts", "sortsWithDescent", "sortsClosed", "sortsExact",
          "runCross", "runCrossStops", "runCrossLost", "claimFull", "tplMemoHits", "algBytes")
