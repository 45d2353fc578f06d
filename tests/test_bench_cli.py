"""bench.py's command line: a plain run prints the headline line only, `--full` holds everything else, and
`--dump-outputs DIR` writes the timed Solve's Results as float64 arrays that are the same from run to run."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("create_ms", "structured_solve_ms", "roofline", "cpu_baseline", "solve_c1", "solve_c3", "solve_c4",
             "consolidation", "consolidation_topology")
ARRAYS = ("pod_nodeclaim", "pod_existing_node", "pod_position", "pod_error", "algorithmic_bytes", "nodeclaim_template",
          "nodeclaim_pod_counts", "nodeclaim_instance_type_counts", "nodeclaim_instance_types")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_cli_under_test", BENCH)
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


class _FakeResults:
    new_nodeclaims = [{"template": 0, "pods": np.array([4, 0, 2], np.int32), "instance_types": np.array([7, 9], np.int32)},
                      {"template": 1, "pods": np.array([3], np.int32), "instance_types": np.array([1], np.int32)}]
    existing_nodes = [(5, np.array([1], np.int32))]
    pod_errors = {6: "no instance type", 5: "no instance type"}


class _FakeScheduler:
    def solve_structured(self, device=-1):
        return _FakeResults()


def _load(d):
    return {k: np.load(os.path.join(str(d), k + ".npy")) for k in ARRAYS}


def test_dump_outputs_arrays(tmp_path):
    b = _bench()
    assert b._dump_outputs(str(tmp_path / "out"), _FakeScheduler(), 0, 7, 1234.0) == 2
    a = _load(tmp_path / "out")
    assert sorted(os.listdir(str(tmp_path / "out"))) == sorted(k + ".npy" for k in ARRAYS)
    assert all(x.dtype == np.float64 for x in a.values())
    assert a["pod_nodeclaim"].tolist() == [0, -1, 0, 1, 0, -1, -1]
    assert a["pod_existing_node"].tolist() == [-1, 5, -1, -1, -1, -1, -1]
    assert a["pod_position"].tolist() == [1, 0, 2, 0, 0, -1, -1] and a["pod_error"].tolist() == [0, 0, 0, 0, 0, 1, 1]
    assert a["nodeclaim_pod_counts"].tolist() == [3, 1]
    assert a["nodeclaim_instance_types"].tolist() == [7, 9, 1] and a["nodeclaim_instance_type_counts"].tolist() == [2, 1]
    assert a["nodeclaim_template"].tolist() == [0, 1]
    assert a["algorithmic_bytes"].tolist() == [1234.0]


def test_dump_outputs_writes_no_empty_array(tmp_path):
    class NoClaims(_FakeResults):
        new_nodeclaims = []

    class Sch:
        def solve_structured(self, device=-1):
            return NoClaims()

    assert _bench()._dump_outputs(str(tmp_path), Sch(), 0, 7, 1.0) == 0
    names = sorted(os.listdir(str(tmp_path)))
    assert names == sorted(k + ".npy" for k in ARRAYS if not k.startswith("nodeclaim_"))
    assert all(np.load(os.path.join(str(tmp_path), n)).size > 0 for n in names)


def test_dump_outputs_cap_is_a_fixed_sample(tmp_path):
    b = _bench()
    b.DUMP_CAP_BYTES = 8 * len(ARRAYS) * 2  # 2 elements per array: less than the 38 the fake Results make
    for d in ("a", "b"):
        b._dump_outputs(str(tmp_path / d), _FakeScheduler(), 0, 7, 1.0)
    a, c = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= b.DUMP_CAP_BYTES
    assert a["pod_nodeclaim"].size == 2 and a["nodeclaim_instance_types"].size == 2 and a["pod_error"].size == 2
    assert all(np.array_equal(a[k], c[k]) for k in ARRAYS)


def test_other_workloads_need_full():
    for extra in (["--only-consolidation"], ["--only-solve", "c1"]):
        p = subprocess.run([sys.executable, BENCH] + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "--full" in p.stderr and p.stdout == ""


@pytest.mark.gpu
def test_plain_run_headline_and_dump(tmp_path):
    from karpenter_amd import Scheduler, synth

    pods, its = 700, 60
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--pods", str(pods),
                        "--its", str(its), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1
    doc = json.loads(lines[0])
    assert all(k in doc for k in HEADLINE) and not any(k in doc for k in FULL_ONLY)
    assert doc["steps"] == 3 and doc["unit"] == "pods/s" and doc["higher_is_better"] is True and doc["dtype"] == "int64"
    assert doc["ms_per_step"] > 0 and abs(doc["value"] - pods / (doc["ms_per_step"] / 1000.0)) <= 0.01 * doc["value"]
    # the dumped arrays are the Results of the same problem solved here
    a = _load(out)
    r = Scheduler(json.dumps(synth.benchmark_snapshot(pods, its, 42, False))).solve(device=0)
    want = np.full(pods, -1.0)
    for i, c in enumerate(r.new_nodeclaims):
        want[c["pods"]] = i
    assert all(x.dtype == np.float64 for x in a.values())
    assert np.array_equal(a["pod_nodeclaim"], want)
    pos, err = np.full(pods, -1.0), np.zeros(pods)
    for c in r.new_nodeclaims:
        pos[c["pods"]] = np.arange(len(c["pods"]))
    err[sorted(r.pod_errors)] = 1.0
    assert all(x.size > 0 for x in a.values())
    assert np.array_equal(a["pod_position"], pos) and np.array_equal(a["pod_error"], err)
    assert np.array_equal(a["pod_existing_node"], np.full(pods, -1.0))  # (the snapshot has no existing nodes)
    assert a["nodeclaim_pod_counts"].tolist() == [len(c["pods"]) for c in r.new_nodeclaims]
    assert a["algorithmic_bytes"].tolist() == [r.algorithmic_bytes]
    assert doc["config"]["new_nodeclaims"] == len(r.new_nodeclaims)
