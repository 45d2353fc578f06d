"""KS_CONS_PLACEMENTS and ks_cons_sim_results from plain C: tests/c/placements_check.c is compiled with gcc against
include/karpenter_amd.h only and linked to libkarpenter_amd.so.  CPU: the header states both names, the library
exports the function (it refuses a NULL handle without touching a device), and the Python mirror exposes both.
GPU: the C client's documents are the Python binding's."""
import json
import os
import subprocess

import pytest

import placements_cases as pc
from karpenter_amd import Consolidator, scheduler

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "c", "placements_check")
DRIFT = 2  # KS_DISRUPT_DRIFT
KS_ERR_ARG = -6


def _run(*args):
    import __graft_entry__

    __graft_entry__.build_abi_check()
    out = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout)


def test_c_client_sees_the_flag_and_the_function():
    assert _run("abi") == {"KS_CONS_PLACEMENTS": 8, "null_handle": KS_ERR_ARG}


def test_python_mirror_exposes_both():
    import inspect

    assert scheduler.KS_CONS_PLACEMENTS == 8
    assert "placements" in inspect.signature(Consolidator.disrupt).parameters
    assert inspect.signature(Consolidator.disrupt).parameters["placements"].default is False
    assert list(inspect.signature(Consolidator.sim_results).parameters)[:3] == ["self", "sim", "device"]
    assert scheduler._cons_lib().ks_cons_sim_results.argtypes is not None


@pytest.mark.gpu
def test_c_client_placements(tmp_path):
    snap = pc.snapshot("targets")
    path = tmp_path / "snap.json"
    path.write_text(json.dumps(snap))
    got = _run("disrupt", path, DRIFT)
    want = Consolidator(json.dumps(snap)).disrupt("drift", placements=True)
    for doc in (got, want):
        doc.pop("kernel_ms"), doc.pop("placements_ms")
    assert got == want and [len(r["pods"]) for r in got["command"]["replacements"]] == [1, 1]


@pytest.mark.gpu
def test_c_client_sim_results(tmp_path):
    snap = pc.pass_cluster()
    path = tmp_path / "snap.json"
    path.write_text(json.dumps(snap))
    c = Consolidator(json.dumps(snap))
    c.run(0, 1, keep=True)
    sim = c.num_sims - 1
    want = c.sim_results(sim)
    got = _run("sim", path, sim)
    got.pop("kernel_ms"), want.pop("kernel_ms")
    assert got == want and got["sim"] == sim
