"""Drift / Expiration from plain C: tests/c/disrupt_check.c is compiled with gcc against include/karpenter_amd.h
only and linked to libkarpenter_amd.so.  CPU: the host-only entry point answers like the Python binding.  GPU: one
ks_cons_disrupt call answers like Consolidator.disrupt."""
import json
import os
import subprocess

import pytest

import disrupt_cases as dc
from karpenter_amd import Consolidator, inspect_disruption

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "c", "disrupt_check")
DRIFT = 2  # KS_DISRUPT_DRIFT


def _run(mode, snap, tmp_path, *args):
    import __graft_entry__

    __graft_entry__.build_abi_check()
    path = tmp_path / "snap.json"
    path.write_text(json.dumps(snap))
    out = subprocess.run([EXE, mode, str(path)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout)


def test_c_client_inspects(tmp_path):
    snap = dc.mark(dc.small(), "drift")
    got = _run("inspect", snap, tmp_path, DRIFT)
    assert got == inspect_disruption(json.dumps(snap), "drift") and len(got["candidates"]) == 14


@pytest.mark.gpu
def test_c_client_disrupts(tmp_path):
    snap = dc.claims_case(2)
    got = _run("disrupt", snap, tmp_path, DRIFT, 1)  # KS_CONS_ALL_SIMS
    want = Consolidator(json.dumps(snap)).disrupt("drift", all_sims=True)
    got.pop("kernel_ms"), want.pop("kernel_ms")
    assert got == want and len(got["command"]["replacements"]) == 2 and len(got["sims"]) == 4
