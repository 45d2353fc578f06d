"""Launch lists of disruption commands from plain C: tests/c/launch_cmd_check.c is compiled with gcc against
include/karpenter_amd.h only and linked to libkarpenter_amd.so.  The client runs a pass and a Drift command with
ks_solve_opts.launch_lists set, reads ks_cons_claim_launch and ks_cons_disrupt_launch and compares them with the
oracle's lists, which this test writes to files (prices as hexadecimal floating constants: exact)."""
import json
import os
import subprocess

import pytest

import disrupt_cases as dc
import launch_cmd_cases as cc
from karpenter_amd import Consolidator

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "c", "launch_cmd_check")


def _expectation(path, names, prices, nopt):
    path.write_text("%d %d\n" % (len(names), nopt) + "".join("%s %s\n" % (n, float(p).hex()) for n, p in zip(names, prices)))
    return path


@pytest.mark.gpu
def test_c_client_reads_command_launch_lists(tmp_path):
    import __graft_entry__

    __graft_entry__.build_abi_check()
    snap = dc.mark(cc.cut_case(33), "drift")
    for n in snap["stateNodes"]:
        dc.fill(n)  # the drifted node's pods need a replacement
    want = cc.oracle_consolidate("abi", snap)
    cmd = want["multi"]["command"]
    assert cmd["action"] == "replace"
    dwant, dlists = cc.oracle_disrupt("abi", snap)
    assert dwant["command"]["action"] == "replace" and dlists
    got = Consolidator(json.dumps(snap)).consolidate(launch_lists=True)
    sim = got["multi"]["command"]["sim"]
    assert sim >= 0
    snap_path = tmp_path / "snap.json"
    snap_path.write_text(json.dumps(snap))
    cons = _expectation(tmp_path / "cons.txt", *cc.expected_launch(snap, cmd["replacement"]))
    disrupt = _expectation(tmp_path / "disrupt.txt", *dlists[0])
    out = subprocess.run([EXE, str(snap_path), str(sim), str(cons), str(disrupt)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert json.loads(out.stdout) == {"cons_entries": len(cc.expected_launch(snap, cmd["replacement"])[0]),
                                      "disrupt_entries": len(dlists[0][0]), "off_rc_cons": -6, "off_rc_disrupt": -6,
                                      "launch_ms_positive": 1}
