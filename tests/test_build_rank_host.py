"""The rank entry of the mirror table build on the host (no GPU): tools/sim_build.cpp walks every leaf of every rank group both
ways -- through its first four rotations one by one, and by its rank among the decision tree's thresholds with the group's
candidate states -- and compares state, angle and zero event, besides comparing every table entry with the plain chain.  Three
small configurations: most groups ranked (hls 22 / 26), many zero events (cpp 22 / 24), biased groups and groups that split too
late for the rank entry (vhdl 22 / 22).  The 176-configuration sweep (test_build_mirror_host.py) runs the same model: its exit
code covers the rank entry everywhere.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK = re.compile(r"rank entry J 4: groups (?P<ranked>\d+) of (?P<groups>\d+), refused (?P<refused>\d+), leaves that differ from the rotations (?P<differ>\d+), "
                  r"zero events by threshold (?P<zero_thr>\d+) \| by rotation (?P<zero_rot>\d+)")
CASES = [(0, 22, 26, 1), (1, 22, 24, 1), (2, 22, 22, 1)]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sim_rank") / "sim_build")
    subprocess.check_call(["g++", "-O2", "-o", exe, os.path.join(ROOT, "tools", "sim_build.cpp"), "-lquadmath"])
    return exe


@pytest.mark.parametrize("cfg", CASES, ids=lambda c: "model%d-%d-%d-p%d" % c)
def test_rank_entry_equals_the_rotations(sim, cfg):
    r = subprocess.run([sim] + [str(v) for v in cfg], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and len(lines) == 2 and "mismatches 0," in lines[0], r.stdout + r.stderr
    m = RANK.fullmatch(lines[1])
    assert m, lines[1]
    f = {k: int(v) for k, v in m.groupdict().items()}
    assert f["groups"] == 8192 and 0 < f["ranked"] <= f["groups"], f
    assert f["differ"] == 0 and f["refused"] == 0, f
    assert f["zero_thr"] == f["zero_rot"] > 0, f
