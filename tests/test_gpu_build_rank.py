"""The rank entry of the octant-mirror table build (k_table_build_mirror, csrc/bhw_build.hip) on the device: a narrow group's first
four rotations after its split rotation are replaced by a rank among the decision tree's thresholds and one read of the group's
candidate states.  The tables must stay what they were, bit for bit.

Per configuration three windows over one whole period: the probe (aa = [0, 2^(W-2)] under the HLS sum: every bit of every table
entry reaches the output, build_mirror_cases.py) and BH-7 under ALGO_TABLE, against the same windows from ALGO_DIRECT (one chain
per coefficient, no code shared with the table build) -- on the checked copy of the walk (the call that settles the format) and
on the unchecked one (the calls after prepare()), under each format limit.  No tolerance.

Configurations (the host model's count of rank groups, tools/sim_build.cpp, in brackets):
  * the three models at PW 26 / W 32 -- the 1 024-thread shape, the headline's instance <32, 3, 1024> among them; the cpp model
    settles on nibble + escapes there [all but the first degree of the octant];
  * hls at PW 22 / W 26 and cpp at PW 24 / W 28 -- the 256-thread shape with the rank entry in nearly every group [7 990 of
    8 192; 31 972 of 32 768];
  * hls at PW 22 / W 32 -- no mirror configuration (its residual cell would be 2^5 entries: another build kernel makes this table,
    and in the host model every group splits before the ten-rotation block): the table path next to the changed kernel, compared
    the same way under the default format;
  * vhdl at PW 22 = W -- biased groups, and most groups split too late for the rank entry and keep the rotations [779 of 8 192].
"""
import pytest

import build_mirror_cases as C
from blackman_harris_win_amd import binding as B

pytestmark = pytest.mark.gpu

CASES = [("hls", 26, 32, 1), ("cpp", 26, 32, 1), ("vhdl", 26, 32, 1), ("hls", 22, 26, 1), ("cpp", 24, 28, 1), ("vhdl", 22, 22, 1)]
OTHER_BUILD = ("hls", 22, 32, 1)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _assert_same(torch, got, want, what):
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero().flatten()
    i = int(bad[0])
    entries = got.numel() // 4
    pytest.fail("%s: %d words differ, the first at stream index %d = entry u %d in quadrant %d: got %d, want %d"
                % (what, bad.numel(), i, i % entries, i // entries, int(got[i]), int(want[i])))


def test_the_cases_are_mirror_configurations_of_both_shapes():
    rules = {c: C.mirror_rule(*c) for c in CASES}
    assert all(rules.values()), rules
    assert {r[1] for r in rules.values()} == {256, 1024}
    assert rules[("hls", 26, 32, 1)] == (32, 1024, 9) and rules[("vhdl", 22, 22, 1)][0] == 21
    assert C.mirror_rule(*OTHER_BUILD) is None
    rows = C.host_rows()
    assert C.predicted_format(rows[("cpp", 26, 32, 1)], "nibble") == "nibble+esc"


@pytest.mark.parametrize("cfg", CASES, ids=C.case_id)
def test_tables_with_the_rank_entry_are_exact(torch, cfg):
    import blackman_harris_win_amd as bhw
    n_iter, threads, _ = C.mirror_rule(*cfg)
    n = 1 << cfg[1]
    probe, bh7 = C.probe_params(*cfg), C.bh7_params(*cfg)
    want = {"probe": bhw.generate(probe, 0, n, algo=B.ALGO_DIRECT), "BH-7": bhw.generate(bh7, 0, n, algo=B.ALGO_DIRECT)}
    got = torch.zeros(n, dtype=torch.int32, device=want["probe"].device)
    for limit_name, limit, fmt in C.LIMITS:
        C.forget_verdicts(probe)
        plan = B.describe_plan(probe, 0, n, algo=B.ALGO_TABLE, table_format=limit)
        assert "unverified" in plan and "k_table_build_mirror<%d,%d,%d>" % (n_iter, fmt, threads) in plan, plan
        bhw.generate(probe, 0, n, algo=B.ALGO_TABLE, table_format=limit, out=got)               # the checked walk
        _assert_same(torch, got, want["probe"], "probe, checked walk under %s" % limit_name)
        bhw.prepare(probe)
        for what, p in (("probe", probe), ("BH-7", bh7)):
            settled = B.describe_plan(p, 0, n, algo=B.ALGO_TABLE, table_format=limit)
            assert "unverified" not in settled, settled
            got.zero_()
            bhw.generate(p, 0, n, algo=B.ALGO_TABLE, table_format=limit, out=got)               # the unchecked walk
            _assert_same(torch, got, want[what], "%s, unchecked walk under %s (%s)" % (what, limit_name, settled))


def test_table_of_another_build_kernel_is_exact(torch):
    import blackman_harris_win_amd as bhw
    n = 1 << OTHER_BUILD[1]
    for what, p in (("probe", C.probe_params(*OTHER_BUILD)), ("BH-7", C.bh7_params(*OTHER_BUILD))):
        want = bhw.generate(p, 0, n, algo=B.ALGO_DIRECT)
        assert "k_table_build_mirror" not in B.describe_plan(p, 0, n, algo=B.ALGO_TABLE)
        C.forget_verdicts(p)
        for walk in ("first call", "after prepare()"):
            got = bhw.generate(p, 0, n, algo=B.ALGO_TABLE)
            _assert_same(torch, got, want, "%s, %s" % (what, walk))
            bhw.prepare(p)
