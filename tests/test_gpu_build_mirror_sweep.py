"""The octant-mirror table build (k_table_build_mirror, pass 1 of the table strategy) at every configuration the planner sends to
it at PW 22..26 (GPU): the three bit-models at every width (the VHDL model also at precisions 2 and 7), 176 configurations that
between them run all 60 reachable instances <NITER 21..32, FMT 2 | 3 | 5, THREADS 256 | 1024> of the dispatch with every cell log
(build_mirror_cases.py, test_build_mirror_cases.py).

Per configuration the table is read through a PROBE: the two-term window aa = [0, 2^(W-2)] under the HLS sum is -cos word for word
(proved on the oracle alone in test_build_mirror_cases.py), so over one whole period the quadrant map puts c and s of every
first-quadrant entry, every bit of them, into the output.  The built-in windows hide last bits (BH-7 weighs a table word's LSB
by 0.43 of an output LSB and less); BH-7 is compared as well, as the window the headline path produces.

  * reference: the same windows from ALGO_DIRECT (one chain per coefficient, no code shared with the table), kept on the device and
    tied to the CPU oracle in six slices of 4 096 words: the start, the middle entry E/2 (a deferred chain of the build's last
    workgroup), the quadrant seam (entries E-1 and 0), the half and three-quarter points, and the end;
  * under each format limit -- nibble, nibble + escapes, residual -- the configuration's verdicts are forgotten, the plan must
    name the predicted instance as unverified, the call that settles the format (the checked copy of the walk) and the calls after
    prepare() (the unchecked copy) must reproduce the reference bit for bit;
  * the format each limit settles on is the one the host model predicts (tools/sim_build.cpp through test_build_mirror_host.py,
    tests/golden/build_mirror_host.json): plain nibbles if and only if no entry leaves the four-bit fields, nibble + escapes if
    and only if no build workgroup lists more than kEscFill = 96 entries (vhdl 25 / 26 and 26 / 30 list 98 and 99).

No tolerance anywhere.  A failure names the first differing stream index, its table entry u = index mod E, the quadrant and the
two words.

The kernel's "list full" branch (a worklist beyond kWorkMax deferred images) is not covered here or anywhere: the host sweep
shows it unreached at PW <= 26, the fullest workgroup holding a seventh of the list (test_build_mirror_host.py).

PW 27..30 are left out: they run the same instances as PW 26 (test_build_mirror_cases.py enumerates them), and windows of 0.5 to
4 GiB do not belong in a test of a fraction of a second.
"""
import numpy as np
import pytest

import build_mirror_cases as C
import oracle_lib as O
from blackman_harris_win_amd import binding as B

pytestmark = pytest.mark.gpu

SLICE = 4096
FMT_OF = {"nibble": 3, "nibble+esc": 5, "residual": 2}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def host_rows():
    rows = C.host_rows()
    assert set(rows) == set(C.configurations())
    return rows


def _assert_same(torch, got, want, what):
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero().flatten()
    i = int(bad[0])
    entries = got.numel() // 4
    pytest.fail("%s: %d words differ, the first at stream index %d = entry u %d in quadrant %d: got %d, want %d"
                % (what, bad.numel(), i, i % entries, i // entries, int(got[i]), int(want[i])))


def _format_name(plan):
    return plan[len("table["):plan.index("]")].split(",")[0]


def test_settled_table_of_the_build_loop_test_agrees_with_the_host_figures():
    from test_build_mirror_host import test_settled_table_of_the_build_loop_test_agrees as check
    check()


@pytest.mark.parametrize("cfg", C.configurations(), ids=C.case_id)
def test_mirror_build_is_exact_under_every_format_limit(torch, host_rows, cfg):
    import blackman_harris_win_amd as bhw
    model, pw, w, precision = cfg
    n_iter, threads, _ = C.mirror_rule(*cfg)
    n = 1 << pw
    probe, bh7 = C.probe_params(*cfg), C.bh7_params(*cfg)
    for p in (probe, bh7):
        assert B.describe_plan(p, 0, n, algo=B.ALGO_DIRECT).startswith("direct:")
    want = {"probe": bhw.generate(probe, 0, n, algo=B.ALGO_DIRECT), "BH-7": bhw.generate(bh7, 0, n, algo=B.ALGO_DIRECT)}
    for name, p in (("probe", probe), ("BH-7", bh7)):
        for a in (0, n // 8 - SLICE // 2, n // 4 - SLICE // 2, n // 2 - SLICE // 2, 3 * n // 4 - SLICE // 2, n - SLICE):
            assert np.array_equal(want[name][a:a + SLICE].cpu().numpy(), O.generate_mt(O.from_bhw(p), a, SLICE, threads=1)), (name, a)
    got = torch.zeros(n, dtype=torch.int32, device=want["probe"].device)

    for limit_name, limit, fmt in C.LIMITS:
        C.forget_verdicts(probe)
        plan = B.describe_plan(probe, 0, n, algo=B.ALGO_TABLE, table_format=limit)
        assert "unverified" in plan and "k_table_build_mirror<%d,%d,%d>" % (n_iter, fmt, threads) in plan, plan
        got.zero_()
        bhw.generate(probe, 0, n, algo=B.ALGO_TABLE, table_format=limit, out=got)           # settles the format: checked builds
        _assert_same(torch, got, want["probe"], "probe, checked builds under %s" % limit_name)
        settled = B.describe_plan(probe, 0, n, algo=B.ALGO_TABLE, table_format=limit)
        assert "unverified" not in settled, settled
        name = _format_name(settled)
        predicted = C.predicted_format(host_rows[cfg], limit_name)
        if predicted:
            assert name == predicted, (settled, host_rows[cfg])
        else:
            assert name not in ("nibble", "nibble+esc"), (settled, host_rows[cfg])
        if name in FMT_OF:
            assert "k_table_build_mirror<%d,%d,%d>" % (n_iter, FMT_OF[name], threads) in settled, settled
        bhw.prepare(probe)
        for what, p in (("probe", probe), ("BH-7", bh7)):
            again = B.describe_plan(p, 0, n, algo=B.ALGO_TABLE, table_format=limit)
            assert _format_name(again) == name and "unverified" not in again, (again, settled)
            got.zero_()
            bhw.generate(p, 0, n, algo=B.ALGO_TABLE, table_format=limit, out=got)           # the settled format: no check
            _assert_same(torch, got, want[what], "%s, settled format %s under %s" % (what, name, limit_name))
