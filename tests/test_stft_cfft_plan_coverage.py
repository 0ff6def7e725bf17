"""The case table of tests/stft_cfft_cases.py reaches every plan class of the fused window + complex FFT front for I/Q input: every
class has a case, every claim holds on the describe line of its case (host arithmetic, no GPU), a sweep of the planner over every
supported n_fft and over row counts at the edges emits no shape -- radix schedule, rows per workgroup, lanes per row, columns per
lane, LDS bytes -- that the table's cases do not hold, and the plan of n complex points has the lanes per row, the rows per workgroup
and the passes of the real plan (bhwp_stft_fft_plan) of 2n points."""
import pytest

from blackman_harris_win_amd import binding as B

import stft_cfft_cases as CC
import stft_fft_cases as FC

CLAIMS = [(c["id"], name) for c in CC.CASES for name in c["classes"]]


@pytest.mark.parametrize("name", list(CC.CLASSES))
def test_every_class_has_a_case(name):
    claimed = [c for c in CC.CASES if name in c["classes"]]
    assert claimed, f"no case claims the class {name!r}"
    for c in claimed:
        line = CC.line(c)
        assert CC.CLASSES[name](c, CC.parse(line)), f"case {c['id']} is not of the class {name!r}: {line}"


@pytest.mark.parametrize("cid,name", CLAIMS, ids=[f"{c}: {n}" for c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(cid, name):
    assert name in CC.CLASSES, f"case {cid} claims {name!r}, which is no class"
    c = CC.case(cid)
    line = CC.line(c)
    assert CC.CLASSES[name](c, CC.parse(line)), f"case {cid} is not of the class {name!r}: {line}"


def test_case_ids_are_unique_and_every_case_is_there_for_a_class():
    ids = CC.case_ids()
    assert len(set(ids)) == len(ids), ids
    assert all(c["classes"] for c in CC.CASES)


def _shape(d):
    return (d["n_fft"], d["schedule"], d["lpf"], d["fy"], d["cpl"], d["lds"])


def test_the_planner_emits_no_shape_without_a_case():
    """The plan's shape is a function of n_fft alone; rows only set the groups and the grid, the flags only the output.  Every n_fft
    the checks accept, at one row, at the edges of a group and of the grid, under every flag combination: the shape is one a case has,
    the groups cover the rows once and the grid is min(groups, 2048)."""
    p = CC.params(4)
    covered = {_shape(CC.parse(CC.line(c))) for c in CC.CASES}
    seen = set()
    for lg in range(4, 12):
        n = 1 << lg
        assert n in CC.SCHEDULES
        for rows in (1, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 64 * 2048, 64 * 2048 + 1, 300000):
            for flags in range(8):
                s = B.make_stft(1, (rows - 1) * 7 + n, rows, 7, n, channels=2, shift=31)
                d = CC.parse(B.describe_stft_cfft(p, n, s, detrend=bool(flags & 1), power=bool(flags & 2), fftshift=bool(flags & 4)))
                assert _shape(d) in covered, d["line"]
                assert (d["detrend"], d["power"], d["shifted"]) == (bool(flags & 1), bool(flags & 2), bool(flags & 4)), d["line"]
                assert d["schedule"] == CC.SCHEDULES[n] and d["m"] == n and d["lpf"] * d["fy"] == 256 and d["lpf"] * d["cpl"] == n
                assert d["cpl"] in (4, 8) and d["lpf"] == min(256, max(4, n // 4))
                assert d["lds"] == 2 * d["fy"] * n * 8 + n // 2 * 8 + d["fy"] * 8 <= 2 * 2048 * 8 + 1024 * 8 + 8
                assert d["groups"] == -(-rows // d["fy"]) and d["grid"] == min(d["groups"], CC.MAX_GRID)
                seen.add(_shape(d))
    assert seen == covered                          # and no case is of a shape the planner would not emit


def test_the_plan_of_n_complex_points_is_the_real_plan_of_2n():
    p = CC.params(4)
    for lg in range(4, 12):
        n = 1 << lg
        d = CC.parse(B.describe_stft_cfft(p, n, B.make_stft(2, 100000, 5, 7, n, channels=2, shift=31)))
        r = FC.parse(B.describe_stft_fft(p, n, B.make_stft(2, 100000, 5, 7, 2 * n, shift=31)))
        assert (d["lpf"], d["fy"], d["schedule"], d["m"]) == (r["lpf"], r["fy"], r["schedule"], r["m"]), (d["line"], r["line"])
        assert CC.SCHEDULES[n] == FC.SCHEDULES[2 * n]


def test_unsupported_sizes_have_no_plan():
    p = CC.params(4)
    for n in (8, 15, 17, 100, 4096, 8192):
        with pytest.raises(B.BhwError) as e:
            B.describe_stft_cfft(p, min(n, 8), B.make_stft(1, 100000, 3, 7, n, channels=2, shift=31))
        assert e.value.code == -2, e.value                 # BHW_ERR_UNSUPPORTED
    with pytest.raises(B.BhwError) as e:                   # real input has calls of its own
        B.describe_stft_cfft(p, 8, B.make_stft(1, 100000, 3, 7, 64, channels=1, shift=31))
    assert e.value.code == -2 and "bhw_stft_fft_f32_" in e.value.detail
