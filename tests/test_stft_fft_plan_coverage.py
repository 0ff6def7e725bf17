"""The case table of tests/stft_fft_cases.py reaches every plan class of the fused window + FFT front: every class has a case, every
claim holds on the describe line of its case (host arithmetic, no GPU), and a sweep of the planner over every supported n_fft and
over row counts at the edges emits no shape -- radix schedule, rows per workgroup, lanes per row, columns per lane, LDS bytes -- that
the table's cases do not hold."""
import pytest

from blackman_harris_win_amd import binding as B

import stft_fft_cases as FC

CLAIMS = [(c["id"], name) for c in FC.CASES for name in c["classes"]]


@pytest.mark.parametrize("name", list(FC.CLASSES))
def test_every_class_has_a_case(name):
    claimed = [c for c in FC.CASES if name in c["classes"]]
    assert claimed, f"no case claims the class {name!r}"
    for c in claimed:
        line = FC.line(c)
        assert FC.CLASSES[name](c, FC.parse(line)), f"case {c['id']} is not of the class {name!r}: {line}"


@pytest.mark.parametrize("cid,name", CLAIMS, ids=[f"{c}: {n}" for c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(cid, name):
    assert name in FC.CLASSES, f"case {cid} claims {name!r}, which is no class"
    c = FC.case(cid)
    line = FC.line(c)
    assert FC.CLASSES[name](c, FC.parse(line)), f"case {cid} is not of the class {name!r}: {line}"


def test_case_ids_are_unique_and_every_case_is_there_for_a_class():
    ids = FC.case_ids()
    assert len(set(ids)) == len(ids), ids
    assert all(c["classes"] for c in FC.CASES)


def _shape(d):
    return (d["n_fft"], d["schedule"], d["lpf"], d["fy"], d["cpl"], d["lds"])


def test_the_planner_emits_no_shape_without_a_case():
    """The plan's shape is a function of n_fft alone; rows only set the groups and the grid.  Every n_fft the checks accept, at one row,
    at the edges of a group and of the grid, with and without detrending: the shape is one a case has, the groups cover the rows once
    and the grid is min(groups, 2048)."""
    p = FC.params(4)
    covered = {_shape(FC.parse(FC.line(c))) for c in FC.CASES}
    seen = set()
    for lg in range(4, 13):
        n = 1 << lg
        assert n in FC.SCHEDULES
        for rows in (1, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 64 * 2048, 64 * 2048 + 1, 300000):
            for det in (False, True):
                s = B.make_stft(1, (rows - 1) * 7 + n, rows, 7, n, shift=31)
                d = FC.parse(B.describe_stft_fft(p, n, s, detrend=det))
                assert _shape(d) in covered, d["line"]
                assert d["schedule"] == FC.SCHEDULES[n] and d["m"] == n // 2 and d["lpf"] * d["fy"] == 256 and d["lpf"] * d["cpl"] == n
                assert d["lds"] == 2 * d["fy"] * d["m"] * 8 + d["m"] * 8 + d["fy"] * 4 <= 65536
                assert d["groups"] == -(-rows // d["fy"]) and d["grid"] == min(d["groups"], FC.MAX_GRID)
                seen.add(_shape(d))
    assert seen == covered                          # and no case is of a shape the planner would not emit


def test_unsupported_sizes_have_no_plan():
    p = FC.params(4)
    for n in (8, 15, 17, 100, 8192):
        with pytest.raises(B.BhwError) as e:
            B.describe_stft_fft(p, min(n, 8), B.make_stft(1, 100000, 3, 7, n, shift=31))
        assert e.value.code == -2, e.value                 # BHW_ERR_UNSUPPORTED
