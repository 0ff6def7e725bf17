"""The case table of tests/stft_mfft_cases.py reaches every plan class of the mixed-radix fused window + FFT front: every class has a
case, every claim holds on the describe line of its case (host arithmetic, no GPU), and a sweep of the planner over EVERY supported
n_fft and over row counts at the edges emits no shape -- a pass of some radix in some place with idle, exactly enough or too few
lanes; a lane layout; a column layout -- that the table's cases do not hold, with at most 16 columns per lane and 64 KiB of LDS
everywhere."""
import pytest

from blackman_harris_win_amd import binding as B

import stft_mfft_cases as MC

CLAIMS = [(c["id"], name) for c in MC.CASES for name in c["classes"]]
SUPPORTED = [n for n in range(1, 5001) if B.mfft_supported(n)]


@pytest.mark.parametrize("name", list(MC.CLASSES))
def test_every_class_has_a_case(name):
    claimed = [c for c in MC.CASES if name in c["classes"]]
    assert claimed, f"no case claims the class {name!r}"
    for c in claimed:
        line = MC.line(c)
        assert MC.CLASSES[name](c, MC.parse(line)), f"case {c['id']} is not of the class {name!r}: {line}"


@pytest.mark.parametrize("cid,name", CLAIMS, ids=[f"{c}: {n}" for c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(cid, name):
    assert name in MC.CLASSES, f"case {cid} claims {name!r}, which is no class"
    c = MC.case(cid)
    line = MC.line(c)
    assert MC.CLASSES[name](c, MC.parse(line)), f"case {cid} is not of the class {name!r}: {line}"


def test_case_ids_are_unique_and_every_case_is_there_for_a_class():
    ids = MC.case_ids()
    assert len(set(ids)) == len(ids), ids
    assert all(c["classes"] for c in MC.CASES)
    assert all(c["B"] <= 5 and c["T"] <= 17500 for c in MC.CASES)


def test_the_supported_sizes():
    assert len(SUPPORTED) == 95 and SUPPORTED[0] == 18 and SUPPORTED[-1] == 4050
    for n in (400, 480, 960, 1000, 1200, 1920, 18, 4050):
        assert n in SUPPORTED
    for n in (16, 512, 4096, 14, 15, 45, 28, 22, 4374, 4500):        # powers of two, out of range, odd, factors 7 and 11
        assert n not in SUPPORTED


def test_the_planner_emits_no_shape_without_a_case():
    """The plan's shape is a function of n_fft alone; rows only set the groups and the grid, the flags only the output form.  Every
    n_fft the checks accept, at one row, at the edges of a group and of the grid, in the three forms: every pass shape, the lane layout
    and the column layout are ones a case has; the lanes, the columns and the LDS follow the contract's formulas; the groups cover the
    rows once and the grid is min(groups, 2048)."""
    p = MC.params(4)
    parsed = [MC.parse(MC.line(c)) for c in MC.CASES]
    passes = set().union(*(MC.pass_shapes(d) for d in parsed))
    layouts = {MC.layout(d) for d in parsed}
    seen_passes, seen_layouts, worst_cpl, worst_lds = set(), set(), 0, 0
    for n in SUPPORTED:
        M = n // 2
        for rows in (1, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 64 * 2048, 64 * 2048 + 1, 300000):
            for flags in range(4):
                s = B.make_stft(1, (rows - 1) * 7 + n, rows, 7, n, shift=31)
                d = MC.parse(B.describe_stft_mfft(p, n, s, detrend=bool(flags & 1), power=bool(flags & 2)))
                assert (d["detrend"], d["form"]) == (bool(flags & 1), "power" if flags & 2 else "spectrum"), d["line"]
                assert MC.pass_shapes(d) <= passes, (sorted(MC.pass_shapes(d) - passes), d["line"])
                assert MC.layout(d) in layouts, d["line"]
                lpf = d["lpf"]
                assert d["m"] == M and lpf * d["fy"] == 256 and lpf & (lpf - 1) == 0 and 4 <= lpf <= 256
                assert (4 * lpf >= M or lpf == 256) and (lpf == 4 or 2 * lpf < M), d["line"]      # the smallest power of two >= M / 4
                assert d["cpl"] == -(-n // lpf) <= 16
                assert d["lds"] == 2 * d["fy"] * M * 8 + M * 8 + d["fy"] * 4 <= 65536
                assert d["fy"] == 1 or d["fy"] * M <= 1024
                r = d["radices"]
                assert r == sorted(r, key=(5, 3, 4, 2).index) and r.count(2) <= 1, d["line"]
                a2 = (M & -M).bit_length() - 1                                                      # M = 2^a2 * odd
                assert r.count(4) == a2 // 2 and r.count(2) == a2 % 2, d["line"]
                assert d["groups"] == -(-rows // d["fy"]) and d["grid"] == min(d["groups"], MC.MAX_GRID)
                seen_passes |= MC.pass_shapes(d)
                seen_layouts.add(MC.layout(d))
                worst_cpl, worst_lds = max(worst_cpl, d["cpl"]), max(worst_lds, d["lds"])
    assert seen_passes == passes and seen_layouts == layouts          # and no case is of a shape the planner would not emit
    assert worst_cpl == 16 and worst_lds == 2 * 2025 * 8 + 2025 * 8 + 4 == 48604


def test_the_printed_schedules():
    p = MC.params(4)
    for n, want in ((400, "5x5x4x2"), (480, "5x3x4x4"), (18, "3x3"), (4050, "5x5x3x3x3x3"), (20, "5x2"), (30, "5x3"), (50, "5x5"), (96, "3x4x4"),
                    (1000, "5x5x5x4"), (1200, "5x5x3x4x2"), (1536, "3x4x4x4x4"), (4000, "5x5x5x4x4"), (2916, "3x3x3x3x3x3x2")):
        d = MC.parse(B.describe_stft_mfft(p, 16, B.make_stft(2, 100000, 5, 7, n, shift=31)))
        assert d["schedule"] == want, d["line"]


def test_unsupported_sizes_have_no_plan():
    p = MC.params(4)
    for n in (14, 15, 45, 28, 22, 4374, 4500, 512, 4096):
        with pytest.raises(B.BhwError) as e:
            B.describe_stft_mfft(p, 8, B.make_stft(1, 100000, 3, 7, n, shift=31))
        assert e.value.code == -2, e.value                 # BHW_ERR_UNSUPPORTED
    with pytest.raises(B.BhwError) as e:                   # a power of two has calls of its own
        B.describe_stft_mfft(p, 8, B.make_stft(1, 100000, 3, 7, 512, shift=31))
    assert e.value.code == -2 and "bhw_stft_fft_f32_" in e.value.detail
