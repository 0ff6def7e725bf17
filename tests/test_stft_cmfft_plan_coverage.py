"""The case table of tests/stft_cmfft_cases.py reaches every plan class of the mixed-radix fused window + complex FFT front for I/Q
input: every class has a case, every claim holds on the describe line of its case (host arithmetic, no GPU), and a sweep of the
planner over EVERY supported n_fft, over row counts at the edges and every flag combination emits no shape -- a pass of some radix
in some place with idle, exactly enough or too few lanes; a row layout -- that the table's cases do not hold, with at most 8 columns
per lane and 48 608 bytes of LDS everywhere."""
import pytest

from blackman_harris_win_amd import binding as B

import stft_cmfft_cases as XC

CLAIMS = [(c["id"], name) for c in XC.CASES for name in c["classes"]]
ODD = [25, 27, 45, 75, 81, 125, 135, 225, 243, 375, 405, 625, 675, 729, 1125, 1215, 1875, 2025]


@pytest.mark.parametrize("name", list(XC.CLASSES))
def test_every_class_has_a_case(name):
    claimed = [c for c in XC.CASES if name in c["classes"]]
    assert claimed, f"no case claims the class {name!r}"
    for c in claimed:
        line = XC.line(c)
        assert XC.CLASSES[name](c, XC.parse(line)), f"case {c['id']} is not of the class {name!r}: {line}"


@pytest.mark.parametrize("cid,name", CLAIMS, ids=[f"{c}: {n}" for c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(cid, name):
    assert name in XC.CLASSES, f"case {cid} claims {name!r}, which is no class"
    c = XC.case(cid)
    line = XC.line(c)
    assert XC.CLASSES[name](c, XC.parse(line)), f"case {cid} is not of the class {name!r}: {line}"


def test_case_ids_are_unique_and_every_case_is_there_for_a_class():
    ids = XC.case_ids()
    assert len(set(ids)) == len(ids), ids
    assert all(c["classes"] for c in XC.CASES)
    assert all(c["B"] <= 5 and c["T"] <= 10000 for c in XC.CASES)


def test_the_supported_sizes():
    sizes = [n for n in range(1, 5000) if B.cmfft_supported(n)]
    assert sizes == XC.SIZES and len(sizes) == 91 and sizes[0] == 18 and sizes[-1] == 2025
    assert [n for n in sizes if n % 2] == ODD and len(sizes) - len(ODD) == 73
    assert (B.CMFFT_MIN_N, B.CMFFT_MAX_N) == (16, 2047)
    for n in (1536, 1200, 600, 300, 180, 1000, 2000, 480, 960):
        assert n in sizes
    for n in (16, 512, 1024, 2048, 15, 14, 21, 28, 35, 49, 2160, 2187, 2250, 4050):      # powers of two, out of range, factors of 7
        assert n not in sizes


def test_the_planner_emits_no_shape_without_a_case():
    """The plan's shape is a function of n_fft alone; rows only set the groups and the grid, the flags only the output form, the
    route only the kernel (tests/cpp/san_stft_cmfft.cpp sweeps the planner with from_table true and false: the same fields; the table
    route's line needs a device and is read by tests/test_gpu_stft_iq_mixed.py).  Every n_fft the checks accept, at one row, at the
    edges of a group and of the grid, under every flag combination: every pass shape and the row layout are ones a case has; the
    lanes, the columns, the twiddles and the LDS follow the contract's formulas; the product of the schedule is n; the groups cover
    the rows once."""
    p = XC.params(4)
    parsed = [XC.parse(XC.line(c)) for c in XC.CASES]
    passes = set().union(*(XC.pass_shapes(d) for d in parsed))
    layouts = {XC.layout(d) for d in parsed}
    seen_passes, seen_layouts, worst_cpl, worst_lds, worst_passes = set(), set(), 0, 0, 0
    for n in XC.SIZES:
        for rows in (1, 3, 31, 32, 33, 255, 256, 257, 2047, 2048, 2049, 32 * 2048, 32 * 2048 + 1, 300000):
            for flags in range(8):
                s = B.make_stft(1, (rows - 1) * 7 + n, rows, 7, n, channels=2, shift=31)
                d = XC.parse(B.describe_stft_cmfft(p, n, s, detrend=bool(flags & 1), power=bool(flags & 2), fftshift=bool(flags & 4)))
                assert d["line"].startswith("stft cmfft direct (") and "k_stft_cmfft_direct" in d["kernels"], d["line"]
                assert (d["detrend"], d["power"], d["shifted"]) == (bool(flags & 1), bool(flags & 2), bool(flags & 4)), d["line"]
                assert XC.pass_shapes(d) <= passes, (sorted(XC.pass_shapes(d) - passes), d["line"])
                assert XC.layout(d) in layouts, d["line"]
                lpf = d["lpf"]
                assert d["m"] == n and lpf * d["fy"] == 256 and lpf & (lpf - 1) == 0 and 4 <= lpf <= 256
                assert (4 * lpf >= n or lpf == 256) and (lpf == 4 or 2 * lpf < n), d["line"]       # the smallest power of two >= n / 4
                assert 3 <= d["cpl"] == -(-n // lpf) <= 8
                assert d["fold"] == (n if n % 2 else n // 2)
                assert d["lds"] == 2 * d["fy"] * n * 8 + d["fold"] * 8 + d["fy"] * 8 <= 48608
                assert 4 * n <= d["fy"] * n * 8                                                      # the staged window inside the first buffer
                r = d["radices"]
                prod = 1
                for q in r:
                    prod *= q
                assert prod == n and r == sorted(r, key=(5, 3, 4, 2).index) and r.count(2) <= 1 and len(r) <= 7, d["line"]
                a2 = (n & -n).bit_length() - 1                                                       # n = 2^a2 * odd
                assert r.count(4) == a2 // 2 and r.count(2) == a2 % 2, d["line"]
                assert d["groups"] == -(-rows // d["fy"]) and d["grid"] == min(d["groups"], XC.MAX_GRID)
                seen_passes |= XC.pass_shapes(d)
                seen_layouts.add(XC.layout(d))
                worst_cpl, worst_lds, worst_passes = max(worst_cpl, d["cpl"]), max(worst_lds, d["lds"]), max(worst_passes, len(r))
    assert seen_passes == passes and seen_layouts == layouts          # and no case is of a shape the planner would not emit
    assert (worst_cpl, worst_lds, worst_passes) == (8, 2 * 2025 * 8 + 2025 * 8 + 8, 7)


def test_the_printed_schedules():
    p = XC.params(4)
    for n, want in ((18, "3x3x2"), (25, "5x5"), (27, "3x3x3"), (48, "3x4x4"), (75, "5x5x3"), (100, "5x5x4"), (400, "5x5x4x4"), (1000, "5x5x5x4x2"),
                    (1200, "5x5x3x4x4"), (1215, "5x3x3x3x3x3"), (1280, "5x4x4x4x4"), (1458, "3x3x3x3x3x3x2"), (1536, "3x4x4x4x4x2"),
                    (2000, "5x5x5x4x4"), (2025, "5x5x3x3x3x3")):
        d = XC.parse(B.describe_stft_cmfft(p, 16, B.make_stft(2, 100000, 5, 7, n, channels=2, shift=31)))
        assert d["schedule"] == want and f"complex FFT of {n} points in passes {want} (no split)" in d["line"], d["line"]


def test_unsupported_sizes_have_no_plan():
    p = XC.params(4)
    for n in (14, 15, 21, 28, 35, 2160, 2187, 4050, 512, 2048):
        with pytest.raises(B.BhwError) as e:
            B.describe_stft_cmfft(p, 8, B.make_stft(1, 100000, 3, 7, n, channels=2, shift=31))
        assert e.value.code == -2, e.value                 # BHW_ERR_UNSUPPORTED
    with pytest.raises(B.BhwError) as e:                   # a power of two has calls of its own
        B.describe_stft_cmfft(p, 8, B.make_stft(1, 100000, 3, 7, 512, channels=2, shift=31))
    assert e.value.code == -2 and "bhw_stft_cfft_f32_" in e.value.detail
    with pytest.raises(B.BhwError) as e:                   # and so has real input
        B.describe_stft_cmfft(p, 8, B.make_stft(1, 100000, 3, 7, 400, channels=1, shift=31))
    assert e.value.code == -2 and "bhw_stft_mfft_f32_" in e.value.detail
