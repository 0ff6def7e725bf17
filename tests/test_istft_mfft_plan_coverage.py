"""The case table of tests/istft_mfft_cases.py reaches every plan class of the fused inverse mixed-radix FFT + overlap-add front: every
class has a case, every claim holds on the describe line of its case (host arithmetic, no GPU), a sweep of the planner over EVERY
supported n_fft and a grid of (L, hop, B, F) emits no pass shape, lane / column layout, slot count or column count that the table's
cases do not hold, with at most 16 columns per lane and 64 KiB of LDS everywhere, and the frame list of every span, taken from the
plan's S, is exactly the frames that reach the span's outputs."""
import pytest

from blackman_harris_win_amd import binding as B

import istft_mfft_cases as XC

CLAIMS = [(c["id"], name) for c in XC.CASES for name in c["classes"]]
SUPPORTED = [n for n in range(1, 5001) if B.mfft_supported(n)]


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
    """... and the describe line of every case restates the case's own shape, library form."""
    ids = XC.case_ids()
    assert len(set(ids)) == len(ids), ids
    for c in XC.CASES:
        assert c["classes"], c["id"]
        L, col0, pad, _, _ = XC.geometry(c)
        d = XC.parse(XC.line(c))
        assert (d["signals"], d["frames"], d["n_fft"], d["L"], d["col0"], d["pad"]) == (c["B"], c["F"], c["n_fft"], L, col0, pad), d["line"]
        assert d["normalize"] == c["normalize"] and not d["table"] and "k_istft_mfft_direct" in d["kernels"], d["line"]
        assert d["line"].startswith("istft mfft direct ")


# schedule, spans per workgroup, columns per lane of the issue's table of cases
PLANS = {
    "n18-l13": ("3x3", 64, 5), "n20-one-span-raw": ("5x2", 64, 5), "n30-l24-short": ("5x3", 64, 8), "n50-hop4-few": ("5x5", 32, 7),
    "n54-l40-padded-long": ("3x3x3", 32, 7), "n96-nocenter-form1": ("3x4x4", 16, 6), "n250-l100-hop300": ("5x5x5", 8, 8),
    "n400": ("5x5x4x2", 4, 7), "n480-l400-raw": ("5x3x4x4", 4, 8), "n1000-raw": ("5x5x5x4", 2, 8), "n1200-nocenter": ("5x5x3x4x2", 1, 5),
    "n1200-hop8-heavy": ("5x5x3x4x2", 1, 5), "n1536": ("3x4x4x4x4", 1, 6), "n2560-l100-loop": ("5x4x4x4x4", 1, 10),
    "n4000": ("5x5x5x4x4", 1, 16), "n4050": ("5x5x3x3x3x3", 1, 16), "bench-64x998x201": ("5x5x4x2", 4, 7),
}


def test_the_plans_of_the_cases():
    assert set(PLANS) == set(XC.case_ids())
    for cid, want in PLANS.items():
        d = XC.parse(XC.line(XC.case(cid)))
        assert (d["schedule"], d["fy"], d["cpl"]) == want, d["line"]
    d = XC.parse(XC.line(XC.case("n18-l13")))
    assert (d["spans"], d["S"], d["halo"]) == (3, 8, 2), d["line"]
    d = XC.parse(XC.line(XC.case("n50-hop4-few")))
    assert (d["S"], d["halo"]) == (6, 12), d["line"]
    d = XC.parse(XC.line(XC.case("n400")))
    assert (d["spans"], d["S"], d["halo"], d["lds"]) == (4, 8, 2, 16000), d["line"]
    d = XC.parse(XC.line(XC.case("n1200-hop8-heavy")))
    assert (d["S"], d["halo"], d["groups"], d["heavy"]) == (596, 149, 2, True), d["line"]
    d = XC.parse(XC.line(XC.case("n2560-l100-loop")))
    assert (d["groups"], d["grid"]) == (2052, 2048), d["line"]
    d = XC.parse(XC.line(XC.case("n4050")))
    assert d["lds"] == 64800, d["line"]
    d = XC.parse(XC.line(XC.case("bench-64x998x201")))
    assert (d["S"], d["groups"]) == (15, 1072), d["line"]


def _sweep(sizes):
    for n in sizes:
        for L in (1, 13, n // 2 + 1, n):
            for hop in (1, 7, n // 4 + 3, n + 5):
                for nb in (1, 3, 64):
                    for F in (1, 2, 65, 2049):
                        yield n, L, hop, nb, F


def test_the_planner_emits_no_shape_without_a_case():
    """The lane layout and the schedule are functions of n_fft alone; L, hop, the batch and the frames set S, the spans, the groups and
    the grid.  For every n_fft the checks accept, against windows, hops, batches and frame counts at the edges: every pass shape, the
    lane / column layout, the slots and the columns per lane are ones a case has; the LDS follows the contract's formula; S is at
    least four halos unless the frames run out, the spans cover the outputs, the groups cover the spans and the grid is
    min(groups, 2048)."""
    p = XC.params(4)
    parsed = [XC.parse(XC.line(c)) for c in XC.CASES]
    passes = set().union(*(XC.pass_shapes(d) for d in parsed))
    layouts = {XC.layout(d) for d in parsed}
    slots = {d["fy"] for d in parsed}
    seen_passes, seen_layouts, seen_slots, worst_cpl, worst_lds = set(), set(), set(), 0, 0
    for n, L, hop, nb, F in _sweep(SUPPORTED):
        pad, col0 = n // 2, (n - L) // 2
        T = n + hop * (F - 1) - 2 * pad
        if T < 1:
            continue
        s = B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, shift=31)
        d = XC.parse(B.describe_istft_mfft(p, L, s, normalize=True))
        M, lpf = n // 2, d["lpf"]
        assert XC.pass_shapes(d) <= passes, (sorted(XC.pass_shapes(d) - passes), d["line"])
        assert XC.layout(d) in layouts and d["fy"] in slots, d["line"]
        assert d["m"] == M and lpf * d["fy"] == 256 and lpf & (lpf - 1) == 0 and 4 <= lpf <= 256
        assert (4 * lpf >= M or lpf == 256) and (lpf == 4 or 2 * lpf < M), d["line"]
        assert d["cpl"] == -(-n // lpf) <= 16
        assert d["lds"] == 2 * d["fy"] * M * 8 + M * 8 + n * 4 <= 65536
        r = d["radices"]
        assert r == sorted(r, key=(5, 3, 4, 2).index) and r.count(2) <= 1, d["line"]
        end, heff = d["t0"] + T, min(hop, d["t0"] + T)
        assert d["halo"] == -(-L // heff) - 1
        assert 1 <= d["S"] <= F and (d["S"] >= XC.HALO_FACTOR * d["halo"] or d["S"] == min(F, -(-end // heff))), d["line"]
        assert d["spans"] == -(-end // (d["S"] * heff))
        assert d["groups"] == -(-nb * d["spans"] // d["fy"]) and d["grid"] == min(d["groups"], XC.MAX_GRID)
        assert d["trips"] == min(d["S"] + d["halo"], F)
        assert d["repeated"] <= 100 // (XC.HALO_FACTOR + 1) or d["S"] < XC.HALO_FACTOR * d["halo"], d["line"]
        seen_passes |= XC.pass_shapes(d)
        seen_layouts.add(XC.layout(d))
        seen_slots.add(d["fy"])
        worst_cpl, worst_lds = max(worst_cpl, d["cpl"]), max(worst_lds, d["lds"])
    assert seen_passes == passes and seen_layouts == layouts and seen_slots == slots   # no case is of a shape the planner would not emit
    assert worst_cpl == 16 and worst_lds == 64800                   # n_fft 4050


def _reaching(L, hop, F, wlo, whi):
    """The frames f < F whose window [f * hop, f * hop + L) meets [wlo, whi), by the definition."""
    return [f for f in range(F) if f * hop < whi and f * hop + L > wlo]


@pytest.mark.parametrize("cid", [c["id"] for c in XC.CASES if c["B"] * c["F"] <= 4096])
def test_every_spans_frame_list_is_the_frames_that_reach_it(cid):
    c = XC.case(cid)
    d = XC.parse(XC.line(c))
    T = XC.geometry(c)[4]
    covered_to = d["t0"]
    for s in range(d["spans"]):
        wlo, whi, f_lo, f_hi = XC.span_frames(d, c["hop"], c["F"], T, s)
        assert wlo == covered_to or whi == wlo, (s, wlo, covered_to)
        covered_to = max(covered_to, whi)
        want = _reaching(c["L"], c["hop"], c["F"], wlo, whi) if whi > wlo else []
        assert list(range(f_lo, f_hi)) == want, (cid, s, f_lo, f_hi, want[:3], want[-3:])
        assert f_hi - f_lo <= d["trips"]
    assert covered_to == d["t0"] + T                 # the spans' outputs are the signal's, each once


def test_span_frame_lists_over_a_grid_of_shapes():
    p = XC.params(4)
    done = 0
    for n, L, hop, nb, F in _sweep((18, 20, 30, 50, 54, 96, 250)):
        if nb > 1:
            continue
        pad, col0 = n // 2, (n - L) // 2
        for extra in (0, -1, n + 2 * hop + 3):
            T = n + hop * (F - 1) - 2 * pad + extra
            if T < 1:
                continue
            d = XC.parse(B.describe_istft_mfft(p, L, B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, shift=31)))
            if d["spans"] > 300:
                continue
            for s in range(d["spans"]):
                wlo, whi, f_lo, f_hi = XC.span_frames(d, hop, F, T, s)
                lo = max(0, (wlo - L) // hop - 1)
                want = [f for f in range(lo, min(F, whi // hop + 2)) if f * hop < whi and f * hop + L > wlo] if whi > wlo else []
                assert list(range(f_lo, f_hi)) == want, (n, L, hop, F, extra, s)
                assert f_hi - f_lo <= d["trips"]
            done += 1
    assert done > 200


def test_the_printed_schedules():
    p = XC.params(4)
    for n, want in ((400, "5x5x4x2"), (480, "5x3x4x4"), (18, "3x3"), (4050, "5x5x3x3x3x3"), (20, "5x2"), (30, "5x3"), (50, "5x5"), (96, "3x4x4"),
                    (1000, "5x5x5x4"), (1200, "5x5x3x4x2"), (1536, "3x4x4x4x4"), (4000, "5x5x5x4x4"), (2916, "3x3x3x3x3x3x2")):
        d = XC.parse(B.describe_istft_mfft(p, 16, B.make_stft(2, 1000, 5, 7, n, col0=(n - 16) // 2, pad=n // 2, shift=31)))
        assert d["schedule"] == want, d["line"]


def test_unsupported_sizes_have_no_plan():
    p = XC.params(4)
    for n in (14, 15, 45, 28, 22, 4374, 4500, 512, 4096):
        with pytest.raises(B.BhwError) as e:
            B.describe_istft_mfft(p, 8, B.make_stft(1, 1000, 3, 7, n, col0=(n - 8) // 2, pad=n // 2, shift=31))
        assert e.value.code == -2, e.value                 # BHW_ERR_UNSUPPORTED
    with pytest.raises(B.BhwError) as e:                   # a power of two has calls of its own
        B.describe_istft_mfft(p, 8, B.make_stft(1, 1000, 3, 7, 512, col0=252, pad=256, shift=31))
    assert e.value.code == -2 and "bhw_istft_fft_f32_" in e.value.detail
