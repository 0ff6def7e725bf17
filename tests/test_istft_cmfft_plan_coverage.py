"""The case table of tests/istft_cmfft_cases.py reaches every plan class of the fused inverse mixed-radix complex FFT + overlap-add
front: every class has a case, every claim holds on the describe line of its case (host arithmetic, no GPU), a sweep of the planner
over all 91 supported n_fft, all four flag combinations and a grid of (L, hop, B, F) emits no pass shape, row layout or slot count that
the table's cases do not hold, the lanes, slots, passes and twiddle entries are those of bhwp_stft_cmfft_plan for the same n_fft,
cpl <= 8 and LDS <= 56 700 everywhere, and the frame list of every span, taken from the plan's S, is exactly the frames that reach the
span's outputs."""
import pytest

from blackman_harris_win_amd import binding as B

import istft_cmfft_cases as IC
import stft_cmfft_cases as FC

CLAIMS = [(c["id"], name) for c in IC.CASES for name in c["classes"]]


@pytest.mark.parametrize("name", list(IC.CLASSES))
def test_every_class_has_a_case(name):
    claimed = [c for c in IC.CASES if name in c["classes"]]
    assert claimed, f"no case claims the class {name!r}"
    for c in claimed:
        line = IC.line(c)
        assert IC.CLASSES[name](c, IC.parse(line)), f"case {c['id']} is not of the class {name!r}: {line}"


@pytest.mark.parametrize("cid,name", CLAIMS, ids=[f"{c}: {n}" for c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(cid, name):
    assert name in IC.CLASSES, f"case {cid} claims {name!r}, which is no class"
    c = IC.case(cid)
    line = IC.line(c)
    assert IC.CLASSES[name](c, IC.parse(line)), f"case {cid} is not of the class {name!r}: {line}"


def test_case_ids_are_unique_and_every_case_is_there_for_a_class():
    """... the describe line of every case restates the case's own shape, library form, and no case is more than a few thousand rows."""
    ids = IC.case_ids()
    assert len(set(ids)) == len(ids), ids
    for c in IC.CASES:
        assert c["classes"], c["id"]
        assert 50 <= c["B"] * c["F"] <= 4096, c["id"]       # enough rows for the GPU test's ratio gate, and no more than a few thousand
        L, col0, pad, _, _ = IC.geometry(c)
        d = IC.parse(IC.line(c))
        assert (d["signals"], d["frames"], d["n_fft"], d["L"], d["col0"], d["pad"]) == (c["B"], c["F"], c["n_fft"], L, col0, pad), d["line"]
        assert d["normalize"] == c["normalize"] and not d["table"] and "k_istft_cmfft_direct" in d["kernels"], d["line"]
        assert d["shifted"] == bool(c.get("fftshift")) and d["in_order"] != d["shifted"], d["line"]
        assert d["line"].startswith("istft cmfft direct"), d["line"]


def _shape(d):
    """What the kernel branches on beyond the spans: the pass shapes, the row layout and the slots of a workgroup."""
    return (frozenset(IC.pass_shapes(d)), IC.layout(d), min(d["fy"], 2))


def _sweep():
    for n in IC.SIZES:
        for L in (1, 13, n // 2 + 1, n):
            for hop in (1, 7, n // 4, n // 4 + 3, n + 5):
                for nb in (1, 3, 64):
                    for F in (1, 2, 65, 2049):
                        yield n, L, hop, nb, F


def test_the_planner_emits_no_shape_without_a_case():
    """The lane layout is a function of n_fft alone; L, hop, the batch and the frames set S, the spans, the groups and the grid; the
    flags change neither.  For all 91 n_fft and all four flag combinations, against windows, hops, batches and frame counts at the
    edges: every pass shape and every layout is one a case has, S is at least four halos unless the frames run out, the spans cover
    the outputs, the groups cover the spans and the grid is min(groups, 2048)."""
    p = IC.params(4)
    parsed = [IC.parse(IC.line(c)) for c in IC.CASES]
    passes = set().union(*(IC.pass_shapes(d) for d in parsed))
    layouts = {IC.layout(d) for d in parsed}
    slots = {min(d["fy"], 2) for d in parsed}
    assert len(IC.SIZES) == 91
    for n, L, hop, nb, F in _sweep():
        pad, col0 = n // 2, (n - L) // 2
        T = n + hop * (F - 1) - 2 * pad
        if T < 1:
            continue
        s = B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, channels=2, shift=31)
        lines = [B.describe_istft_cmfft(p, L, s, normalize=nz, fftshift=sh) for nz in (False, True) for sh in (False, True)]
        plans = {ln[ln.index("signals x"):] for ln in lines}
        assert len(plans) == 1, lines
        d = IC.parse(lines[3])
        assert d["normalize"] and d["shifted"]
        assert IC.pass_shapes(d) <= passes, (sorted(IC.pass_shapes(d) - passes), d["line"])
        assert IC.layout(d) in layouts and min(d["fy"], 2) in slots, d["line"]
        fold = n if n % 2 else n // 2
        assert d["m"] == n and d["lpf"] * d["fy"] == 256 and d["cpl"] == -(-n // d["lpf"]) and 3 <= d["cpl"] <= 8 and d["fold"] == fold
        assert d["lds"] == 2 * d["fy"] * n * 8 + fold * 8 + n * 4 <= 56700
        end, heff = d["t0"] + T, min(hop, d["t0"] + T)
        assert d["halo"] == -(-L // heff) - 1
        assert 1 <= d["S"] <= F and (d["S"] >= IC.HALO_FACTOR * d["halo"] or d["S"] == min(F, -(-end // heff))), d["line"]
        assert d["spans"] == -(-end // (d["S"] * heff))
        assert d["groups"] == -(-nb * d["spans"] // d["fy"]) and d["grid"] == min(d["groups"], IC.MAX_GRID)
        assert d["trips"] == min(d["S"] + d["halo"], F)


def test_lds_at_the_two_largest_sizes():
    p = IC.params(4)
    for n, lds in ((2000, 48000), (2025, 56700)):
        d = IC.parse(B.describe_istft_cmfft(p, n, B.make_stft(2, 9 * n, 19, n // 2, n, pad=n // 2, channels=2, shift=31)))
        assert d["lds"] == lds, d["line"]


@pytest.mark.parametrize("n", IC.SIZES)
def test_lanes_slots_passes_and_twiddles_are_the_forward_plans(n):
    p = IC.params(4)
    fwd = FC.parse(B.describe_stft_cmfft(p, n, B.make_stft(2, 10 * n, 19, n // 2, n, pad=n // 2, channels=2, shift=31)))
    inv = IC.parse(B.describe_istft_cmfft(p, n, B.make_stft(2, 9 * n, 19, n // 2, n, pad=n // 2, channels=2, shift=31)))
    for k in ("lpf", "fy", "cpl", "schedule", "m", "fold"):
        assert inv[k] == fwd[k], (k, inv["line"], fwd["line"])


def _reaching(L, hop, F, wlo, whi):
    """The frames f < F whose window [f * hop, f * hop + L) meets [wlo, whi), by the definition."""
    return [f for f in range(F) if f * hop < whi and f * hop + L > wlo]


@pytest.mark.parametrize("cid", IC.case_ids())
def test_every_spans_frame_list_is_the_frames_that_reach_it(cid):
    c = IC.case(cid)
    d = IC.parse(IC.line(c))
    T = IC.geometry(c)[4]
    covered_to = d["t0"]
    for s in range(d["spans"]):
        wlo, whi, f_lo, f_hi = IC.span_frames(d, c["hop"], c["F"], T, s)
        assert wlo == covered_to or whi == wlo, (s, wlo, covered_to)
        covered_to = max(covered_to, whi)
        want = _reaching(c["L"], c["hop"], c["F"], wlo, whi) if whi > wlo else []
        assert list(range(f_lo, f_hi)) == want, (cid, s, f_lo, f_hi, want[:3], want[-3:])
        assert f_hi - f_lo <= d["trips"]
    assert covered_to == d["t0"] + T                 # the spans' outputs are the signal's, each once


def test_span_frame_lists_over_a_grid_of_shapes():
    p = IC.params(4)
    done = 0
    for n, L, hop, nb, F in _sweep():
        if nb > 1 or n > 100 or F > 65:
            continue
        pad, col0 = n // 2, (n - L) // 2
        for extra in (0, -1, n + 2 * hop + 3):
            T = n + hop * (F - 1) - 2 * pad + extra
            if T < 1:
                continue
            d = IC.parse(B.describe_istft_cmfft(p, L, B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, channels=2, shift=31)))
            for s in range(d["spans"]):
                wlo, whi, f_lo, f_hi = IC.span_frames(d, hop, F, T, s)
                want = _reaching(L, hop, F, wlo, whi) if whi > wlo else []
                assert list(range(f_lo, f_hi)) == want, (n, L, hop, F, extra, s)
                assert f_hi - f_lo <= d["trips"]
            done += 1
    assert done > 200


def test_unsupported_sizes_have_no_plan():
    p = IC.params(4)
    for n in (8, 15, 17, 512, 700, 2048, 2160, 4050):
        with pytest.raises(B.BhwError) as e:
            B.describe_istft_cmfft(p, min(n, 8), B.make_stft(1, 1000, 3, 7, n, pad=n // 2, channels=2, shift=31))
        assert e.value.code == -2, e.value                 # BHW_ERR_UNSUPPORTED
