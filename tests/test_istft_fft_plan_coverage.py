"""The case table of tests/istft_fft_cases.py reaches every plan class of the fused inverse FFT + overlap-add front: every class has a
case, every claim holds on the describe line of its case (host arithmetic, no GPU), a sweep of the planner over every supported n_fft
and a grid of (L, hop, B, F) emits no shape -- radix schedule, spans per workgroup, lanes per row, columns per lane, LDS bytes -- that
the table's cases do not hold, and the frame list of every span, taken from the plan's S, is exactly the frames that reach the span's
outputs."""
import pytest

from blackman_harris_win_amd import binding as B

import istft_fft_cases as IC

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
    """... and the describe line of every case restates the case's own shape, library form."""
    ids = IC.case_ids()
    assert len(set(ids)) == len(ids), ids
    for c in IC.CASES:
        assert c["classes"], c["id"]
        L, col0, pad, _, _ = IC.geometry(c)
        d = IC.parse(IC.line(c))
        assert (d["signals"], d["frames"], d["n_fft"], d["L"], d["col0"], d["pad"]) == (c["B"], c["F"], c["n_fft"], L, col0, pad), d["line"]
        assert d["normalize"] == c["normalize"] and not d["table"] and "k_istft_fft_direct" in d["kernels"], d["line"]


def _shape(d):
    return (d["n_fft"], d["schedule"], d["lpf"], d["fy"], d["cpl"], d["lds"])


def _sweep():
    for lg in range(4, 13):
        n = 1 << lg
        for L in (1, 13, n // 2 + 1, n):
            for hop in (1, 7, n // 4, n // 4 + 3, n + 5):
                for nb in (1, 3, 64):
                    for F in (1, 2, 65, 2049, 40000):
                        if nb * F * n > 1 << 34:
                            continue
                        yield n, L, hop, nb, F


def test_the_planner_emits_no_shape_without_a_case():
    """The lane layout is a function of n_fft alone; L, hop, the batch and the frames set S, the spans, the groups and the grid.  For
    every n_fft the checks accept, against windows, hops, batches and frame counts at the edges: the shape is one a case has, S is
    at least four halos unless the frames run out, the spans cover the outputs, the groups cover the spans and the grid is
    min(groups, 2048)."""
    p = IC.params(4)
    covered = {_shape(IC.parse(IC.line(c))) for c in IC.CASES}
    seen = set()
    for n, L, hop, nb, F in _sweep():
        pad, col0 = n // 2, (n - L) // 2
        T = n + hop * (F - 1) - 2 * pad
        if T < 1:
            continue
        s = B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, shift=31)
        d = IC.parse(B.describe_istft_fft(p, L, s, normalize=True))
        assert _shape(d) in covered, d["line"]
        assert d["schedule"] == IC.SCHEDULES[n] and d["m"] == n // 2 and d["lpf"] * d["fy"] == 256 and d["lpf"] * d["cpl"] == n
        assert d["lds"] == 2 * d["fy"] * d["m"] * 8 + d["m"] * 8 + n * 4 <= 65536
        end, heff = d["t0"] + T, min(hop, d["t0"] + T)
        assert d["halo"] == -(-L // heff) - 1
        assert 1 <= d["S"] <= F and (d["S"] >= IC.HALO_FACTOR * d["halo"] or d["S"] == min(F, -(-end // heff))), d["line"]
        assert d["spans"] == -(-end // (d["S"] * heff))
        assert d["groups"] == -(-nb * d["spans"] // d["fy"]) and d["grid"] == min(d["groups"], IC.MAX_GRID)
        assert d["trips"] == min(d["S"] + d["halo"], F)
        assert d["repeated"] <= 100 // (IC.HALO_FACTOR + 1) or d["S"] < IC.HALO_FACTOR * d["halo"], d["line"]
        seen.add(_shape(d))
    assert seen == covered                          # and no case is of a shape the planner would not emit


def _reaching(L, hop, F, wlo, whi):
    """The frames f < F whose window [f * hop, f * hop + L) meets [wlo, whi), by the definition."""
    return [f for f in range(F) if f * hop < whi and f * hop + L > wlo]


@pytest.mark.parametrize("cid", [c["id"] for c in IC.CASES if c["B"] * c["F"] <= 4096])
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
        if F > 2049 or nb > 1 or n > 256:
            continue
        pad, col0 = n // 2, (n - L) // 2
        for extra in (0, -1, n + 2 * hop + 3):
            T = n + hop * (F - 1) - 2 * pad + extra
            if T < 1:
                continue
            d = IC.parse(B.describe_istft_fft(p, L, B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, shift=31)))
            if d["spans"] > 300:
                continue
            for s in range(d["spans"]):
                wlo, whi, f_lo, f_hi = IC.span_frames(d, hop, F, T, s)
                lo = max(0, (wlo - L) // hop - 1)
                want = [f for f in range(lo, min(F, whi // hop + 2)) if f * hop < whi and f * hop + L > wlo] if whi > wlo else []
                assert list(range(f_lo, f_hi)) == want, (n, L, hop, F, extra, s)
                assert f_hi - f_lo <= d["trips"]
            done += 1
    assert done > 200


def test_unsupported_sizes_have_no_plan():
    p = IC.params(4)
    for n in (8, 15, 17, 100, 8192):
        with pytest.raises(B.BhwError) as e:
            B.describe_istft_fft(p, min(n, 8), B.make_stft(1, 1000, 3, 7, n, pad=n // 2, shift=31))
        assert e.value.code == -2, e.value                 # BHW_ERR_UNSUPPORTED
