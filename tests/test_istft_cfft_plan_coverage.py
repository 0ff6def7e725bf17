"""The case table of tests/istft_cfft_cases.py reaches every plan class of the fused inverse complex FFT + overlap-add front: every
class has a case, every claim holds on the describe line of its case (host arithmetic, no GPU), a sweep of the planner over every
supported n_fft, all four flag combinations and a grid of (L, hop, B, F) emits no shape -- radix schedule, spans per workgroup, lanes
per row, columns per lane, LDS bytes -- that the table's cases do not hold, the lanes, slots and passes are those of
bhwp_stft_cfft_plan for the same n_fft, and the frame list of every span, taken from the plan's S, is exactly the frames that reach the
span's outputs."""
import pytest

from blackman_harris_win_amd import binding as B

import istft_cfft_cases as IC
import stft_cfft_cases as FC

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
        assert d["normalize"] == c["normalize"] and not d["table"] and "k_istft_cfft_direct" in d["kernels"], d["line"]
        assert d["shifted"] == bool(c.get("fftshift")) and d["in_order"] != d["shifted"], d["line"]
        assert d["line"].startswith("istft cfft direct"), d["line"]


def test_the_grid_target_case_is_the_smallest_of_its_kind():
    """One frame, one signal or one halo less and the halo, not the grid target, would set S."""
    c = IC.case("n1024-grid-target")
    d = IC.parse(IC.line(c))
    assert (d["fy"], d["halo"], d["S"]) == (1, 1, 5) and d["groups"] >= IC.TARGET_GROUPS, d["line"]
    assert c["B"] * c["F"] // (IC.TARGET_GROUPS * d["fy"]) == IC.HALO_FACTOR * d["halo"] + 1


def _shape(d):
    return (d["n_fft"], d["schedule"], d["lpf"], d["fy"], d["cpl"], d["lds"])


def _sweep():
    for lg in range(4, 12):
        n = 1 << lg
        for L in (1, 13, n // 2 + 1, n):
            for hop in (1, 7, n // 4, n // 4 + 3, n + 5):
                for nb in (1, 3, 64):
                    for F in (1, 2, 65, 2049, 40000):
                        if nb * F * n > 1 << 34:
                            continue
                        yield n, L, hop, nb, F


def test_the_planner_emits_no_shape_without_a_case():
    """The lane layout is a function of n_fft alone; L, hop, the batch and the frames set S, the spans, the groups and the grid; the
    flags change neither.  For every n_fft the checks accept and all four flag combinations, against windows, hops, batches and frame
    counts at the edges: the shape is one a case has, S is at least four halos unless the frames run out, the spans cover the
    outputs, the groups cover the spans and the grid is min(groups, 2048)."""
    p = IC.params(4)
    covered = {_shape(IC.parse(IC.line(c))) for c in IC.CASES}
    seen = set()
    for n, L, hop, nb, F in _sweep():
        pad, col0 = n // 2, (n - L) // 2
        T = n + hop * (F - 1) - 2 * pad
        if T < 1:
            continue
        s = B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, channels=2, shift=31)
        lines = [B.describe_istft_cfft(p, L, s, normalize=nz, fftshift=sh) for nz in (False, True) for sh in (False, True)]
        shapes = {_shape(IC.parse(ln)) for ln in lines}
        plans = {ln[ln.index("signals x"):] for ln in lines}
        assert len(shapes) == 1 and len(plans) == 1, lines
        d = IC.parse(lines[3])
        assert d["normalize"] and d["shifted"]
        assert _shape(d) in covered, d["line"]
        assert d["schedule"] == IC.SCHEDULES[n] and d["m"] == n and d["lpf"] * d["fy"] == 256 and d["lpf"] * d["cpl"] == n
        assert d["lds"] == 2 * d["fy"] * n * 8 + n // 2 * 8 + n * 4 <= 48 * 1024
        end, heff = d["t0"] + T, min(hop, d["t0"] + T)
        assert d["halo"] == -(-L // heff) - 1
        assert 1 <= d["S"] <= F and (d["S"] >= IC.HALO_FACTOR * d["halo"] or d["S"] == min(F, -(-end // heff))), d["line"]
        assert d["spans"] == -(-end // (d["S"] * heff))
        assert d["groups"] == -(-nb * d["spans"] // d["fy"]) and d["grid"] == min(d["groups"], IC.MAX_GRID)
        assert d["trips"] == min(d["S"] + d["halo"], F)
        assert d["repeated"] <= 100 // (IC.HALO_FACTOR + 1) or d["S"] < IC.HALO_FACTOR * d["halo"], d["line"]
        seen.add(_shape(d))
    assert seen == covered                          # and no case is of a shape the planner would not emit


@pytest.mark.parametrize("n", sorted(IC.SCHEDULES))
def test_lanes_slots_and_passes_are_the_forward_plans(n):
    """lpf = min(256, max(4, n / 4)), fy = 256 / lpf, cpl = n / lpf and the radix schedule: those of bhwp_stft_cfft_plan."""
    p = IC.params(4)
    fwd = FC.parse(B.describe_stft_cfft(p, n, B.make_stft(2, 10 * n, 19, n // 2, n, pad=n // 2, channels=2, shift=31)))
    inv = IC.parse(B.describe_istft_cfft(p, n, B.make_stft(2, 9 * n, 19, n // 2, n, pad=n // 2, channels=2, shift=31)))
    assert (inv["lpf"], inv["fy"], inv["cpl"], inv["schedule"], inv["m"]) == (fwd["lpf"], fwd["fy"], fwd["cpl"], fwd["schedule"], fwd["m"])
    assert inv["lpf"] == min(256, max(4, n // 4)) and inv["cpl"] in (4, 8)


def _reaching(L, hop, F, wlo, whi):
    """The frames f < F whose window [f * hop, f * hop + L) meets [wlo, whi), by the definition."""
    return [f for f in range(F) if f * hop < whi and f * hop + L > wlo]


@pytest.mark.parametrize("cid", [c["id"] for c in IC.CASES if c["B"] * c["F"] <= 8192])
def test_every_spans_frame_list_is_the_frames_that_reach_it(cid):
    c = IC.case(cid)
    d = IC.parse(IC.line(c))
    T = IC.geometry(c)[4]
    covered_to = d["t0"]
    for s in range(d["spans"]):
        wlo, whi, f_lo, f_hi = IC.span_frames(d, c["hop"], c["F"], T, s)
        assert wlo == covered_to or whi == wlo, (s, wlo, covered_to)
        covered_to = max(covered_to, whi)
        lo = max(0, (wlo - c["L"]) // c["hop"] - 1)
        want = [f for f in range(lo, min(c["F"], whi // c["hop"] + 2)) if f * c["hop"] < whi and f * c["hop"] + c["L"] > wlo] if whi > wlo else []
        assert list(range(f_lo, f_hi)) == want, (cid, s, f_lo, f_hi, want[:3], want[-3:])
        if s % 97 == 0:
            assert want == (_reaching(c["L"], c["hop"], c["F"], wlo, whi) if whi > wlo else [])
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
            d = IC.parse(B.describe_istft_cfft(p, L, B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, channels=2, shift=31)))
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
    for n in (8, 15, 17, 100, 4096, 8192):
        with pytest.raises(B.BhwError) as e:
            B.describe_istft_cfft(p, min(n, 8), B.make_stft(1, 1000, 3, 7, n, pad=n // 2, channels=2, shift=31))
        assert e.value.code == -2, e.value                 # BHW_ERR_UNSUPPORTED
