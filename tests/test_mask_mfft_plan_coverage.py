"""The case table of tests/mask_mfft_cases.py reaches every plan class of the mixed-radix fused STFT + mask + inverse STFT front: every
class has a case, every claim holds on the describe line of its case (host arithmetic, no GPU), a sweep of the planner over all 73
supported n_fft emits no pass shape, lane / column layout or slot count the table lacks, every plan field of the line is
describe_istft_mfft's for the same synthesis descriptor but for the LDS bytes, which hold a second twiddle table, and everywhere a lane
has at most 8 columns and the workgroup at most 40 000 bytes of LDS."""
import pytest

from blackman_harris_win_amd import binding as B

import istft_mfft_cases as XC
import mask_mfft_cases as MM

CLAIMS = [(c["id"], name) for c in MM.CASES for name in c["classes"]]
PLAN_FIELDS = ("signals", "frames", "rows", "n_fft", "m", "lpf", "fy", "cpl", "S", "halo", "spans", "trips", "repeated", "groups", "grid",
               "L", "col0", "pad", "t0", "schedule", "normalize", "heavy")


@pytest.mark.parametrize("name", list(MM.CLASSES))
def test_every_class_has_a_case(name):
    claimed = [c for c in MM.CASES if name in c["classes"]]
    assert claimed, f"no case claims the class {name!r}"
    for c in claimed:
        line = MM.line(c)
        assert MM.CLASSES[name](c, MM.parse(line)), f"case {c['id']} is not of the class {name!r}: {line}"


@pytest.mark.parametrize("cid,name", CLAIMS, ids=[f"{c}: {n}" for c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(cid, name):
    assert name in MM.CLASSES, f"case {cid} claims {name!r}, which is no class"
    c = MM.case(cid)
    line = MM.line(c)
    assert MM.CLASSES[name](c, MM.parse(line)), f"case {cid} is not of the class {name!r}: {line}"


def test_the_sizes_are_the_73_below_2048():
    assert len(MM.SIZES) == 73 and MM.SIZES[0] == 18 and MM.SIZES[-1] == 2000
    assert len([n for n in range(1, 5001) if B.mfft_supported(n)]) == 95
    assert [n for n in MM.SIZES if (n // 2) % 2][:8] == [18, 30, 50, 54, 90, 150, 162, 250]
    assert len([n for n in MM.SIZES if (n // 2) % 2]) == 16
    assert all(B.mask_mfft_supported(n) for n in MM.SIZES)
    assert not any(B.mask_mfft_supported(n) for n in (16, 512, 2048, 2160, 2560, 4000, 4050, 4096, 22, 19))


def test_the_cases_are_the_inverse_cases_below_2048_with_every_padding_mode_and_gain_layout():
    want = [c["id"] for c in XC.CASES if c["n_fft"] < 2048]
    want.insert(want.index("bench-64x998x201"), "n1500-l100-loop")          # in the place of n2560-l100-loop
    assert MM.case_ids() == want
    assert {c["id"] for c in XC.CASES} - set(MM.case_ids()) == {"n2560-l100-loop", "n4000", "n4050"}
    # a class of the parent is here, or dropped by name with its reason
    assert set(XC.CLASSES) - set(MM.CLASSES) == set(MM.DROPPED) - {"direct form 1", "direct form 2"}
    assert all(MM.DROPPED.values())
    assert {c["pad_mode"] for c in MM.CASES} == {"reflect", "constant"}
    assert any(not c["center"] for c in MM.CASES)
    assert {c["gains"] for c in MM.CASES} == set(MM.LAYOUTS)
    assert any(c["gains"] == "padded" and c.get("padded") for c in MM.CASES)
    ids = MM.case_ids()
    assert len(set(ids)) == len(ids)
    for c in MM.CASES:
        assert c["classes"], c["id"]
        L, col0, pad, Tin, _ = MM.geometry(c)
        d = MM.parse(MM.line(c))
        assert (d["signals"], d["frames"], d["n_fft"], d["L"], d["col0"], d["pad"]) == (c["B"], c["F"], c["n_fft"], L, col0, pad), d["line"]
        assert (d["T_in"], d["pad_in"], d["pad_mode"]) == (Tin, pad, c["pad_mode"]), d["line"]
        assert d["normalize"] == c["normalize"] and not d["table"] and list(d["kernels"]) == ["k_mask_mfft_direct"] and d["both_ffts"], d["line"]
        assert d["line"].startswith("mask mfft direct ")
        # the analysis input gives exactly the case's frames
        assert 1 + (Tin + 2 * pad - c["n_fft"]) // c["hop"] == c["F"]


def test_the_group_loop_case():
    d = MM.parse(MM.line(MM.case("n1500-l100-loop")))
    assert d["fy"] == 1 and d["groups"] > d["grid"] == XC.MAX_GRID, d["line"]


def _lds(d):
    return 2 * d["fy"] * d["m"] * 8 + 2 * d["m"] * 8 + d["n_fft"] * 4


@pytest.mark.parametrize("cid", MM.case_ids())
def test_every_plan_field_is_the_inverse_calls(cid):
    c = MM.case(cid)
    sa, ss, L, _, _, gs, gbs = MM.desc(c)
    p = MM.params(c["setup"])
    d = MM.parse(MM.line(c))
    parent = XC.parse(B.describe_istft_mfft(p, L, ss, normalize=c["normalize"]))
    for name in PLAN_FIELDS:
        assert d[name] == parent[name], (cid, name, d["line"], parent["line"])
    assert d["lds"] == _lds(d) == parent["lds"] + d["m"] * 8 and d["lds"] <= 40000 and d["cpl"] <= 8


def _sweep():
    for n in MM.SIZES:
        for L in (1, 13, n // 2 + 1, n):
            for hop in (1, 7, n // 4 + 3, n + 5):
                for nb in (1, 3, 64):
                    for F in (1, 2, 65, 2049):
                        yield n, L, hop, nb, F


def test_the_planner_emits_no_shape_without_a_case():
    """For every n_fft the checks accept, against windows, hops, batches and frame counts at the edges, with zero padding on the analysis
    side (reflection needs pad < T): every pass shape, lane / column layout and slot count is one a case has, every plan field is the
    inverse call's, a lane has at most 8 columns and the LDS is at most 40 000 bytes (reached at 2000)."""
    p = MM.params(4)
    parsed = [MM.parse(MM.line(c)) for c in MM.CASES]
    passes = set().union(*(MM.pass_shapes(d) for d in parsed))
    layouts = {MM.layout(d) for d in parsed}
    slots = {d["fy"] for d in parsed}
    seen_passes, seen_layouts, seen_slots, worst_cpl, worst_lds = set(), set(), set(), 0, (0, 0)
    for n, L, hop, nb, F in _sweep():
        pad, col0 = n // 2, (n - L) // 2
        T = n + hop * (F - 1) - 2 * pad
        if T < 1:
            continue
        sa = B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, pad_mode=0, shift=31)
        ss = B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, shift=31)
        d = MM.parse(B.describe_mask_mfft(p, L, sa, ss, normalize=True))
        parent = XC.parse(B.describe_istft_mfft(p, L, ss, normalize=True))
        assert MM.pass_shapes(d) <= passes, (sorted(MM.pass_shapes(d) - passes), d["line"])
        assert MM.layout(d) in layouts and d["fy"] in slots, d["line"]
        for name in PLAN_FIELDS:
            assert d[name] == parent[name], (name, d["line"], parent["line"])
        assert 8 * d["lpf"] >= n and d["cpl"] <= 8, d["line"]
        assert d["lds"] == _lds(d) <= 40000, d["line"]
        seen_passes |= MM.pass_shapes(d)
        seen_layouts.add(MM.layout(d))
        seen_slots.add(d["fy"])
        worst_cpl, worst_lds = max(worst_cpl, d["cpl"]), max(worst_lds, (d["lds"], n))
    assert seen_passes == passes and seen_layouts == layouts and seen_slots == slots   # no case is of a shape the planner would not emit
    assert worst_cpl == 8 and worst_lds == (40000, 2000)


def test_unsupported_sizes_have_no_plan():
    p = MM.params(4)
    for n in (14, 15, 22, 45, 512, 2048, 2160, 2560, 4000, 4050, 4096, 4374, 8192):
        with pytest.raises(B.BhwError) as e:
            s = B.make_stft(1, 10000, 3, 7, n, pad=n // 2, shift=31)
            B.describe_mask_mfft(p, min(n, 8), s, s)
        assert e.value.code == -2, e.value                 # BHW_ERR_UNSUPPORTED


def test_all_48_instances_are_built_without_scratch():
    """The compiler's report of the build (kernel_resources.json): 3 direct and 45 table instances of the new kernel, none with
    scratch or a VGPR spill, and the parent's 48 as they were counted."""
    import json
    import os
    from blackman_harris_win_amd import _build
    if not os.path.exists(_build.RESOURCES):
        _build.build_library(force=True)
    with open(_build.RESOURCES) as f:
        res = json.load(f)
    for family in ("k_mask_mfft", "k_istft_mfft"):
        direct = [k for k in res if k.startswith(family + "_direct<")]
        table = [k for k in res if k.startswith(family + "_table<")]
        assert (len(direct), len(table)) == (3, 45), (family, len(direct), len(table))
        for k in direct + table:
            assert res[k]["ScratchSize"] == 0 and res[k]["VGPRs Spill"] == 0, (k, res[k])
