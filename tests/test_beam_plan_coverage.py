"""The case table of tests/beam_cases.py against the planner, with no GPU: every class has a case and every claim holds on the describe
line of its case; the table is the complex-gain table at C = 3, case for case, and the further channel counts; every plan field of a
filter-and-sum line equals the complex-gain call's line for the same descriptors -- the plan IS that call's for the B output signals:
lanes per row, spans, columns per lane and LDS bytes -- at all 8 + 73 sizes and every channel count at the edges; and the lines begin
"beam", name the new kernels and say "channels C" and the three gain strides."""
import re

import pytest

from blackman_harris_win_amd import binding as B

import beam_cases as BC
import cmask_cases as CC

CLAIMS = [(c["id"], name) for c in BC.CASES for name in c["classes"]]
CLASS_IDS = [(fam, name) for fam in BC.FAMILIES for name in BC.CLASSES[fam]]
PLAN_FIELDS = ("signals", "frames", "rows", "n_fft", "m", "lpf", "fy", "cpl", "S", "halo", "spans", "trips", "repeated", "groups", "grid",
               "L", "col0", "pad", "t0", "schedule", "normalize", "heavy", "lds", "T_in", "pad_in", "pad_mode", "both_ffts")


@pytest.mark.parametrize("fam,name", CLASS_IDS, ids=[f"{f}: {n}" for f, n in CLASS_IDS])
def test_every_class_has_a_case(fam, name):
    claimed = [c for c in BC.CASES if c["family"] == fam and name in c["classes"]]
    assert claimed, f"no {fam} case claims the class {name!r}"
    for c in claimed:
        text = BC.line(c)
        assert BC.CLASSES[fam][name](c, BC.parse(c, text)), f"case {c['id']} is not of the class {name!r}: {text}"


@pytest.mark.parametrize("cid,name", CLAIMS, ids=[f"{c}: {n}" for c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(cid, name):
    c = BC.case(cid)
    assert name in BC.CLASSES[c["family"]], f"case {cid} claims {name!r}, which is no class"
    text = BC.line(c)
    assert BC.CLASSES[c["family"]][name](c, BC.parse(c, text)), f"case {cid} is not of the class {name!r}: {text}"


def test_the_cases_are_the_complex_gain_cases_at_three_channels_and_the_other_counts():
    three = [c for c in BC.CASES if c["C"] == 3]
    assert [c["id"] for c in three] == [f"{i}-c3" for i in CC.case_ids()]
    for c, r in zip(three, CC.CASES):
        for key in r:
            if key not in ("id", "classes"):
                assert c[key] == r[key], (c["id"], key)
    for fam in BC.FAMILIES:
        mine = [c for c in BC.CASES if c["family"] == fam]
        assert {c["C"] for c in mine} == {1, 2, 3, 8, BC.MAX_CH}
        assert {c["gains"] for c in mine if c["C"] == 3} == set(BC.LAYOUTS) and {c["pad_mode"] for c in mine} == {"reflect", "constant"}
        most = [c for c in mine if c["C"] == BC.MAX_CH]
        assert len(most) == 1 and most[0]["F"] == 2
    assert BC.MAX_CH == 64
    ids = BC.case_ids()
    assert len(set(ids)) == len(ids)
    assert {"mfft-n18-l13-c3", "mfft-n50-hop4-few-c3", "mfft-n250-l100-hop300-c3", "mfft-n1500-l100-loop-c3", "fft-n16-l13-c3",
            "fft-n2048-l100-loop-c3"} <= set(ids)


def _swap(fam, text):
    """A filter-and-sum line as the complex-gain call would have written it, but for the gain strides."""
    assert text.startswith(f"beam {fam} ")
    text = "cmask" + text[4:]
    return re.sub(r"complex gains: .*?, (\d+ signals x )", r"complex gains: \1", text.replace(f"k_beam_{fam}_", f"k_cmask_{fam}_"))


@pytest.mark.parametrize("cid", BC.case_ids())
def test_every_plan_field_is_the_complex_gain_calls(cid):
    c = BC.case(cid)
    fam = c["family"]
    text, cm = BC.line(c), BC.cmask_line(c)
    d, r = BC.parse(c, text), CC.parse(c, cm)
    for name in PLAN_FIELDS:
        assert d[name] == r[name], (cid, name, text, cm)
    assert d["signals"] == c["B"] and d["channels"] == c["C"]
    assert d["cpl"] <= 8 and d["lds"] <= BC.family(c).max_lds
    assert list(d["kernels"]) == [f"k_beam_{fam}_direct"] and d["kernels"][f"k_beam_{fam}_direct"] == r["kernels"][f"k_cmask_{fam}_direct"]
    sa, ss, L, Tin, T, C, xcs, gs, gcs, gbs = BC.desc(c)
    assert f", complex gains: channels {C}, g_stride {gs}, g_ch_stride {gcs}, g_batch_stride {gbs}, " in text
    # nothing else differs: the line is the complex-gain call's but for the first word, the kernel's name and the gain strides
    assert _swap(fam, text) == re.sub(r"complex gains: .*?, (\d+ signals x )", r"complex gains: \1", cm)


def _sweep(fam):
    for n in BC.FAMILIES[fam].sizes:
        for L in (1, 13, n // 2 + 1, n):
            for hop in (1, 7, n // 4 + 3, n + 5):
                for nb, F in ((1, 1), (3, 2), (64, 65), (1, 2049)):
                    yield n, L, hop, nb, F


@pytest.mark.parametrize("fam", list(BC.FAMILIES))
def test_the_plan_is_the_complex_gain_plan_at_every_size(fam):
    """All 8 (fft) / 73 (mfft) sizes against windows, hops, batches and frame counts at the edges, every weight layout and the channel
    counts 1, 2, 3, 8 and 64 in turn."""
    f = BC.FAMILIES[fam]
    p = f.cmask.real.params(4)
    layouts = list(BC.LAYOUTS.values())
    chans = (1, 2, 3, 8, BC.MAX_CH)
    seen, worst_cpl, worst_lds, i = set(), 0, (0, 0), 0
    for n, L, hop, nb, F in _sweep(fam):
        pad, col0 = n // 2, (n - L) // 2
        T = n + hop * (F - 1) - 2 * pad
        if T < 1:
            continue
        C = chans[i % len(chans)]
        gs, gcs, gbs = layouts[i % len(layouts)](C, F, n // 2 + 1)
        i += 1
        sa = B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, pad_mode=0, shift=31)
        ss = B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, shift=31)
        text = f.describe(p, L, sa, ss, C, normalize=True, g_stride=gs, g_ch_stride=gcs, g_batch_stride=gbs)
        cm = f.cmask.describe(p, L, sa, ss, normalize=True, g_stride=gs, g_batch_stride=gbs)
        assert _swap(fam, text) == re.sub(r"complex gains: .*?, (\d+ signals x )", r"complex gains: \1", cm), (text, cm)
        d = f.cmask.real.parse(text)
        assert d["cpl"] <= 8 and d["lds"] <= f.max_lds, text
        # a lane owns at most cpl / 4 + 1 = 3 values of k <= M / 2: what the kernels' register sums hold
        assert (d["m"] // 2) // d["lpf"] + 1 <= 3, text
        assert f"k_beam_{fam}_direct<" in text and f", complex gains: channels {C}, " in text
        seen.add(n)
        worst_cpl, worst_lds = max(worst_cpl, d["cpl"]), max(worst_lds, (d["lds"], n))
    assert sorted(seen) == f.sizes
    assert worst_cpl == 8 and worst_lds == ((40960, 2048) if fam == "fft" else (40000, 2000))


def test_the_describe_lines_name_the_new_kernels_the_channels_and_three_strides():
    for fam, f in BC.FAMILIES.items():
        n = 512 if fam == "fft" else 400
        p = f.cmask.real.params(4)
        sa = B.make_stft(2, 4000, 26, 160, n, pad=n // 2, pad_mode=1, shift=31)
        ss = B.make_stft(2, 4000, 26, 160, n, pad=n // 2, shift=31)
        K = n // 2 + 1
        text = f.describe(p, n, sa, ss, 5, normalize=True, g_stride=K, g_ch_stride=26 * K, g_batch_stride=5 * 26 * K)
        assert text.startswith(f"beam {fam} direct (L = {n}, n_fft {n},") and f"k_beam_{fam}_direct<" in text
        assert f", forward + inverse FFT, complex gains: channels 5, g_stride {K}, g_ch_stride {26 * K}, g_batch_stride {5 * 26 * K}, 2 signals x " in text
        assert "complex gains: channels 1, g_stride 0, g_ch_stride 0, g_batch_stride 0, " in f.describe(p, n, sa, ss, 1)
        # the channel stride of x does not enter the plan
        assert f.describe(p, n, sa, ss, 5, x_ch_stride=4100, g_ch_stride=K) == f.describe(p, n, sa, ss, 5, g_ch_stride=K)
        s0 = B.make_stft(2, 0, 26, 160, n, pad=n // 2, shift=31)
        assert f.describe(p, n, sa, s0, 5).startswith(f"beam {fam} direct (L = {n}, n_fft {n}), ") and "nothing (samples 0)" in f.describe(p, n, sa, s0, 5)


def test_unsupported_sizes_have_no_plan():
    for fam, bad in (("fft", (8, 400, 2000, 4096, 4050, 22)), ("mfft", (14, 22, 512, 2048, 2160, 4050, 4096))):
        f = BC.FAMILIES[fam]
        for n in bad:
            s = B.make_stft(1, 10000, 3, 7, n, pad=n // 2, shift=31)
            with pytest.raises(B.BhwError) as e:
                f.describe(f.cmask.real.params(4), min(n, 8), s, s, 2, g_ch_stride=n)
            assert e.value.code in (-2, -1), (fam, n, e.value)


def test_all_96_instances_are_built_without_scratch():
    """The compiler's report of the build (kernel_resources.json): 3 direct and 45 table instances of each new kernel, none with scratch
    or a VGPR spill (as in the siblings, scalar registers parked in vector lanes are no scratch).  The twelve register sums cost a workgroup of occupancy against the complex-gain siblings (3 waves per SIMD where they
    have 4: DESIGN.md section 45), which this test records: no further one may go unnoticed."""
    import json
    import os
    from blackman_harris_win_amd import _build
    if not os.path.exists(_build.RESOURCES):
        _build.build_library(force=True)
    with open(_build.RESOURCES) as fjson:
        res = json.load(fjson)
    for fam in BC.FAMILIES:
        direct = [k for k in res if k.startswith(f"k_beam_{fam}_direct<")]
        table = [k for k in res if k.startswith(f"k_beam_{fam}_table<")]
        assert (len(direct), len(table)) == (3, 45), (fam, len(direct), len(table))
        for k in direct + table:
            assert res[k]["ScratchSize"] == 0 and res[k]["VGPRs Spill"] == 0, (k, res[k])
            assert res[k]["Occupancy"] >= 3 and res[k]["VGPRs"] <= 168, (k, res[k])
