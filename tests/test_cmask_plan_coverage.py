"""The case table of tests/cmask_cases.py against the planner, with no GPU: every class has a case and every claim holds on the describe
line of its case; the table is the two real-gain tables, case for case; every plan field of a complex-gain line equals the real-gain
call's line for the same arguments -- the plan IS that call's: lanes per row, spans, columns per lane and LDS bytes -- at all 8 + 73
sizes, with at most 8 columns per lane and 40 960 / 40 000 bytes of LDS; and the lines name the new kernels and "complex gains" while
the real calls' lines are the strings they were."""
import pytest

from blackman_harris_win_amd import binding as B

import cmask_cases as CC

CLAIMS = [(c["id"], name) for c in CC.CASES for name in c["classes"]]
CLASS_IDS = [(fam, name) for fam in CC.FAMILIES for name in CC.CLASSES[fam]]
PLAN_FIELDS = ("signals", "frames", "rows", "n_fft", "m", "lpf", "fy", "cpl", "S", "halo", "spans", "trips", "repeated", "groups", "grid",
               "L", "col0", "pad", "t0", "schedule", "normalize", "heavy", "lds", "T_in", "pad_in", "pad_mode", "g_stride", "g_batch_stride",
               "one_row_per_frame", "one_set_per_signal", "both_ffts")


@pytest.mark.parametrize("fam,name", CLASS_IDS, ids=[f"{f}: {n}" for f, n in CLASS_IDS])
def test_every_class_has_a_case(fam, name):
    claimed = [c for c in CC.CASES if c["family"] == fam and name in c["classes"]]
    assert claimed, f"no {fam} case claims the class {name!r}"
    for c in claimed:
        text = CC.line(c)
        assert CC.CLASSES[fam][name](c, CC.parse(c, text)), f"case {c['id']} is not of the class {name!r}: {text}"


@pytest.mark.parametrize("cid,name", CLAIMS, ids=[f"{c}: {n}" for c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(cid, name):
    c = CC.case(cid)
    assert name in CC.CLASSES[c["family"]], f"case {cid} claims {name!r}, which is no class"
    text = CC.line(c)
    assert CC.CLASSES[c["family"]][name](c, CC.parse(c, text)), f"case {cid} is not of the class {name!r}: {text}"


def test_the_cases_are_the_real_gain_cases_of_both_families():
    for fam, f in CC.FAMILIES.items():
        mine = [c for c in CC.CASES if c["family"] == fam]
        assert [c["id"] for c in mine] == [f"{fam}-{i}" for i in f.real.case_ids()]
        for c, r in zip(mine, f.real.CASES):
            for key in r:
                if key not in ("id", "classes"):
                    assert c[key] == r[key], (c["id"], key)
            assert set(r["classes"]) < set(c["classes"])
        assert set(CC.CLASSES[fam]) == set(f.real.CLASSES) | {"complex gains"}
        assert {c["gains"] for c in mine} == set(CC.LAYOUTS) and {c["pad_mode"] for c in mine} == {"reflect", "constant"}
    assert len(CC.FAMILIES["fft"].sizes) == 8 and len(CC.FAMILIES["mfft"].sizes) == 73
    ids = CC.case_ids()
    assert len(set(ids)) == len(ids)
    # the smallest shapes of every plan class are here: odd M, one row per workgroup at the largest sizes, the group loop
    assert {"mfft-n18-l13", "mfft-n50-hop4-few", "mfft-n250-l100-hop300", "mfft-n1500-l100-loop", "fft-n16-l13", "fft-n2048-l100-loop"} <= set(ids)


def _swap(fam, text):
    """A complex-gain line as the real-gain call would have written it."""
    assert text.startswith(f"cmask {fam} ")
    return text[1:].replace(f"k_cmask_{fam}_", f"k_mask_{fam}_").replace(", complex gains: ", ", gains: ")


@pytest.mark.parametrize("cid", CC.case_ids())
def test_every_plan_field_is_the_real_gain_calls(cid):
    c = CC.case(cid)
    fam = c["family"]
    text, real = CC.line(c), CC.real_line(c)
    d, r = CC.parse(c, text), CC.parse(c, real)
    for name in PLAN_FIELDS:
        assert d[name] == r[name], (cid, name, text, real)
    assert d["cpl"] <= 8 and d["lds"] <= CC.family(c).max_lds
    assert list(d["kernels"]) == [f"k_cmask_{fam}_direct"] and list(r["kernels"]) == [f"k_mask_{fam}_direct"]
    assert d["kernels"][f"k_cmask_{fam}_direct"] == r["kernels"][f"k_mask_{fam}_direct"]
    assert d["complex_gains"] and "complex gains" not in real and real.startswith(f"mask {fam} direct ")
    # nothing else differs: the line is the real call's but for the first letter, the kernel's name and the word "complex"
    assert _swap(fam, text) == real


def _sweep(fam):
    for n in CC.FAMILIES[fam].sizes:
        for L in (1, 13, n // 2 + 1, n):
            for hop in (1, 7, n // 4 + 3, n + 5):
                for nb, F in ((1, 1), (3, 2), (64, 65), (1, 2049)):
                    yield n, L, hop, nb, F


@pytest.mark.parametrize("fam", list(CC.FAMILIES))
def test_the_plan_is_the_real_gain_plan_at_every_size(fam):
    """All 8 (fft) / 73 (mfft) sizes against windows, hops, batches and frame counts at the edges, every gain layout in turn."""
    f = CC.FAMILIES[fam]
    p = f.real.params(4)
    layouts = list(CC.LAYOUTS.values())
    seen, worst_cpl, worst_lds, i = set(), 0, (0, 0), 0
    for n, L, hop, nb, F in _sweep(fam):
        pad, col0 = n // 2, (n - L) // 2
        T = n + hop * (F - 1) - 2 * pad
        if T < 1:
            continue
        gs, gbs = layouts[i % len(layouts)](F, n // 2 + 1)
        i += 1
        sa = B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, pad_mode=0, shift=31)
        ss = B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, shift=31)
        kw = dict(normalize=True, g_stride=gs, g_batch_stride=gbs)
        text, real = f.describe(p, L, sa, ss, **kw), f.describe_real(p, L, sa, ss, **kw)
        assert _swap(fam, text) == real, (text, real)
        d = f.real.parse(text)
        assert d["cpl"] <= 8 and d["lds"] <= f.max_lds, text
        assert f"k_cmask_{fam}_direct<" in text and ", complex gains: " in text
        seen.add(n)
        worst_cpl, worst_lds = max(worst_cpl, d["cpl"]), max(worst_lds, (d["lds"], n))
    assert sorted(seen) == f.sizes
    assert worst_cpl == 8 and worst_lds == ((40960, 2048) if fam == "fft" else (40000, 2000))


def test_the_describe_lines_name_the_new_kernels_and_complex_gains():
    for fam, f in CC.FAMILIES.items():
        n = 512 if fam == "fft" else 400
        p = f.real.params(4)
        sa = B.make_stft(2, 4000, 26, 160, n, pad=n // 2, pad_mode=1, shift=31)
        ss = B.make_stft(2, 4000, 26, 160, n, pad=n // 2, shift=31)
        K = n // 2 + 1
        text = f.describe(p, n, sa, ss, normalize=True, g_stride=K, g_batch_stride=26 * K)
        assert text.startswith(f"cmask {fam} direct (L = {n}, n_fft {n},") and f"k_cmask_{fam}_direct<" in text
        assert f", forward + inverse FFT, complex gains: g_stride {K}, g_batch_stride {26 * K}, " in text
        assert "complex gains: one gain row for every frame and every signal" in f.describe(p, n, sa, ss)
        real = f.describe_real(p, n, sa, ss, normalize=True, g_stride=K, g_batch_stride=26 * K)
        assert real.startswith(f"mask {fam} direct (") and f"k_mask_{fam}_direct<" in real and ", forward + inverse FFT, gains: g_stride" in real
        # samples 0: nothing to do, in the new call's name
        s0 = B.make_stft(2, 0, 26, 160, n, pad=n // 2, shift=31)
        assert f.describe(p, n, sa, s0).startswith(f"cmask {fam} direct (L = {n}, n_fft {n}), ") and "nothing (samples 0)" in f.describe(p, n, sa, s0)


def test_unsupported_sizes_have_no_plan():
    for fam, bad in (("fft", (8, 400, 2000, 4096, 4050, 22)), ("mfft", (14, 22, 512, 2048, 2160, 4050, 4096))):
        f = CC.FAMILIES[fam]
        for n in bad:
            s = B.make_stft(1, 10000, 3, 7, n, pad=n // 2, shift=31)
            with pytest.raises(B.BhwError) as e:
                f.describe(f.real.params(4), min(n, 8), s, s)
            assert e.value.code in (-2, -1), (fam, n, e.value)


def test_all_96_instances_are_built_without_scratch_at_four_workgroups():
    """The compiler's report of the build (kernel_resources.json): 3 direct and 45 table instances of each new kernel, none with scratch
    or a VGPR spill, at the occupancy of the real-gain siblings (4 waves per SIMD: under 128 registers)."""
    import json
    import os
    from blackman_harris_win_amd import _build
    if not os.path.exists(_build.RESOURCES):
        _build.build_library(force=True)
    with open(_build.RESOURCES) as fjson:
        res = json.load(fjson)
    for fam in CC.FAMILIES:
        for kernel in (f"k_cmask_{fam}", f"k_mask_{fam}"):
            direct = [k for k in res if k.startswith(kernel + "_direct<")]
            table = [k for k in res if k.startswith(kernel + "_table<")]
            assert (len(direct), len(table)) == (3, 45), (kernel, len(direct), len(table))
            for k in direct + table:
                assert res[k]["ScratchSize"] == 0 and res[k]["VGPRs Spill"] == 0, (k, res[k])
                assert res[k]["Occupancy"] == 4 and res[k]["VGPRs"] <= 128, (k, res[k])
