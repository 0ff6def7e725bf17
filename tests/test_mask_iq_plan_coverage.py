"""The case table of tests/mask_iq_cases.py against the planner, with no GPU: every class has a case and every claim holds on the
describe line of its case; the table is the two inverse I/Q tables, case for case; a sweep of the planner over all 8 + 91 sizes emits
no (schedule, spans per workgroup, columns per lane) shape the table lacks; every plan field of a line equals the inverse I/Q
parent's line for the synthesis descriptor, CHARACTER FOR CHARACTER, except for the kernel name, the LDS bytes and the added words;
the LDS bytes are the parent's plus one twiddle table (power of two) or the parent's (mixed radix); and the 192 new kernel instances
are built without scratch or a VGPR spill."""
import re

import pytest

from blackman_harris_win_amd import binding as B

import mask_iq_cases as MC

CLAIMS = [(c["id"], name) for c in MC.CASES for name in c["classes"]]
CLASS_IDS = [(fam, name) for fam in MC.FAMILIES for name in MC.CLASSES[fam]]
MAX_LDS = {"cfft": 57344, "cmfft": 56700}


@pytest.mark.parametrize("fam,name", CLASS_IDS, ids=[f"{f}: {n}" for f, n in CLASS_IDS])
def test_every_class_has_a_case(fam, name):
    claimed = [c for c in MC.CASES if c["family"] == fam and name in c["classes"]]
    assert claimed, f"no {fam} case claims the class {name!r}"
    for c in claimed:
        text = MC.line(c)
        assert MC.CLASSES[fam][name](c, MC.parse(c, text)), f"case {c['id']} is not of the class {name!r}: {text}"


@pytest.mark.parametrize("cid,name", CLAIMS, ids=[f"{c}: {n}" for c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(cid, name):
    c = MC.case(cid)
    assert name in MC.CLASSES[c["family"]], f"case {cid} claims {name!r}, which is no class"
    text = MC.line(c)
    assert MC.CLASSES[c["family"]][name](c, MC.parse(c, text)), f"case {cid} is not of the class {name!r}: {text}"


def test_the_cases_are_the_inverse_iq_cases_of_both_families():
    for fam, f in MC.FAMILIES.items():
        mine = [c for c in MC.CASES if c["family"] == fam]
        assert [c["id"] for c in mine] == [f"{fam}-{i}" for i in f.parent.case_ids()]       # every case: the new calls accept them all
        for c, r in zip(mine, f.parent.CASES):
            for key in r:
                if key not in ("id", "classes"):
                    assert c[key] == r[key], (c["id"], key)
            assert {n for n in r["classes"] if n in MC.CLASSES[fam]} <= set(c["classes"])
        assert {c["gains"] for c in mine} == set(MC.LAYOUTS) and {c["pad_mode"] for c in mine} == {"reflect", "constant"}
        assert {c["gtype"] for c in mine} == set(MC.GTYPES)
        for c in mine:                                                   # what the Python calls refuse is not in the table
            L, col0, pad, Tin, T = MC.geometry(c)
            assert c["center"] or c["L"] == c["n_fft"]
            assert c["pad_mode"] == "constant" or pad < Tin, c["id"]
    assert len(MC.FAMILIES["cfft"].sizes) == 8 and len(MC.FAMILIES["cmfft"].sizes) == 91
    ids = MC.case_ids()
    assert len(set(ids)) == len(ids)
    shifted = {c["n_fft"] for c in MC.CASES if c.get("fftshift")}
    assert any(n % 2 for n in shifted) and any(n % 2 == 0 for n in shifted)
    assert any(c.get("odd") for c in MC.CASES if c["family"] == "cfft") and any(c.get("odd") for c in MC.CASES if c["family"] == "cmfft")


def _as_parent(c, text):
    """A mask line with the added words taken out and the kernel renamed: what is left must be the parent's line but for the LDS."""
    fam, stem = c["family"], MC.c_name(c["family"], c["gtype"])
    head, rest = text.split(": ", 1) if "t0 = " not in text.split(": ", 1)[0] else (None, None)
    m = re.match(r"^c?mask (\w+) (\w+) \((.*?); analysis of \d+ samples, pad \d+ (?:reflect|constant)\), (.*?): (k_\w+)(<[\w,]+>), "
                 r"forward \+ inverse FFT, (?:complex )?gains: .*?, gain columns (shifted|in order), (.*)$", text)
    assert m, text
    family, route, geo, norm, kern, inst, cols, fields = m.groups()
    assert family == fam and kern in (f"k_{stem}_direct", f"k_{stem}_table")
    bins = "bins shifted" if cols == "shifted" else "bins in order"
    return f"istft {fam} {route} ({geo}), {norm}, {bins}: {kern.replace(stem, 'istft_' + fam)}{inst}, {fields}"


def _lds(text):
    return int(re.search(r"(\d+) bytes of LDS", text).group(1))


def _without_lds(text):
    return re.sub(r"\d+ bytes of LDS", "# bytes of LDS", text)


@pytest.mark.parametrize("cid", MC.case_ids())
def test_every_plan_field_is_the_inverse_parents_character_for_character(cid):
    c = MC.case(cid)
    text, parent = MC.line(c), MC.parent_line(c)
    assert _without_lds(_as_parent(c, text)) == _without_lds(parent), (text, parent)
    n = c["n_fft"]
    assert _lds(text) == _lds(parent) + (n // 2 * 8 if c["family"] == "cfft" else 0), (text, parent)
    d = MC.parse(c, text)
    assert d["cpl"] <= 8 and d["lds"] <= MAX_LDS[c["family"]] and d["both_ffts"]
    assert d["T_in"] == MC.geometry(c)[3] and d["pad_mode"] == c["pad_mode"]
    assert d["columns_shifted"] == bool(c.get("fftshift")) and d["complex_gains"] == (c["gtype"] == "pair")


def _sweep(fam):
    for n in MC.FAMILIES[fam].sizes:
        for L in (1, 13, n // 2 + 1, n):
            for hop in (1, 7, n // 4 + 3, n + 5):
                for nb, F in ((1, 1), (3, 2), (64, 65), (1, 2049)):
                    yield n, L, hop, nb, F


@pytest.mark.parametrize("fam", list(MC.FAMILIES))
def test_a_sweep_of_the_planner_emits_no_shape_the_table_lacks(fam):
    """All 8 (cfft) / 91 (cmfft) sizes against windows, hops, batches and frame counts at the edges, every gain layout and both gain
    types in turn: the line is the parent's but for the LDS, and its (schedule, spans per workgroup, columns per lane) is in the table."""
    f = MC.FAMILIES[fam]
    p = MC.params_of(4)
    layouts = list(MC.LAYOUTS.values())
    seen, shapes, parsed, worst_cpl, worst_lds, i = set(), {}, {}, 0, (0, 0), 0
    for n, L, hop, nb, F in _sweep(fam):
        pad, col0 = n // 2, (n - L) // 2
        T = n + hop * (F - 1) - 2 * pad
        if T < 1:
            continue
        gs, gbs = layouts[i % len(layouts)](F, n)
        gtype, shift = MC.GTYPES[i % 2], bool(i % 3 == 0)
        i += 1
        sa = B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, pad_mode=0, channels=2, shift=31)
        ss = B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, channels=2, shift=31)
        text = MC.describe(fam, gtype)(p, L, sa, ss, normalize=True, fftshift=shift, g_stride=gs, g_batch_stride=gbs)
        parent = f.describe_parent(p, L, ss, normalize=True, fftshift=shift)
        c = dict(family=fam, gtype=gtype)
        assert _without_lds(_as_parent(c, text)) == _without_lds(parent), (text, parent)
        assert _lds(text) == _lds(parent) + (n // 2 * 8 if fam == "cfft" else 0)
        d = MC.parse(c, text)
        shapes.setdefault(n, set()).add((d["schedule"], d["fy"], d["cpl"], d["lpf"]))
        parsed[n] = d
        seen.add(n)
        worst_cpl, worst_lds = max(worst_cpl, d["cpl"]), max(worst_lds, (d["lds"], n))
    assert sorted(seen) == f.sizes
    assert all(len(s) == 1 for s in shapes.values())                      # the lanes and the schedule are a function of n_fft alone
    # what the kernels branch on beyond the spans, as the parents' coverage tests define it: the table has all the sweep emits
    P = f.parent
    have = [MC.parse(c, MC.line(c)) for c in MC.CASES if c["family"] == fam]
    if fam == "cfft":
        shapes_of = lambda d: {(d["schedule"], min(d["fy"], 2), d["cpl"])}
    else:
        shapes_of = lambda d: {("pass",) + s for s in P.pass_shapes(d)} | {("layout", P.layout(d)), ("slots", min(d["fy"], 2))}
    table_shapes = set().union(*(shapes_of(d) for d in have))
    for n, d in parsed.items():
        assert shapes_of(d) <= table_shapes, (n, sorted(map(str, shapes_of(d) - table_shapes)), d["line"])
    assert worst_cpl == 8 and worst_lds == ((57344, 2048) if fam == "cfft" else (56700, 2025))


def test_the_describe_lines_name_the_new_kernels_the_gains_and_the_columns():
    for fam, f in MC.FAMILIES.items():
        n = 512 if fam == "cfft" else 75
        p = MC.params_of(4)
        sa = B.make_stft(2, 4000, 26, 150, n, pad=n // 2, pad_mode=1, channels=2, shift=31)
        ss = B.make_stft(2, 4000, 26, 150, n, pad=n // 2, channels=2, shift=31)
        for gtype, c, word in (("real", "", ""), ("pair", "c", "complex ")):
            d = MC.describe(fam, gtype)
            text = d(p, n, sa, ss, normalize=True, g_stride=n, g_batch_stride=26 * n)
            assert text.startswith(f"{c}mask {fam} direct (L = {n}, n_fft {n},") and f"k_{c}mask_{fam}_direct<" in text
            assert f", forward + inverse FFT, {word}gains: g_stride {n}, g_batch_stride {26 * n}, gain columns in order, 2 signals x " in text
            assert f"{word}gains: one gain row for every frame and every signal, gain columns shifted, " in d(p, n, sa, ss, fftshift=True)
            s0 = B.make_stft(2, 0, 26, 150, n, pad=n // 2, channels=2, shift=31)
            assert d(p, n, sa, s0).startswith(f"{c}mask {fam} direct (L = {n}, n_fft {n}), ") and "nothing (samples 0)" in d(p, n, sa, s0)


def test_unsupported_sizes_have_no_plan():
    for fam, bad in (("cfft", (8, 400, 2000, 4096, 4050, 22)), ("cmfft", (14, 22, 512, 2048, 2160, 4050, 4096))):
        for n in bad:
            s = B.make_stft(1, 10000, 3, 7, n, pad=n // 2, channels=2, shift=31)
            for gtype in MC.GTYPES:
                with pytest.raises(B.BhwError) as e:
                    MC.describe(fam, gtype)(MC.params_of(4), min(n, 8), s, s)
                assert e.value.code in (-2, -1), (fam, n, e.value)


def test_all_192_instances_are_built_without_scratch_or_spills():
    """The compiler's report of the build (kernel_resources.json): 3 direct and 45 table instances of each of the four new kernels,
    none with scratch or a VGPR spill, and no fewer waves per SIMD than the inverse parent of the family has (three workgroups a CU)."""
    import json
    import os
    from blackman_harris_win_amd import _build
    if not os.path.exists(_build.RESOURCES):
        _build.build_library(force=True)
    with open(_build.RESOURCES) as fjson:
        res = json.load(fjson)
    for fam in MC.FAMILIES:
        parent = min(res[k]["Occupancy"] for k in res if k.startswith(f"k_istft_{fam}_"))
        for gtype in MC.GTYPES:
            kernel = "k_" + MC.c_name(fam, gtype)
            direct = [k for k in res if k.startswith(kernel + "_direct<")]
            table = [k for k in res if k.startswith(kernel + "_table<")]
            assert (len(direct), len(table)) == (3, 45), (kernel, len(direct), len(table))
            for k in direct + table:
                assert res[k]["ScratchSize"] == 0 and res[k]["VGPRs Spill"] == 0, (k, res[k])
                assert res[k]["Occupancy"] >= parent, (k, res[k], parent)
