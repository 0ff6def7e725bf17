"""The case table of tests/hold_real_cases.py reaches every plan class of the fused max-hold / min-hold traces for real input, both
families: every class has a case, every claim holds on the describe line of its case (host arithmetic, no GPU), a sweep of the planner
over all 9 + 95 supported n_fft and over frame counts at the edges of a chunk, a run, a block and the grid emits no regime the table's
cases do not hold, and the line is the Welch sibling's field for field, with the traces behind it."""
import pytest

from blackman_harris_win_amd import binding as B

import hold_real_cases as H

CLAIMS = [(c["id"], name) for c in H.CASES for name in c["classes"]]
CLASS_IDS = [(fam, name) for fam in H.FAMILIES for name in H.CLASSES[fam]]


@pytest.mark.parametrize("family,name", CLASS_IDS, ids=[f"{f}: {n}" for f, n in CLASS_IDS])
def test_every_class_has_a_case(family, name):
    claimed = [c for c in H.CASES if c["family"] == family and name in c["classes"]]
    assert claimed, f"no {family} case claims the class {name!r}"
    for c in claimed:
        line = H.line(family, c, traces=c["traces"])
        assert H.CLASSES[family][name](c, H.parse(family, line)), f"case {c['id']} is not of the class {name!r}: {line}"


@pytest.mark.parametrize("cid,name", CLAIMS, ids=[f"{c}: {n}" for c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(cid, name):
    c = H.case(cid)
    assert name in H.CLASSES[c["family"]], f"case {cid} claims {name!r}, which is no class"
    line = H.line(c["family"], c, traces=c["traces"])
    assert H.CLASSES[c["family"]][name](c, H.parse(c["family"], line)), f"case {cid} is not of the class {name!r}: {line}"


def test_the_table_is_the_siblings_and_every_selection_meets_both_regimes():
    ids = H.case_ids()
    assert len(set(ids)) == len(ids), ids
    assert len(H.case_ids("fft")) == len(H.WF.CASES) == 14 and len(H.case_ids("mfft")) == len(H.WM.CASES) == 14
    for fam in H.FAMILIES:
        for t in H.TRACES:
            fys = [H.parse(fam, H.line(fam, c))["fy"] for c in H.CASES if c["family"] == fam and c["traces"] == t]
            assert any(fy >= H.CHUNK for fy in fys) and any(fy < H.CHUNK for fy in fys), (fam, t, fys)
    assert H.SIZES["fft"] == [16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
    assert len(H.SIZES["mfft"]) == 95 and H.SIZES["mfft"][0] == 18 and H.SIZES["mfft"][-1] == 4050
    assert all(n % 2 == 0 and n & (n - 1) for n in H.SIZES["mfft"])


@pytest.mark.parametrize("family", H.FAMILIES)
def test_the_planner_emits_no_regime_without_a_case(family):
    """Every n_fft the checks accept, at frame counts around a chunk, a run, a block and the grid cap, every selection of traces: the
    regime (fy, groups per run, pairs carried per lane, bin M aside) is one a case has, the line is the Welch sibling's in the hold
    call's names, and the workspace is the sibling's figure."""
    p = H.params(4)
    welch, hold = H._WELCH[family], H._DESCRIBE[family]
    covered = {H.regime(family, H.parse(family, H.line(family, c))) for c in H.CASES if c["family"] == family}
    classes = lambda r: (r[0], r[1], r[3])           # noqa: E731  the branches; the count of pairs is the bound of a predicate
    seen = set()
    for n in H.SIZES[family]:
        K = n // 2 + 1
        for F in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513, 4097, 16 * 2048 + 1, 64 * 2048 + 1, 140000):
            if F * K > 1 << 33:
                continue
            for nb in (1, 3):
                if nb * F * K > 1 << 34:
                    continue
                for i, det in enumerate((False, True)):
                    t = H.TRACES[(i + F) % 3]
                    s = B.make_stft(nb, (F - 1) * 3 + n, F, 3, n, shift=31)
                    line = hold(p, min(n, 16), s, detrend=det, traces=t)
                    d = H.parse(family, line)
                    assert classes(H.regime(family, d)) in {classes(r) for r in covered}, line
                    assert d["traces"] == t and d["detrend"] == det
                    assert H.to_welch(family, line) == welch(p, min(n, 16), s, detrend=det)
                    assert d["acc"] == (0 if d["fy"] >= H.CHUNK else -(-K // 256)) <= (9 if family == "fft" else 8)
                    assert d["chunks"] == -(-F // H.CHUNK) and d["blocks"] == -(-F // H.BLOCK)
                    assert d["workspace"] == H.HOLD_WS[family](s) == H.WELCH_WS[family](s) == 8 * H.WF.workspace_doubles(nb, F, K)
                    seen.add(classes(H.regime(family, d)))
    assert seen == {classes(r) for r in covered}    # and no case is of a regime the planner would not emit


@pytest.mark.parametrize("cid", H.case_ids())
def test_the_shared_fields_are_the_welch_siblings(cid):
    c = H.case(cid)
    fam = c["family"]
    for t in H.TRACES:
        h = H.line(fam, c, traces=t)
        w = H.welch_line(fam, c)
        assert h.startswith(f"hold {fam} direct (") and f"k_hold_{fam}_direct<" in h and "k_hold_join" in h and "welch" not in h
        assert H.to_welch(fam, h) == w, (h, w)
        assert h.endswith({"both": "; traces: max, min", "max": "; traces: max", "min": "; traces: min"}[t])
        dh, dw = H.parse(fam, h), H._MOD[fam].parse(w)
        for name in dw:
            if name not in ("line", "kernels"):
                assert dh[name] == dw[name], (cid, name, h, w)


def test_frames_0_has_a_line_with_the_traces():
    p = H.params(4)
    for fam, n in (("fft", 64), ("mfft", 400)):
        s = B.make_stft(2, 10, 0, 3, n, shift=31)
        h = H._DESCRIBE[fam](p, 16, s, traces="min")
        assert h.endswith("nothing (frames 0); traces: min") and H.to_welch(fam, h) == H._WELCH[fam](p, 16, s)


def test_unsupported_sizes_have_no_plan():
    p = H.params(4)
    for fam, sizes in (("fft", (8, 18, 400, 8192)), ("mfft", (8, 14, 15, 16, 17, 21, 64, 448, 512, 2048, 4096, 4374))):
        for n in sizes:
            with pytest.raises(B.BhwError) as e:
                H._DESCRIBE[fam](p, min(n, 8), B.make_stft(1, 100000, 3, 7, n, shift=31))
            assert e.value.code in (-1, -2), e.value           # n_fft 8 is below the window rule of some checks; the rest are UNSUPPORTED
            if n >= 14:
                assert e.value.code == -2, e.value
