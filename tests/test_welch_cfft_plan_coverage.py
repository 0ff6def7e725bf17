"""The case table of tests/welch_cfft_cases.py reaches every plan class of the fused Welch PSD for I/Q input: every class has a case,
every claim holds on the describe line of its case (host arithmetic, no GPU), a sweep of the planner over all eight supported n_fft
and over frame counts at the edges of a chunk, a run, a block and the grid emits no shape the table's cases do not hold, and the
fields the line shares with bhw_describe_stft_cfft are that call's."""
import pytest

from blackman_harris_win_amd import binding as B

import stft_cfft_cases as SC
import welch_cfft_cases as WC

CLAIMS = [(c["id"], name) for c in WC.CASES for name in c["classes"]]
SHARED = ("signals", "frames", "rows", "n_fft", "m", "lpf", "fy", "cpl", "lds", "L", "col0", "pad", "schedule", "detrend", "reflect", "table",
          "shifted")


@pytest.mark.parametrize("name", list(WC.CLASSES))
def test_every_class_has_a_case(name):
    claimed = [c for c in WC.CASES if name in c["classes"]]
    assert claimed, f"no case claims the class {name!r}"
    for c in claimed:
        line = WC.line(c)
        assert WC.CLASSES[name](c, WC.parse(line)), f"case {c['id']} is not of the class {name!r}: {line}"


@pytest.mark.parametrize("cid,name", CLAIMS, ids=[f"{c}: {n}" for c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(cid, name):
    assert name in WC.CLASSES, f"case {cid} claims {name!r}, which is no class"
    c = WC.case(cid)
    line = WC.line(c)
    assert WC.CLASSES[name](c, WC.parse(line)), f"case {cid} is not of the class {name!r}: {line}"


def test_case_ids_are_unique_and_every_case_is_there_for_a_class():
    ids = WC.case_ids()
    assert len(set(ids)) == len(ids), ids
    assert all(c["classes"] for c in WC.CASES)
    assert set(WC.SHIFTED) <= set(ids)
    # one shifted case of each regime, and 2048
    fys = {WC.parse(WC.line(WC.case(cid), fftshift=True))["fy"] for cid in WC.SHIFTED}
    assert any(fy >= WC.CHUNK for fy in fys) and any(fy < WC.CHUNK for fy in fys) and "n2048-detrend-1x35" in WC.SHIFTED


@pytest.mark.parametrize("cid", WC.case_ids())
def test_the_cases_have_the_frames_the_issue_names(cid):
    c = WC.case(cid)
    s, _, frames, _ = WC.desc(c)
    assert s.channels == 2 and s.y_stride == 0 and s.y_batch_stride == 0
    if "F" in c:
        assert frames == c["F"] == s.frames
    if cid == "n16-1x131142":
        assert s.samples == 262298


def _shape(d):
    return (d["n_fft"], d["schedule"], d["lpf"], d["fy"], d["cpl"], d["lds"], d["run"], d["gpr"], d["acc"])


def test_the_planner_emits_no_shape_without_a_case():
    """The plan's shape is a function of n_fft alone; the frames and the batch only set the runs, the chunks, the blocks and the grid.
    Every n_fft the checks accept, at frame counts around a chunk, a run, a block and the grid cap: the shape is one a case has, the
    layout is lpf = min(256, max(4, n / 4)) and fy = 256 / lpf, the runs cover every signal's padded frame axis once and never cross
    a signal, and the workspace is the header's formula."""
    p = WC.params(4)
    covered = {_shape(WC.parse(WC.line(c))) for c in WC.CASES}
    seen = set()
    for lg in range(4, 12):
        n = 1 << lg
        for F in (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 513, 4096, 4097, 16 * 2048, 16 * 2048 + 1, 64 * 2048, 64 * 2048 + 1, 140000):
            if F * n > 1 << 33:
                continue
            for nb in (1, 3):
                if nb * F * n > 1 << 34:
                    continue
                for det in (False, True):
                    for sh in (False, True):
                        s = B.make_stft(nb, (F - 1) * 3 + n, F, 3, n, channels=2, shift=31)
                        d = WC.parse(B.describe_welch_cfft(p, n, s, detrend=det, fftshift=sh))
                        assert _shape(d) in covered, d["line"]
                        assert d["lpf"] == min(256, max(4, n // 4)) and d["fy"] == 256 // d["lpf"] and d["shifted"] == sh
                        assert d["chunk"] == WC.CHUNK and d["run"] == max(WC.CHUNK, d["fy"]) and d["gpr"] == d["run"] // d["fy"]
                        assert d["acc"] == (0 if d["fy"] >= WC.CHUNK else -(-n // 256)) <= 8
                        fpad = -(-F // d["run"]) * d["run"]
                        assert d["runs"] == nb * fpad // d["run"] and d["groups"] == d["runs"] * d["gpr"] == nb * fpad // d["fy"]
                        assert d["grid"] == min(d["runs"], WC.MAX_GRID)
                        assert d["chunks"] == -(-F // WC.CHUNK) and d["blocks"] == -(-F // WC.BLOCK)
                        assert d["joins"] == (2 if d["blocks"] > 1 else 1)
                        assert d["workspace"] == 8 * WC.workspace_doubles(nb, F, n) == B.welch_cfft_workspace_bytes(s)
                        seen.add(_shape(d))
    assert seen == covered                          # and no case is of a shape the planner would not emit


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("cid", WC.case_ids())
def test_the_shared_fields_are_describe_stft_cffts(cid, shifted):
    c = WC.case(cid)
    s, L, _, det = WC.desc(c)
    p = WC.params(c["setup"])
    w = WC.parse(B.describe_welch_cfft(p, L, s, detrend=det, fftshift=shifted))
    f = SC.parse(B.describe_stft_cfft(p, L, s, detrend=det, fftshift=shifted))
    for name in SHARED:
        assert w[name] == f[name], (cid, name, w["line"], f["line"])
    assert not w["power"]
    # the same words around them: the text from the signals to the columns per lane (the groups and the grid are recounted)
    cut = lambda t: t[t.index(" signals x"):t.index(" groups, grid")].rsplit(",", 1)[0]
    assert cut(w["line"]) == cut(f["line"])
    # and before them, but for the call's name and the output form, which this call has not
    head = lambda t, name: t[:t.index(": k_")].replace(name, "X")
    assert head(w["line"], "welch cfft") == head(f["line"], "stft cfft").replace(", spectrum rows", "")
    assert {k.replace("welch_cfft", "stft_cfft"): a for k, a in w["kernels"].items() if k != "k_welch_fft_join"} == f["kernels"]


def test_unsupported_sizes_have_no_plan():
    p = WC.params(4)
    for n in (8, 15, 17, 100, 400, 4096, 8192):
        with pytest.raises(B.BhwError) as e:
            B.describe_welch_cfft(p, min(n, 8), B.make_stft(1, 100000, 3, 7, n, channels=2, shift=31))
        assert e.value.code == -2, e.value                 # BHW_ERR_UNSUPPORTED
