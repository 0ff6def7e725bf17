"""The case table of tests/welch_cmfft_cases.py reaches every plan class of the fused Welch PSD for I/Q input at a mixed-radix n_fft:
every class has a case, every claim holds on the describe line of its case (host arithmetic, no GPU), a sweep of the planner over
all 91 supported n_fft and over frame counts at the edges of a chunk, a run, a block and the grid emits no regime the table's cases do
not hold, and the fields the line shares with bhw_describe_stft_cmfft are that call's."""
import pytest

from blackman_harris_win_amd import binding as B

import stft_cmfft_cases as MC
import welch_cmfft_cases as WM

CLAIMS = [(c["id"], name) for c in WM.CASES for name in c["classes"]]
SHARED = ("signals", "frames", "rows", "n_fft", "m", "lpf", "fy", "cpl", "lds", "L", "col0", "pad", "schedule", "detrend", "reflect", "table",
          "shifted", "fold", "radices")


@pytest.mark.parametrize("name", list(WM.CLASSES))
def test_every_class_has_a_case(name):
    claimed = [c for c in WM.CASES if name in c["classes"]]
    assert claimed, f"no case claims the class {name!r}"
    for c in claimed:
        line = WM.line(c)
        assert WM.CLASSES[name](c, WM.parse(line)), f"case {c['id']} is not of the class {name!r}: {line}"


@pytest.mark.parametrize("cid,name", CLAIMS, ids=[f"{c}: {n}" for c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(cid, name):
    assert name in WM.CLASSES, f"case {cid} claims {name!r}, which is no class"
    c = WM.case(cid)
    line = WM.line(c)
    assert WM.CLASSES[name](c, WM.parse(line)), f"case {cid} is not of the class {name!r}: {line}"


def test_case_ids_are_unique_and_every_case_is_there_for_a_class():
    ids = WM.case_ids()
    assert len(set(ids)) == len(ids), ids
    assert all(c["classes"] for c in WM.CASES)
    assert set(WM.SHIFTED) <= set(ids)
    # a shifted case of each regime, an odd n in each, and 2025
    shifted = [WM.parse(WM.line(WM.case(cid), fftshift=True)) for cid in WM.SHIFTED]
    assert all(d["shifted"] for d in shifted)
    assert any(d["fy"] >= WM.CHUNK and d["n_fft"] % 2 for d in shifted) and any(d["fy"] < WM.CHUNK and d["n_fft"] % 2 for d in shifted)
    assert any(d["fy"] >= WM.CHUNK and d["n_fft"] % 2 == 0 for d in shifted) and any(d["fy"] < WM.CHUNK and d["n_fft"] % 2 == 0 for d in shifted)
    assert "n2025-detrend-1x35" in WM.SHIFTED


@pytest.mark.parametrize("cid", WM.case_ids())
def test_the_cases_have_the_frames_the_issue_names(cid):
    c = WM.case(cid)
    s, _, frames, _ = WM.desc(c)
    assert s.channels == 2 and s.y_stride == 0 and s.y_batch_stride == 0
    assert B.cmfft_supported(c["n_fft"]) and c["n_fft"] in WM.SIZES
    if "F" in c:
        assert frames == c["F"] == s.frames
    if cid == "n18-l16-1x131142":
        assert s.samples == 262300 and s.hop == 2 and s.batch == 1


def test_the_sizes_are_the_91():
    assert len(WM.SIZES) == 91 and sum(n % 2 for n in WM.SIZES) == 18
    assert WM.SIZES[0] == 18 and WM.SIZES[-1] == 2025


def test_the_planner_emits_no_regime_without_a_case():
    """The plan's shape is a function of n_fft alone; the frames and the batch only set the runs, the chunks, the blocks and the grid.
    Every n_fft the checks accept, at frame counts around a chunk, a run, a block and the grid cap: the regime (fy, groups per run,
    accumulators) is one a case has, the layout is the header's (lpf the smallest power of two >= n / 4 in 4..256, fy = 256 / lpf, a
    power of two), the schedule is the forward call's, the runs cover every signal's padded frame axis once and never cross a signal,
    and the workspace is the header's formula."""
    p = WM.params(4)
    covered = {WM.regime(WM.parse(WM.line(c))) for c in WM.CASES}
    seen = set()
    for n in WM.SIZES:
        lpf, fy = WM.layout(n)
        for F in (1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, 513, 4097, 16 * 2048, 16 * 2048 + 1, 32 * 2048 + 1, 140000):
            if F * n > 1 << 33:
                continue
            for nb in (1, 3):
                if nb * F * n > 1 << 34:
                    continue
                for det, sh in ((False, False), (True, True)):
                    s = B.make_stft(nb, (F - 1) * 3 + n, F, 3, n, channels=2, shift=31)
                    d = WM.parse(B.describe_welch_cmfft(p, n, s, detrend=det, fftshift=sh))
                    assert WM.regime(d) in covered, d["line"]
                    assert (d["lpf"], d["fy"]) == (lpf, fy) and fy & (fy - 1) == 0 and d["shifted"] == sh and d["detrend"] == det
                    assert d["schedule"] == WM.schedule(n) and d["cpl"] == -(-n // lpf) <= 8
                    assert d["fold"] == (n if n % 2 else n // 2) and d["lds"] == 2 * fy * n * 8 + d["fold"] * 8 + fy * 8
                    assert d["chunk"] == WM.CHUNK and d["run"] == max(WM.CHUNK, fy) and d["gpr"] == d["run"] // fy == max(1, WM.CHUNK // fy)
                    assert d["acc"] == (0 if fy >= WM.CHUNK else -(-n // 256)) <= 8
                    fpad = -(-F // d["run"]) * d["run"]
                    assert d["runs"] == nb * fpad // d["run"] and d["groups"] == d["runs"] * d["gpr"] == nb * fpad // fy
                    assert d["grid"] == min(d["runs"], WM.MAX_GRID)
                    assert d["chunks"] == -(-F // WM.CHUNK) and d["blocks"] == -(-F // WM.BLOCK)
                    assert d["joins"] == (2 if d["blocks"] > 1 else 1)
                    assert d["workspace"] == 8 * WM.workspace_doubles(nb, F, n) == B.welch_cmfft_workspace_bytes(s)
                    seen.add(WM.regime(d))
    assert seen == covered                          # and no case is of a regime the planner would not emit


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("cid", WM.case_ids())
def test_the_shared_fields_are_describe_stft_cmffts(cid, shifted):
    c = WM.case(cid)
    s, L, _, det = WM.desc(c)
    p = WM.params(c["setup"])
    w = WM.parse(B.describe_welch_cmfft(p, L, s, detrend=det, fftshift=shifted))
    f = MC.parse(B.describe_stft_cmfft(p, L, s, detrend=det, fftshift=shifted))
    for name in SHARED:
        assert w[name] == f[name], (cid, name, w["line"], f["line"])
    assert not w["power"]
    # the same words around them: the text from the signals to the columns per lane (the groups and the grid are recounted)
    cut = lambda t: t[t.index(" signals x"):t.index(" groups, grid")].rsplit(",", 1)[0]
    assert cut(w["line"]) == cut(f["line"])
    # and before them, but for the call's name and the output form, which this call has not
    head = lambda t, name: t[:t.index(": k_")].replace(name, "X")
    assert head(w["line"], "welch cmfft") == head(f["line"], "stft cmfft").replace(", spectrum rows", "")
    assert {k.replace("welch_cmfft", "stft_cmfft"): a for k, a in w["kernels"].items() if k != "k_welch_fft_join"} == f["kernels"]


def test_unsupported_sizes_have_no_plan():
    p = WM.params(4)
    for n in (8, 14, 15, 16, 17, 21, 64, 448, 512, 2048, 2160, 4050):
        with pytest.raises(B.BhwError) as e:
            B.describe_welch_cmfft(p, min(n, 8), B.make_stft(1, 100000, 3, 7, n, channels=2, shift=31))
        assert e.value.code == -2, e.value                 # BHW_ERR_UNSUPPORTED
