"""The case table of tests/welch_mfft_cases.py reaches every plan class of the fused Welch PSD at a mixed-radix n_fft: every class has a
case, every claim holds on the describe line of its case (host arithmetic, no GPU), a sweep of the planner over all 95 supported n_fft
and over frame counts at the edges of a chunk, a run, a block and the grid emits no shape the table's cases do not hold, and the
fields the line shares with bhw_describe_stft_mfft are that call's."""
import pytest

from blackman_harris_win_amd import binding as B

import stft_mfft_cases as SM
import welch_mfft_cases as WC

CLAIMS = [(c["id"], name) for c in WC.CASES for name in c["classes"]]
SHARED = ("signals", "frames", "rows", "n_fft", "m", "lpf", "fy", "cpl", "lds", "L", "col0", "pad", "schedule", "detrend", "reflect", "table")
SUPPORTED = [n for n in range(B.MFFT_MIN_N, B.MFFT_MAX_N + 1) if B.mfft_supported(n)]


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


@pytest.mark.parametrize("cid", WC.case_ids())
def test_the_cases_have_the_frames_the_table_names(cid):
    c = WC.case(cid)
    s, _, frames, _ = WC.desc(c)
    if "F" in c:
        assert frames == c["F"] == s.frames
    if cid == "n18-1x131142":
        assert s.samples == 262300


def test_there_are_95_supported_sizes():
    assert len(SUPPORTED) == 95 and SUPPORTED[0] == 18 and SUPPORTED[-1] == 4050


def test_the_planner_emits_no_shape_without_a_case():
    """The plan's shape is a function of n_fft alone; the frames and the batch only set the runs, the chunks, the blocks and the grid.
    Every n_fft the checks accept, at frame counts around a chunk, a run, a block and the grid cap: the shape is one a case has, the
    runs cover every signal's padded frame axis once and never cross a signal, and the workspace is the header's formula."""
    p = WC.params(4)
    covered = {WC.shape(WC.parse(WC.line(c))) for c in WC.CASES}
    seen = set()
    for n in SUPPORTED:
        K = n // 2 + 1
        for F in (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 513, 4096, 4097, 16 * 2048, 16 * 2048 + 1, 70000):
            for nb in (1, 3):
                for det in (False, True):
                    s = B.make_stft(nb, (F - 1) * 3 + n, F, 3, n, shift=31)
                    d = WC.parse(B.describe_welch_mfft(p, n, s, detrend=det))
                    assert WC.shape(d) in covered, d["line"]
                    assert d["fy"] in (1, 2, 4, 8, 16, 32, 64) and d["fy"] == (64 if n <= 32 else d["fy"]) and (n < 1080 or d["fy"] == 1)
                    assert d["chunk"] == WC.CHUNK and d["run"] == max(WC.CHUNK, d["fy"]) and d["gpr"] == d["run"] // d["fy"]
                    assert d["acc"] == (0 if d["fy"] >= WC.CHUNK else -(-K // 256)) <= 8
                    fpad = -(-F // d["run"]) * d["run"]
                    assert d["runs"] == nb * fpad // d["run"] and d["groups"] == d["runs"] * d["gpr"] == nb * fpad // d["fy"]
                    assert d["grid"] == min(d["runs"], WC.MAX_GRID)
                    assert d["chunks"] == -(-F // WC.CHUNK) and d["blocks"] == -(-F // WC.BLOCK)
                    assert d["joins"] == (2 if d["blocks"] > 1 else 1)
                    assert d["workspace"] == 8 * WC.workspace_doubles(nb, F, K) == B.welch_mfft_workspace_bytes(s)
                    seen.add(WC.shape(d))
    assert seen == covered                          # and no case is of a shape the planner would not emit


def test_bin_m_is_taken_aside_at_three_sizes():
    """M a multiple of 256: n_fft 1536, 2560 and 3072.  (n_fft 3840 has M = 1920 = 7.5 x 256: bin M is lane 128's in the eighth trip.)"""
    assert [n for n in SUPPORTED if (n // 2) % 256 == 0] == [1536, 2560, 3072]
    assert (3840 // 2) % 256 == 128 and B.mfft_supported(3840)


@pytest.mark.parametrize("cid", WC.case_ids())
def test_the_shared_fields_are_describe_stft_mffts(cid):
    c = WC.case(cid)
    s, L, _, det = WC.desc(c)
    p = WC.params(c["setup"])
    w, f = WC.parse(B.describe_welch_mfft(p, L, s, detrend=det)), SM.parse(B.describe_stft_mfft(p, L, s, detrend=det))
    for name in SHARED:
        assert w[name] == f[name], (cid, name, w["line"], f["line"])
    assert w["form"] is None and f["form"] == "spectrum"               # the line has no output form
    # the same words around them: the text from the kernel's name to the LDS bytes, but for the groups and the grid, which are recounted
    cut = lambda t: t[t.index(" signals x"):t.index(" groups, grid")].rsplit(",", 1)[0]
    assert cut(w["line"]) == cut(f["line"])
    assert {k.replace("welch_mfft", "stft_mfft"): a for k, a in w["kernels"].items() if k != "k_welch_fft_join"} == f["kernels"]


def test_unsupported_sizes_have_no_plan():
    p = WC.params(4)
    for n in (8, 14, 15, 17, 22, 128, 512, 4096, 8192):
        with pytest.raises(B.BhwError) as e:
            B.describe_welch_mfft(p, min(n, 8), B.make_stft(1, 100000, 3, 7, n, shift=31))
        assert e.value.code == -2, e.value                 # BHW_ERR_UNSUPPORTED
