"""The case table of tests/csd_fft_cases.py reaches every plan class of the fused Welch cross spectra: every class has a case, every
claim holds on the describe line of its case (host arithmetic, no GPU), a sweep of the planner over every supported n_fft and over frame
counts at the edges of a chunk, a run, a block and the grid emits no shape the table's cases do not hold, and the fields the line shares
with bhw_describe_stft_fft are that call's -- but for the lanes of a row at n_fft 2048, where two operands side by side leave 128."""
import pytest

from blackman_harris_win_amd import binding as B

import stft_fft_cases as SF
import csd_fft_cases as CC

CLAIMS = [(c["id"], name) for c in CC.CASES for name in c["classes"]]
SHARED = ("signals", "frames", "rows", "n_fft", "m", "L", "col0", "pad", "schedule", "detrend", "reflect", "table")
LANES = ("lpf", "fy", "cpl", "lds")                 # equal to the forward call's up to n_fft 1024


@pytest.mark.parametrize("name", list(CC.CLASSES))
def test_every_class_has_a_case(name):
    claimed = [c for c in CC.CASES if name in c["classes"]]
    assert claimed, f"no case claims the class {name!r}"
    for c in claimed:
        line = CC.line(c)
        assert CC.CLASSES[name](c, CC.parse(line)), f"case {c['id']} is not of the class {name!r}: {line}"


@pytest.mark.parametrize("cid,name", CLAIMS, ids=[f"{c}: {n}" for c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(cid, name):
    assert name in CC.CLASSES, f"case {cid} claims {name!r}, which is no class"
    c = CC.case(cid)
    line = CC.line(c)
    assert CC.CLASSES[name](c, CC.parse(line)), f"case {cid} is not of the class {name!r}: {line}"


def test_case_ids_are_unique_and_every_case_is_there_for_a_class():
    ids = CC.case_ids()
    assert len(set(ids)) == len(ids), ids
    assert all(c["classes"] for c in CC.CASES)


@pytest.mark.parametrize("cid", CC.case_ids())
def test_the_cases_have_the_frames_the_issue_names(cid):
    c = CC.case(cid)
    s, _, frames, _ = CC.desc(c)
    if "F" in c:
        assert frames == c["F"] == s.frames
    if cid == "n16-1x131142":
        assert s.samples == 262298


def test_the_issues_shapes_are_all_there():
    have = {(c["n_fft"], c["L"], c["hop"], c["B"], c.get("F")) for c in CC.CASES}
    for shape in ((16, 16, 4, 2, 70), (32, 20, 8, 1, 16), (64, 64, 8, 3, 17), (128, 100, 32, 2, 33), (256, 200, 64, 2, 40),
                  (512, 400, 160, 3, 259), (64, 64, 16, 2, 600), (16, 16, 2, 1, 131142)):
        assert shape in have, shape
    assert any(c["n_fft"] == 1024 and (c["B"], c["F"]) == (1, 21) and c.get("padded") for c in CC.CASES)
    assert any(c["n_fft"] == 2048 and (c["B"], c["F"]) == (2, 18) for c in CC.CASES)
    assert any(c.get("F") == 1 for c in CC.CASES) and any(c.get("F") == 15 for c in CC.CASES)
    assert any(c["mode"] == "reflect" for c in CC.CASES) and any(c.get("bcast") for c in CC.CASES)


def _shape(d):
    return (d["n_fft"], d["schedule"], d["lpf"], d["fy"], d["cpl"], d["lds"], d["pairs"], d["run"], d["gpr"], d["acc"], d["chains"])


def test_the_planner_emits_no_shape_without_a_case():
    """The plan's shape is a function of n_fft alone; the frames and the batch only set the runs, the chunks, the blocks and the grid.
    Every n_fft the checks accept, at frame counts around a chunk, a run, a block and the grid cap: the shape is one a case has, the
    runs cover every signal's padded frame axis once and never cross a signal, and the workspace is the header's formula."""
    p = CC.params(4)
    covered = {_shape(CC.parse(CC.line(c))) for c in CC.CASES}
    seen = set()
    for lg in range(4, 12):
        n = 1 << lg
        K = n // 2 + 1
        for F in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 513, 4096, 4097, 16 * 2048, 16 * 2048 + 1, 32 * 2048 + 1, 70000):
            for nb in (1, 3):
                for det in (False, True):
                    s = B.make_stft(nb, (F - 1) * 3 + n, F, 3, n, shift=31)
                    d = CC.parse(B.describe_csd_fft(p, n, s, detrend=det, outputs=CC.ALL, broadcast_x=nb > 1 and det))
                    assert _shape(d) in covered, d["line"]
                    assert d["fy"] >= 2 and d["pairs"] == d["fy"] // 2 and d["lpf"] == min(128, max(4, n // 8)) and d["lpf"] * d["fy"] == 256
                    assert d["cpl"] == n // d["lpf"] <= 16 and d["lds"] == 2 * d["fy"] * (n // 2) * 8 + (n // 2) * 8 + d["fy"] * 4 <= 65536
                    assert d["chunk"] == CC.CHUNK and d["run"] == max(CC.CHUNK, d["pairs"]) and d["gpr"] == d["run"] // d["pairs"]
                    assert d["acc"] == (0 if d["pairs"] >= CC.CHUNK else -(-K // 256)) <= 5 and d["chains"] == 4
                    fpad = -(-F // d["run"]) * d["run"]
                    assert d["runs"] == nb * fpad // d["run"] and d["groups"] == d["runs"] * d["gpr"] == nb * fpad // d["pairs"]
                    assert d["grid"] == min(d["runs"], CC.MAX_GRID)
                    assert d["chunks"] == -(-F // CC.CHUNK) and d["blocks"] == -(-F // CC.BLOCK)
                    assert d["joins"] == (2 if d["blocks"] > 1 else 1)
                    assert d["workspace"] == 8 * CC.workspace_doubles(nb, F, K) == B.csd_fft_workspace_bytes(s) == 4 * B.welch_fft_workspace_bytes(s)
                    assert d["broadcast"] == (nb > 1 and det) and d["onesided"] and d["outputs"] == CC.ALL
                    seen.add(_shape(d))
    assert seen == covered                          # and no case is of a shape the planner would not emit


@pytest.mark.parametrize("cid", CC.case_ids())
def test_the_shared_fields_are_describe_stft_ffts(cid):
    c = CC.case(cid)
    s, L, _, det = CC.desc(c)
    p = CC.params(c["setup"])
    w, f = CC.parse(CC.line(c)), SF.parse(B.describe_stft_fft(p, L, s, detrend=det))
    for name in SHARED:
        assert w[name] == f[name], (cid, name, w["line"], f["line"])
    if c["n_fft"] <= 1024:
        for name in LANES:
            assert w[name] == f[name], (cid, name, w["line"], f["line"])
        # the same words around them: the text from the kernel's name to the LDS bytes, but for the groups and the grid, which are recounted
        cut = lambda t: t[t.index(" signals x"):t.index(" groups, grid")].rsplit(",", 1)[0]
        assert cut(w["line"]) == cut(f["line"])
    else:                                           # the documented difference: 128 lanes a row, two rows, as n_fft 4096 runs forward
        assert (f["lpf"], f["fy"], f["cpl"]) == (256, 1, 8) and (w["lpf"], w["fy"], w["cpl"], w["lds"]) == (128, 2, 16, 40968)
    assert {k.replace("csd_fft", "stft_fft"): a for k, a in w["kernels"].items() if k.startswith("k_csd_fft_d") or k.startswith("k_csd_fft_t")} == f["kernels"]
    # the welch line of the same call has the same chunks, blocks and a quarter of the workspace
    import welch_fft_cases as WC
    wl = WC.parse(B.describe_welch_fft(p, L, s, detrend=det))
    assert (w["chunks"], w["blocks"], w["workspace"]) == (wl["chunks"], wl["blocks"], 4 * wl["workspace"])


def test_unsupported_sizes_have_no_plan():
    p = CC.params(4)
    for n in (8, 15, 17, 100, 400, 4096, 8192):
        with pytest.raises(B.BhwError) as e:
            B.describe_csd_fft(p, min(n, 8), B.make_stft(1, 100000, 3, 7, n, shift=31))
        assert e.value.code == -2, e.value                 # BHW_ERR_UNSUPPORTED
