"""The fused log spectrogram / MFCC without a GPU: the case table's coverage (every class of tests/logspec_cases.py has a case, every
claim holds, the describe line's plan fields are the parent's for the same call), bhw.dct_weights against an independent scalar
restatement, and the numpy restatement of the contract (logspec_cases.log_ref / dct_ref, what the GPU test compares with) against a
float64 MFCC computed from x on noise, next to a float32 stand-in held to the end-to-end bound of the GPU test."""
import math

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd.selector import fbank_bands

import logspec_cases as LC
import spectrogram_cases as SC
import stft_mfft_cases as MC


def test_every_class_has_a_case_and_every_claim_holds():
    claimed = set()
    for c in LC.CASES:
        d = LC.parse(LC.line(c))
        assert d["W"] == LC.width(c) and d["n_fft"] == c["base"]["n_fft"], d["line"]
        assert ("k_logspec_direct" if c["family"] == "pow2" else "k_logspec_mfft_direct") in d["kernels"], d["line"]
        assert d["rows_form"] == ("power" if c["bank"] is None else "bank") and (d["dct"] is None) == (c["coeffs"] == 0)
        mult, floor, add = LC.log_args(c)
        assert (d["mode"], d["floor"], d["mult"]) == ("add" if add else "clamp", floor, mult), d["line"]
        for name in c["classes"]:
            assert LC.CLASSES[name](c, d), (c["id"], name, d["line"])
            claimed.add(name)
    assert claimed == set(LC.CLASSES), set(LC.CLASSES) - claimed
    assert len(set(LC.case_ids())) == len(LC.CASES)


def test_the_parents_tables_are_carried_whole():
    ids = set(LC.case_ids())
    for base in SC.CASES:
        assert "p2-" + base["id"] + "-log" in ids
        assert (base.get("bank") is None) != ("p2-" + base["id"] + "-dct" in ids)
    mixed = [c for c in MC.CASES if c.get("form") in ("power", "bank")]
    assert len(mixed) >= 3
    for base in mixed:
        assert "mx-" + base["id"] + "-log" in ids
        assert (base["form"] == "bank") == ("mx-" + base["id"] + "-dct" in ids)
    for c in LC.CASES:                                                # imported, not edited
        if c["id"].startswith("p2-"):
            assert c["base"] is SC.case(c["base"]["id"])
        if c["id"].startswith("mx-"):
            assert c["base"] is MC.case(c["base"]["id"])
        if c["coeffs"]:
            assert LC.bank(c).shape[1] <= c["base"]["n_fft"] and LC.dct(c).shape == (LC.bank(c).shape[1], c["coeffs"])
    have = {name for c in LC.CASES if c["family"] == "pow2" for name in c["base"].get("classes", ())}
    assert set(LC.PARENT_CLASSES_POW2) <= have, set(LC.PARENT_CLASSES_POW2) - have
    have = {name for c in LC.CASES if c["family"] == "mixed" for name in c["base"].get("classes", ())}
    assert set(LC.PARENT_CLASSES_MIXED) <= have, set(LC.PARENT_CLASSES_MIXED) - have


@pytest.mark.parametrize("cid", LC.case_ids())
def test_the_plan_fields_are_the_parents(cid):
    c = LC.case(cid)
    mine, parent = LC.line(c), LC.parent_line(c)
    assert LC.plan_text(mine) == LC.plan_text(parent), (mine, parent)
    dm, dp = LC.parse(mine), LC.parse(parent)
    for f in ("signals", "frames", "rows", "n_fft", "m", "lpf", "fy", "cpl", "groups", "grid", "lds", "L", "col0", "pad", "schedule", "detrend", "reflect"):
        assert dm[f] == dp[f], (f, mine, parent)


@pytest.mark.parametrize("n_coeffs,n_mels,norm", [(13, 80, "ortho"), (13, 80, None), (40, 40, "ortho"), (1, 10, "ortho"), (20, 128, None), (7, 1, "ortho")])
def test_dct_weights_against_a_scalar_restatement(n_coeffs, n_mels, norm):
    d = bhw.dct_weights(n_coeffs, n_mels, norm=norm)
    assert d.shape == (n_mels, n_coeffs) and d.dtype == np.float32 and d.flags.c_contiguous
    want = np.empty((n_mels, n_coeffs), dtype=np.float32)
    for m in range(n_mels):
        for j in range(n_coeffs):
            v = math.cos(math.pi * (2 * m + 1) * j / (2 * n_mels))           # another grouping of the same angle
            if norm is None:
                v *= 2.0
            else:
                v *= math.sqrt(2.0 / n_mels) * (math.sqrt(0.5) if j == 0 else 1.0)
            want[m, j] = np.float32(v)
    near = np.abs(want) > 1e-6                                                # at a zero of the cosine an ulp of the value means nothing
    assert LC.ulps_apart(d[near], want[near]).max() <= 1
    # there the two groupings differ by the rounding of the angle: a few ulps of an angle below pi * n_coeffs, times a scale of 2 at most
    assert np.abs(d[~near].astype(np.float64) - want[~near]).max(initial=0.0) <= 16 * math.pi * n_coeffs * 2.0 ** -53
    with pytest.raises(ValueError, match="norm"):
        bhw.dct_weights(13, 80, norm="slaney")
    with pytest.raises(ValueError, match=">= 1"):
        bhw.dct_weights(0, 80)


def test_the_restatements_edges():
    q = np.array([0.0, 1e-12, 1e-10, 2.0, np.inf, np.nan, -3.0], dtype=np.float32)
    g = LC.log_ref(q, 1.0, 1e-10, False)
    lf = np.float32(math.log(1e-10))
    assert g[0] == lf and g[1] == lf and g[6] == lf and g[3] == np.float32(math.log(2.0)) and g[4] == np.inf and np.isnan(g[5])
    g = LC.log_ref(q, -2.0, 0.5, True)
    assert g[0] == np.float32(-2.0 * math.log(0.5)) and g[4] == -np.inf and np.isnan(g[5]) and np.isnan(g[6])
    assert LC.ulps_apart(np.float32([1.0, -0.0, np.nan]), np.float32([np.nextafter(np.float32(1), np.float32(2)), 0.0, np.nan])).tolist() == [1, 0, 0]
    eye = np.eye(5, dtype=np.float32)
    rows = np.random.default_rng(1).standard_normal((4, 5)).astype(np.float32)
    assert np.array_equal(LC.dct_ref(rows, eye), rows)


def _bank_chain(P, w):
    """The bank contract: per filter over its band in ascending i, float64 from +0.0, rounded once."""
    first, offset, weight = fbank_bands(w)
    out = np.zeros((P.shape[0], w.shape[1]), dtype=np.float32)
    P64 = P.astype(np.float64)
    for m in range(w.shape[1]):
        acc = np.zeros(P.shape[0])
        for i in range(int(offset[m]), int(offset[m + 1])):
            acc = acc + P64[:, int(first[m]) + i - int(offset[m])] * float(weight[i])
        out[:, m] = acc.astype(np.float32)
    return out


def log_domain_error(got, ref):
    """The end-to-end metric: per row the largest |got - ref|, then the largest row."""
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max(axis=-1).max())


@pytest.mark.parametrize("n_fft,L,hop", [(400, 400, 160), (512, 400, 160)])
def test_the_restatement_against_a_float64_mfcc_from_x(n_fft, L, hop):
    """Noise scaled so the powers sit far above the floor, 80 mel, 13 coefficients, log = ln(q + 1e-6).  Reference: float64 from x.
    The restatement runs on the correctly rounded float32 spectrum (a stand-in for the kernel's float32 FFT); the yardstick is the
    float32 torch route on the CPU, and the bound the project's 2x."""
    import torch
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 8000)) * 100 + 5).astype(np.float32)
    n = np.arange(L, dtype=np.float64)
    win = np.zeros(n_fft, dtype=np.float32)
    win[(n_fft - L) // 2:(n_fft - L) // 2 + L] = (0.5 - 0.5 * np.cos(2 * np.pi * n / L)).astype(np.float32)
    mel, dct = bhw.mel_weights(n_fft, 80, 16000), bhw.dct_weights(13, 80)
    xp = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    frames = 1 + (xp.shape[1] - n_fft) // hop
    rows = np.stack([xp[:, f * hop:f * hop + n_fft] for f in range(frames)], axis=1) * win               # float32 * float32
    assert rows.dtype == np.float32
    Y = np.fft.rfft(rows.astype(np.float64), axis=-1)
    ref = np.log((np.abs(Y) ** 2) @ mel.astype(np.float64) + 1e-6) @ dct.astype(np.float64)
    Yf = Y.astype(np.complex64)
    re, im = Yf.real.astype(np.float64), Yf.imag.astype(np.float64)
    P = (re * re + im * im).astype(np.float32).reshape(-1, n_fft // 2 + 1)
    got = LC.dct_ref(LC.log_ref(_bank_chain(P, mel), 1.0, 1e-6, True), dct).reshape(ref.shape)
    S = torch.stft(torch.from_numpy(x), n_fft, hop, n_fft, window=torch.from_numpy(win), center=True, pad_mode="reflect", return_complex=True)
    route = torch.matmul(torch.log(torch.matmul((S.abs() ** 2).transpose(-1, -2), torch.from_numpy(mel)) + 1e-6), torch.from_numpy(dct)).numpy()
    err, yard = log_domain_error(got, ref), log_domain_error(route, ref)
    print(f"logspec restatement {n_fft} / {hop}: stand-in {err:.3e}, float32 torch route {yard:.3e}, ratio {err / yard:.3f}")
    assert got.shape == route.shape and err <= 2.0 * yard, (err, yard)
    assert err < 1e-4                                                          # the restatement IS the formula: float32 roundings only
