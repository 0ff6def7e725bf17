"""The fused Welch cross spectra on the GPU (bhw_csd_fft_f32_* through bhw.csd_fft, bhw.cross_spectra_fused, the one-output forms and
their ResidentTable forms).

The gate is exact.  include/bhw.h defines the outputs on the float32 pairs bhw_stft_fft_f32_* writes for x and for y: the four terms in
binary64 (one rounding each), each summed over the frames in chunks of 16, the chunks of a block of 256 frames in order, then the
blocks in order, then the output formulas of bhw_welch_csd_f32.  For every case of tests/csd_fft_cases.py, library and table, every
output must equal that restated in torch float64 on bhw.stft(x) and bhw.stft(y) of the same call, word for word: every step of the
restatement is an IEEE elementwise operation, so there is no tolerance.  Around it: pxx / pyy against welch_fft, the agreement with
welch_csd(stft(x), stft(y)) (bit for bit up to 16 frames, the derived bound beyond), the identities of csd_fft(x, x), independence of
the batch and the form, untouched gaps, zeros, NaN containment, graph capture, the end-to-end accuracy bound of test_gpu_csd.py, and
the Python errors."""
import ctypes

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from test_gpu_welch_fft import _signal, _pad_axis, _bits, _capture
from test_gpu_csd import _cross_ref64, _torch_route, _pair, _v

import csd_fft_cases as CC

pytestmark = pytest.mark.gpu

CHUNK, BLOCK = B.WELCH_FFT_CHUNK, B.WELCH_BLOCK
SENTINEL = 12345.5
ALL = CC.ALL


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _words(t):
    import torch
    t = t.contiguous()
    return torch.view_as_real(t).view(torch.int32) if t.is_complex() else t.view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((_words(a) == _words(b)).all())


def _all_nan(t):
    import torch
    return bool(torch.isnan(torch.view_as_real(t) if t.is_complex() else t).all())


def _same_all(got, want, names=None):
    names = list(want) if names is None else names
    return [n for n in names if not _same_bits(got[n], want[n])]


def _ordered_sum(torch, t):
    """include/bhw.h's order on t (B, F, K) float64: 16 explicit adds over the frames of every chunk, 16 over the chunks of every block,
    one per block, each from +0.0.  Appended +0.0 terms change no bit of a sum that starts from +0.0."""
    nb, F, K = t.shape
    tc = _pad_axis(torch, t, 1, CHUNK).view(nb, -1, CHUNK, K)
    A_chunk = torch.zeros((nb, tc.shape[1], K), dtype=torch.float64, device=t.device)
    for i in range(CHUNK):
        A_chunk = A_chunk + tc[:, :, i, :]
    cb = _pad_axis(torch, A_chunk, 1, BLOCK // CHUNK).view(nb, -1, BLOCK // CHUNK, K)
    A_blk = torch.zeros((nb, cb.shape[1], K), dtype=torch.float64, device=t.device)
    for j in range(BLOCK // CHUNK):
        A_blk = A_blk + cb[:, :, j, :]
    A = torch.zeros((nb, K), dtype=torch.float64, device=t.device)
    for blk in range(A_blk.shape[1]):
        A = A + A_blk[:, blk, :]
    return A


def _restate(torch, X, Y, scale, n_fft, onesided):
    """The contract on the spectrum rows X (B or 1, F, K) and Y (B, F, K) complex64, in torch float64 on the device: a dict of all
    five outputs (B, K)."""
    X = X if X.dim() == 3 else X.unsqueeze(0)
    Y = Y if Y.dim() == 3 else Y.unsqueeze(0)
    X = X.expand_as(Y)
    xr, xi, yr, yi = X.real.double(), X.imag.double(), Y.real.double(), Y.imag.double()
    # every product is exact in binary64, so each term is one rounding
    sxx = _ordered_sum(torch, xr * xr + xi * xi)
    syy = _ordered_sum(torch, yr * yr + yi * yi)
    cre = _ordered_sum(torch, xr * yr + xi * yi)
    cim = _ordered_sum(torch, xr * yi - xi * yr)
    K = Y.shape[-1]
    sk = torch.full((K,), float(scale), dtype=torch.float64, device=Y.device)
    if onesided:
        sk[1:] = float(scale) * 2.0
        if n_fft % 2 == 0:
            sk[-1] = float(scale)
    n, m = cre * cre, cim * cim
    return {"pxy": torch.complex((cre * sk).float(), (cim * sk).float()), "pxx": (sxx * sk).float(), "pyy": (syy * sk).float(),
            "coherence": ((n + m) / (sxx * syy)).float(), "h1": torch.complex((cre / sxx).float(), (cim / sxx).float())}


def _kw(c):
    if c["detrend"]:
        return dict(win_length=c["L"], center=False, detrend=True)
    return dict(win_length=c["L"], center=bool(c["mode"]), pad_mode=c["mode"] or "reflect", detrend=False)


def _case_xy(torch, c, seed=0):
    """x and y of a case: y is a delayed, scaled copy of x plus noise of its own (a response to the excitation x).  Broadcast cases
    have a 1-D x; one-signal cases are 1-D now and then."""
    T = CC.frames_to_samples(c)
    x = _signal(torch, 1 if c.get("bcast") else c["B"], T, seed)
    y = 0.5 * torch.roll(x, 3, dims=-1).expand(c["B"], T) + 0.1 * _signal(torch, c["B"], T, seed + 500)
    if c.get("bcast"):
        return x[0], y.contiguous()
    if c["B"] == 1 and seed % 2:
        return x[0], y[0].contiguous()
    return x, y.contiguous()


_REFS = {}


def _case_ref(torch, cid):
    """(p, x, y, X, Y, F) of a case, computed once and shared by the tests that need it; nothing changes them."""
    if cid not in _REFS:
        c = CC.case(cid)
        p = CC.params(c["setup"])
        x, y = _case_xy(torch, c, seed=CC.case_ids().index(cid))
        X = bhw.stft(p, x, c["n_fft"], c["hop"], **_kw(c))
        Y = bhw.stft(p, y, c["n_fft"], c["hop"], **_kw(c))
        _REFS[cid] = (p, x, y, X, Y, CC.desc(c)[2])
    return _REFS[cid]


# ---- the gate ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", CC.case_ids())
def test_word_for_word_equal_to_the_contract_on_stft_rows(torch, cid):
    c = CC.case(cid)
    p, x, y, X, Y, F = _case_ref(torch, cid)
    K = c["n_fft"] // 2 + 1
    assert Y.shape[-2:] == (F, K) and X.shape[-2:] == (F, K)
    for onesided, scale in ((True, 1.0 / (3.7 * F)), (False, 0.37)):
        want = _restate(torch, X, Y, scale, c["n_fft"], onesided)
        if y.dim() == 1:
            want = {n: t[0] for n, t in want.items()}
        out = None
        if c.get("padded"):
            bufs = {n: torch.full((c["B"], K + 5), SENTINEL, dtype=want[n].dtype, device="cuda") for n in ALL}
            out = {n: (b[:, :K] if y.dim() == 2 else b[0, :K]) for n, b in bufs.items()}
        got = bhw.csd_fft(p, x, y, c["n_fft"], c["hop"], scale, outputs=ALL, onesided_doubling=onesided, out=out, **_kw(c))
        if out is not None:
            for n, b in bufs.items():
                assert got[n].data_ptr() == b.data_ptr() and bool((b[:, K:] == SENTINEL).all()), ("a gap was written", n)
        assert set(got) == set(ALL)
        bad = _same_all(got, want)
        for n in bad:
            print(cid, "library", onesided, n, "differing words:", int((_words(got[n]) != _words(want[n])).sum()))
        assert not bad, (cid, "library", onesided, bad)
        with bhw.ResidentTable(p) as tab:
            d = CC.parse(CC.line(c, table=tab._live()))
            assert d["table"] and d["frames"] == F
            tb = tab.csd_fft(p, x, y, c["n_fft"], c["hop"], scale, outputs=ALL, onesided_doubling=onesided, **_kw(c))
            bad = _same_all(tb, want)
            assert not bad, (cid, "table", onesided, bad)
        # any non-empty subset in one call: the same words
        sub = ("coherence", "pxy") if onesided else ("h1",)
        part = bhw.csd_fft(p, x, y, c["n_fft"], c["hop"], scale, outputs=sub, onesided_doubling=onesided, **_kw(c))
        assert set(part) == set(sub) and not _same_all(part, want, sub), (cid, sub)


@pytest.mark.parametrize("cid", CC.case_ids())
def test_pxx_and_pyy_are_welch_fft_of_x_and_of_y(torch, cid):
    c = CC.case(cid)
    p, x, y, _, _, _ = _case_ref(torch, cid)
    got = bhw.csd_fft(p, x, y, c["n_fft"], c["hop"], 0.125, outputs=("pxx", "pyy"), **_kw(c))
    px = bhw.welch_fft(p, x, c["n_fft"], c["hop"], 0.125, **_kw(c))
    py = bhw.welch_fft(p, y, c["n_fft"], c["hop"], 0.125, **_kw(c))
    assert _same_bits(got["pyy"], py), cid
    if c.get("bcast"):
        assert all(_same_bits(got["pxx"][b], px) for b in range(c["B"])), cid
    else:
        assert _same_bits(got["pxx"], px), cid


@pytest.mark.parametrize("cid", CC.case_ids())
def test_against_the_two_call_route(torch, cid):
    """welch_csd(stft(x), stft(y)) sums plain blocks of 256 frames.  Up to 16 frames that is this call's order: every output bit for
    bit.  Beyond, both orders add F products that are exact in binary64, so C_re (C_im) of the two differ by at most 2 F 2^-53 sum
    |term| <= 2 F 2^-53 sqrt(S_xx S_yy) (Cauchy-Schwarz); times s_k that is 2 F 2^-53 sqrt(P_xx P_yy), taken from the route's own
    pxx and pyy, plus the two final roundings: one float32 ulp of the larger result.  The bound of include/bhw.h, as it stands there."""
    c = CC.case(cid)
    p, x, y, X, Y, F = _case_ref(torch, cid)
    scale = 1.0 / (3.7 * F)
    route = bhw.welch_csd(X, Y, scale, nfft=c["n_fft"], onesided=True, outputs=ALL)
    got = bhw.csd_fft(p, x, y, c["n_fft"], c["hop"], scale, outputs=ALL, **_kw(c))
    if F <= CHUNK:
        assert not _same_all(got, route), (cid, _same_all(got, route))
        return
    slack = 2.0 * F * 2.0 ** -53 * torch.sqrt(route["pxx"].double() * route["pyy"].double())
    worst = 0.0
    for part in ("real", "imag"):
        a, b = getattr(got["pxy"], part), getattr(route["pxy"], part)
        big = torch.maximum(a.abs(), b.abs())
        ulp = (torch.nextafter(big, torch.full_like(big, float("inf"))) - big).double()
        diff = (a.double() - b.double()).abs()
        bound = slack + ulp
        worst = max(worst, float((diff / bound).max()))
        assert bool((diff <= bound).all()), (cid, part, float((diff / bound).max()))
    print(f"{cid}: F = {F}, pxy against welch_csd(stft, stft): worst |diff| / bound = {worst:.3f}")


# ---- identities --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", ["n16-2x70", "n128-l100-detrend-2x33", "n512-l400-3x259", "n2048-2x18"])
def test_x_against_itself(torch, cid):
    c = CC.case(cid)
    p, x, _, _, _, F = _case_ref(torch, cid)
    got = bhw.csd_fft(p, x, x, c["n_fft"], c["hop"], 1.0 / F, outputs=ALL, **_kw(c))
    assert _same_bits(got["pxx"], got["pyy"]) and bool((got["pxx"] > 0).all())
    assert _same_bits(got["pxy"].real, got["pxx"]) and bool((_bits(got["pxy"].imag) == 0).all()), cid       # (pxx, +0.0)
    assert bool((got["coherence"] == 1.0).all()), cid
    assert bool((got["h1"].real == 1.0).all()) and bool((_bits(got["h1"].imag) == 0).all()), cid


@pytest.mark.parametrize("n_fft,L,hop,F", [(64, 50, 16, 40), (512, 400, 160, 40), (2048, 2048, 512, 20)])
def test_a_pair_alone_and_as_pair_37_of_64_give_the_same_words(torch, n_fft, L, hop, F):
    p = CC.params(0)
    T = (F - 1) * hop + n_fft
    x = _signal(torch, 64, T, n_fft)
    y = (0.25 * x + _signal(torch, 64, T, n_fft + 1)).contiguous()
    kw = dict(win_length=L, detrend=False, outputs=ALL)
    P64 = bhw.csd_fft(p, x, y, n_fft, hop, 0.01, **kw)
    one = bhw.csd_fft(p, x[37], y[37], n_fft, hop, 0.01, **kw)
    assert one["pxy"].shape == (n_fft // 2 + 1,) and not _same_all(one, {n: t[37] for n, t in P64.items()})
    one = bhw.csd_fft(p, x[37:38], y[37:38], n_fft, hop, 0.01, **kw)
    assert not _same_all({n: t[0] for n, t in one.items()}, {n: t[37] for n, t in P64.items()})
    # x[37] broadcast against all of y: pair 37 is the same pair
    bc = bhw.csd_fft(p, x[37], y, n_fft, hop, 0.01, **kw)
    assert not _same_all({n: t[37] for n, t in bc.items()}, {n: t[37] for n, t in P64.items()})
    with bhw.ResidentTable(p) as tab:
        assert not _same_all(tab.csd_fft(p, x, y, n_fft, hop, 0.01, **kw), P64)
        assert not _same_all(tab.csd_fft(p, x[37], y[37], n_fft, hop, 0.01, **kw), {n: t[37] for n, t in P64.items()})


# ---- gaps, zeros, specials ---------------------------------------------------------------------------------------------------------------

def test_sentinels_survive_in_gaps_behind_the_workspace_and_in_outputs_not_asked_for(torch):
    c = CC.case("n64-3x17")
    p, x, y, _, _, _ = _case_ref(torch, "n64-3x17")
    K, nb = 33, 3
    s = CC.desc(c)[0]
    need = B.csd_fft_workspace_bytes(s) // 8
    ws = torch.full((need + 3,), SENTINEL, dtype=torch.float64, device="cuda")
    want = bhw.csd_fft(p, x, y, 64, c["hop"], 0.5, outputs=("pxy", "coherence"), **_kw(c))
    bufs = {n: torch.full((nb, K + 7), SENTINEL, dtype=want[n].dtype, device="cuda") for n in want}
    got = bhw.csd_fft(p, x, y, 64, c["hop"], 0.5, outputs=("pxy", "coherence"), out={n: b[:, :K] for n, b in bufs.items()}, workspace=ws,
                      **_kw(c))
    assert not _same_all(got, want)
    assert all(bool((b[:, K:] == SENTINEL).all()) for b in bufs.values()) and bool((ws[-3:] == SENTINEL).all())
    with pytest.raises(ValueError, match="workspace"):
        bhw.csd_fft(p, x, y, 64, c["hop"], 0.5, workspace=ws[:need - 4], **_kw(c))
    # the raw call with all five pointers given and two outputs asked for: the other three buffers keep every word
    five = [torch.full((nb, K), SENTINEL, dtype=torch.complex64 if B.CSD_OUTPUTS[n][1] else torch.float32, device="cuda") for n in B.CSD_OUTPUTS]
    xs = x.contiguous()
    s = B.make_stft(nb, xs.shape[1], 17, c["hop"], 64, shift=p.dat_width - 1, x_stride=xs.stride(0))
    flags = B.csd_mask(("pxy", "coherence")) | B.CSD_ONESIDED
    B.check(B.lib().bhw_csd_fft_f32_device(ctypes.byref(p), 64, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(s), 0,
                                           0.5, flags, ctypes.c_void_p(xs.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                                           *[ctypes.c_void_p(t.data_ptr()) for t in five], 0, ctypes.c_void_p(ws.data_ptr()), need * 8))
    torch.cuda.synchronize()
    for n, t in zip(B.CSD_OUTPUTS, five):
        if n in want:
            assert _same_bits(t, want[n]), n
        else:
            assert bool(t.eq(SENTINEL).all()), n                      # a complex buffer holds (SENTINEL, 0) in every element


@pytest.mark.parametrize("cid", ["n16-2x70", "n256-l200-detrend-2x40", "n512-l400-3x259", "n2048-2x18"])
def test_zeros_in_give_positive_zero_pxy_and_nan_coherence(torch, cid):
    c = CC.case(cid)
    p = CC.params(c["setup"])
    z = torch.zeros((c["B"], CC.frames_to_samples(c)), device="cuda")
    got = bhw.csd_fft(p, z, z.clone(), c["n_fft"], c["hop"], 0.25, outputs=ALL, **_kw(c))
    assert bool((_words(got["pxy"]) == 0).all()) and bool((_bits(got["pxx"]) == 0).all()) and bool((_bits(got["pyy"]) == 0).all()), cid
    assert _all_nan(got["coherence"]) and _all_nan(got["h1"]), cid


@pytest.mark.parametrize("cid", ["n64-3x17", "n512-l400-3x259", "n2048-2x18"])
def test_one_nan_in_y_poisons_exactly_the_bins_of_its_own_signal(torch, cid):
    c = CC.case(cid)
    p, x, y, _, _, _ = _case_ref(torch, cid)
    clean = bhw.csd_fft(p, x, y, c["n_fft"], c["hop"], 0.5, outputs=ALL, **_kw(c))
    assert all(bool(torch.isfinite(torch.view_as_real(t) if t.is_complex() else t).all()) for t in clean.values())
    bad = c["B"] - 1
    yn = y.clone()
    yn[bad, yn.shape[1] // 2] = float("nan")
    got = bhw.csd_fft(p, x, yn, c["n_fft"], c["hop"], 0.5, outputs=ALL, **_kw(c))
    for n in ("pxy", "pyy", "coherence", "h1"):
        assert _all_nan(got[n][bad]), (cid, n)
    assert _same_bits(got["pxx"], clean["pxx"]), cid                   # x has no NaN: its own spectrum is untouched
    keep = [b for b in range(c["B"]) if b != bad]
    assert not _same_all({n: t[keep] for n, t in got.items()}, {n: t[keep] for n, t in clean.items()}), cid


# ---- graph capture -----------------------------------------------------------------------------------------------------------------------

def test_csd_fft_is_captured_with_no_warm_call(torch):
    p = B.make_params(B.WIN_BH5, 13, 20)                               # a configuration no other test of this file has used
    n_fft, L, hop, nb, F = 512, 400, 160, 4, 299                      # two blocks: the kernel and both joins are in the graph
    T = (F - 1) * hop + n_fft
    x, y = _signal(torch, nb, T, 7), _signal(torch, nb, T, 9)
    K = n_fft // 2 + 1
    out = {"pxy": torch.full((nb, K), -1.0, dtype=torch.complex64, device="cuda"), "coherence": torch.full((nb, K), -1.0, device="cuda")}
    s = B.make_stft(nb, T, F, hop, n_fft)
    assert CC.parse(B.describe_csd_fft(p, L, s, outputs=tuple(out)))["joins"] == 2
    ws = torch.empty(B.csd_fft_workspace_bytes(s) // 8, dtype=torch.float64, device="cuda")
    kw = dict(win_length=L, outputs=tuple(out), out=out, workspace=ws)
    graph, res = _capture(torch, lambda: bhw.csd_fft(p, x, y, n_fft, hop, 1e-3, **kw))
    assert all(res[n].data_ptr() == out[n].data_ptr() for n in out)
    x.copy_(_signal(torch, nb, T, 8) * 3.0 - 2.0)
    y.copy_(0.5 * x + _signal(torch, nb, T, 10))
    graph.replay()
    torch.cuda.synchronize()
    want = bhw.csd_fft(p, x, y, n_fft, hop, 1e-3, win_length=L, outputs=tuple(out))
    assert not _same_all({n: t.clone() for n, t in out.items()}, want) and bool((out["coherence"] > 0).all())
    with bhw.ResidentTable(p) as tab:                                  # the from-table form on its first call
        out["coherence"].fill_(-1.0)
        graph, res = _capture(torch, lambda: tab.csd_fft(p, x, y, n_fft, hop, 1e-3, **kw))
        graph.replay()
        torch.cuda.synchronize()
        assert not _same_all({n: t.clone() for n, t in out.items()}, want)


def test_table_cross_spectra_fused_is_captured_after_one_warm_call_and_replayed_on_new_data(torch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    L, nfft, T, nb = 400, 512, 48000, 4                                # 299 segments
    x, y = _signal(torch, nb, T, 11), _signal(torch, nb, T, 13)
    kw = dict(length=L, noverlap=240, nfft=nfft)
    with bhw.ResidentTable(p) as tab:
        f0, r0 = tab.cross_spectra_fused(p, x, y, 16000.0, **kw)       # the warm call reads the window sums
        out = {n: torch.empty_like(t) for n, t in r0.items()}
        ws = torch.empty(B.csd_fft_workspace_bytes(B.make_stft(nb, T, 299, 160, nfft)) // 8, dtype=torch.float64, device="cuda")
        graph, (f, r) = _capture(torch, lambda: tab.cross_spectra_fused(p, x, y, 16000.0, out=out, workspace=ws, **kw))
        assert all(r[n].data_ptr() == out[n].data_ptr() for n in out) and f is f0
        x.copy_(_signal(torch, nb, T, 12) * 3.0 - 2.0)
        y.copy_(0.5 * x + _signal(torch, nb, T, 14))
        r["pxx"].fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        fe, re_ = tab.cross_spectra_fused(p, x, y, 16000.0, **kw)
        fl, rl = bhw.cross_spectra_fused(p, x, y, 16000.0, **kw)
        assert not _same_all(r, re_) and torch.equal(f, fe) and not _same_all(rl, re_) and bool((r["pxx"] > 0).all())
        # pxx / pyy are welch_fused of x / of y at any length
        assert _same_bits(re_["pxx"], tab.welch_fused(p, x, 16000.0, **kw)[1]) and _same_bits(re_["pyy"], tab.welch_fused(p, y, 16000.0, **kw)[1])
        # the one-output forms are the same words
        assert _same_bits(tab.csd_fused(p, x, y, 16000.0, **kw)[1], re_["pxy"])
        assert _same_bits(tab.coherence_fused(p, x, y, 16000.0, **kw)[1], re_["coherence"])
        assert _same_bits(tab.transfer_function_fused(p, x, y, 16000.0, **kw)[1], re_["h1"])
        assert _same_bits(bhw.csd_fused(p, x, y, 16000.0, **kw)[1], re_["pxy"])
        assert _same_bits(bhw.coherence_fused(p, x, y, 16000.0, **kw)[1], re_["coherence"])
        assert _same_bits(bhw.transfer_function_fused(p, x, y, 16000.0, **kw)[1], re_["h1"])


def test_cross_spectra_fused_under_capture_needs_the_sums_read_first(torch, monkeypatch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    x = torch.zeros((2, 4000), device="cuda")
    with bhw.ResidentTable(p) as tab:
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="window sums"):
            tab.cross_spectra_fused(p, x, x, length=397, nfft=512)
        monkeypatch.undo()
        f1, _ = tab.cross_spectra_fused(p, x, x, length=397, nfft=512)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        f2, _ = tab.cross_spectra_fused(p, x, x, length=397, nfft=512)  # cached: no read, no error
        with pytest.raises(RuntimeError, match="frequency axis"):
            tab.cross_spectra_fused(p, x, x, 8000.0, length=397, nfft=512)
        monkeypatch.undo()
        assert f2 is f1 and tab.welch_fused(p, x, length=397, nfft=512)[0] is f1     # welch_fused's shared, read-only axis
    torch.cuda.synchronize()


# ---- end to end against the model --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,noverlap,nfft", [(2048, 1024, 2048), (400, 240, 512)])
def test_end_to_end_within_twice_the_torch_route(torch, L, noverlap, nfft):
    """test_gpu_csd.py's signal pair (its noise level matters: DESIGN.md section 16) against that file's float64 restatements of
    scipy.signal.csd and scipy.signal.coherence; the yardstick is the error of the torch-only float32 route on the same GPU and the
    bound twice the yardstick, the project's standing bound.  The csd at the strong tone of 1e3, the coherence at 4, as there."""
    p = B.make_params(B.WIN_BH7, 16, 32)
    vh = _v(p, L)
    v = torch.from_numpy(vh).cuda()
    xh, yh = _pair(200000, 5, 1e3)
    x, y = torch.from_numpy(xh).cuda(), torch.from_numpy(yh).cuda()
    fr, ref, _ = _cross_ref64(xh, yh, vh, 1.0, L, noverlap, nfft)
    f, r = bhw.cross_spectra_fused(p, x, y, 1.0, length=L, noverlap=noverlap, nfft=nfft)
    with bhw.ResidentTable(p) as tab:
        ft, rt = tab.cross_spectra_fused(p, x, y, 1.0, length=L, noverlap=noverlap, nfft=nfft)
    assert not _same_all(r, rt) and torch.equal(f, ft)
    assert f.dtype == torch.float64 and np.allclose(f.cpu().numpy(), fr, rtol=0, atol=1e-15)
    Pyard, _ = _torch_route(torch, x, y, v, 1.0, L, noverlap, nfft)
    top = np.abs(ref).max()
    yard = float(np.abs(Pyard.cpu().numpy().astype(np.complex128) - ref).max() / top)
    err = float(np.abs(r["pxy"].cpu().numpy().astype(np.complex128) - ref).max() / top)
    print(f"csd_fused end to end L={L} nfft={nfft} hop={L - noverlap}: cross_spectra_fused {err:.3e}, torch-only route {yard:.3e}, "
          f"ratio {err / yard:.3f}")
    assert err <= 2.0 * yard, (err, yard)
    xh, yh = _pair(200000, 5, 4.0)
    x, y = torch.from_numpy(xh).cuda(), torch.from_numpy(yh).cuda()
    _, _, cref = _cross_ref64(xh, yh, vh, 1.0, L, noverlap, nfft)
    _, C = bhw.coherence_fused(p, x, y, 1.0, length=L, noverlap=noverlap, nfft=nfft)
    _, Cyard = _torch_route(torch, x, y, v, 1.0, L, noverlap, nfft)
    yard = float(np.abs(Cyard.cpu().numpy().astype(np.float64) - cref).max())
    err = float(np.abs(C.cpu().numpy().astype(np.float64) - cref).max())
    print(f"coherence_fused end to end L={L} nfft={nfft} hop={L - noverlap}: coherence_fused {err:.3e}, torch-only route {yard:.3e}, "
          f"ratio {err / yard:.3f}")
    assert err <= 2.0 * yard, (err, yard)


# ---- Python errors -----------------------------------------------------------------------------------------------------------------------

def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    x = torch.zeros((2, 1000), device="cuda")
    xc = torch.zeros((2, 1000), dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError, match="real float32.*stft_iq"):
        bhw.csd_fft(p, xc, xc, 64, 16, 1.0)
    with pytest.raises(ValueError, match="real float32"):
        bhw.cross_spectra_fused(p, x, xc, length=64)
    with pytest.raises(ValueError, match="mixed-radix.*stft_mixed"):
        bhw.csd_fft(p, x, x, 48, 16, 1.0, win_length=8)
    with pytest.raises(ValueError, match="mixed-radix.*stft_mixed"):
        bhw.cross_spectra_fused(p, x, x, length=60)
    with pytest.raises(ValueError, match="4096.*16..2048.*welch_csd"):
        bhw.csd_fft(p, torch.zeros((2, 9000), device="cuda"), torch.zeros((2, 9000), device="cuda"), 4096, 16, 1.0, win_length=8)
    with pytest.raises(ValueError, match="4096.*fft='fused'"):
        bhw.cross_spectra_fused(p, torch.zeros(9000, device="cuda"), torch.zeros(9000, device="cuda"), length=1000, nfft=4096)
    for n in (8, 8192, 17):
        with pytest.raises(ValueError, match="power of two in 16..2048"):
            bhw.csd_fft(p, x, x, n, 16, 1.0, win_length=8)
    with pytest.raises(ValueError, match="same length.*pad or cut"):
        bhw.csd_fft(p, x, x[:, :900], 64, 16, 1.0)
    with pytest.raises(ValueError, match="same length"):
        bhw.cross_spectra_fused(p, x[:, :900], x, length=64)
    with pytest.raises(ValueError, match="x must be \\(T,\\)"):
        bhw.csd_fft(p, x, x[0], 64, 16, 1.0)
    with pytest.raises(ValueError, match="x must be \\(T,\\)"):
        bhw.csd_fft(p, torch.zeros((3, 1000), device="cuda"), x, 64, 16, 1.0)
    with pytest.raises(TypeError):
        bhw.cross_spectra_fused(p, x, x, length=64, average="median")
    with pytest.raises(TypeError):
        bhw.cross_spectra_fused(p, x, x, length=64, return_onesided=False)
    with pytest.raises(TypeError):
        bhw.cross_spectra_fused(p, x, x, length=64, fft="fused")
    with pytest.raises(ValueError, match="'torch' or 'fused'"):
        bhw.cross_spectra(p, x, x, length=64, fft="accumulate")
    with pytest.raises(ValueError, match="detrend"):
        bhw.cross_spectra_fused(p, x, x, length=64, detrend="linear")
    with pytest.raises(ValueError, match="scaling"):
        bhw.cross_spectra_fused(p, x, x, length=64, scaling="power")
    with pytest.raises(ValueError, match="noverlap"):
        bhw.cross_spectra_fused(p, x, x, length=64, noverlap=64)
    with pytest.raises(ValueError, match="nfft"):
        bhw.cross_spectra_fused(p, x, x, length=64, nfft=32)
    with pytest.raises(ValueError, match="zero segments"):
        bhw.cross_spectra_fused(p, x[:, :50], x[:, :50], length=64)
    with pytest.raises(ValueError, match="zero frames"):
        bhw.csd_fft(p, x[:, :50], x[:, :50], 64, 16, 1.0)
    with pytest.raises(ValueError, match="hop"):
        bhw.csd_fft(p, x, x, 64, 0, 1.0)
    with pytest.raises(ValueError, match="center=False"):
        bhw.csd_fft(p, x, x, 64, 16, 1.0, center=True, detrend=True)
    with pytest.raises(ValueError, match="CUDA"):
        bhw.csd_fft(p, x.cpu(), x.cpu(), 64, 16, 1.0)
    with pytest.raises(ValueError, match="CUDA"):
        bhw.csd_fft(p, x.cpu(), x, 64, 16, 1.0)
    with pytest.raises(ValueError):
        bhw.csd_fft(p, x, x, 64, 16, 1.0, outputs=("pxz",))
    with pytest.raises(ValueError):
        bhw.csd_fft(p, x, x, 64, 16, 1.0, outputs=())
    with pytest.raises(ValueError, match="out must be a dict"):
        bhw.csd_fft(p, x, x, 64, 16, 1.0, out={"pxx": torch.zeros((2, 33), device="cuda")})
    with pytest.raises(ValueError, match=r"out\['pxy'\] must be"):
        bhw.csd_fft(p, x, x, 64, 16, 1.0, out={"pxy": torch.zeros((2, 33), device="cuda")})
    with pytest.raises(ValueError, match="same row stride"):
        bhw.csd_fft(p, x, x, 64, 16, 1.0, outputs=("pxx", "pyy"), out={"pxx": torch.zeros((2, 40), device="cuda")[:, :33],
                                                                       "pyy": torch.zeros((2, 33), device="cuda")})
    with pytest.raises(ValueError, match="workspace"):
        bhw.csd_fft(p, x, x, 64, 16, 1.0, workspace=torch.zeros(8, dtype=torch.float64, device="cuda"))
    with pytest.raises(B.BhwError, match="not finite"):
        bhw.csd_fft(p, x, x, 64, 16, float("inf"))
    # a centred, reflect-padded call is fine; 1-D x and y give 1-D outputs; the same tensor may be both operands
    r = bhw.csd_fft(p, x[0], x[0], 64, 16, 1.0, center=True)
    assert set(r) == {"pxy"} and r["pxy"].shape == (33,) and r["pxy"].dtype == torch.complex64
    # x and y with different batch strides are made to agree (one descriptor serves both)
    wide = torch.zeros((2, 1500), device="cuda")
    assert bhw.csd_fft(p, wide[:, :1000], x, 64, 16, 1.0)["pxy"].shape == (2, 33)
