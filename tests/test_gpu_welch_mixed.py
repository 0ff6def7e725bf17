"""The fused Welch PSD at a mixed-radix n_fft on the GPU (bhw_welch_mfft_f32_* through bhw.welch_fft_mixed, bhw.welch_fused_mixed and
their ResidentTable forms).

The gate is exact.  include/bhw.h defines P on the float32 pairs bhw_stft_mfft_f32_* writes: q = re^2 + im^2 in binary64, summed over
the frames in chunks of 16, the chunks of a block of 256 frames in order, then the blocks in order, times s_k, rounded once.  For every
case of tests/welch_mfft_cases.py, library and table, doubled and not, P must equal that restated in torch float64 on bhw.stft_mixed
of the same call, word for word: every step of the restatement is an IEEE elementwise operation, so there is no tolerance.  Around it:
the agreement with welch_psd(stft_mixed(...)) (bit for bit up to 16 frames, one float32 ulp always), independence of the batch and
the form, untouched gaps, zeros, NaN containment, graph capture, the Python errors, and the end-to-end accuracy bound of
test_gpu_welch_fft.py against a float64 restatement of scipy.signal.welch at nfft 400 and 1000.

Measured on an MI355X: every case 0 differing words, library and table, and 0 ulp from
welch_psd(stft_mixed(...)); end to end 2.290e-8 against the torch-only route's 1.900e-7 at 400 / 240 / 400 (ratio 0.121) and 6.798e-8
against 1.542e-7 at 1000 / 500 / 1000 (ratio 0.441), the bound being 2."""
import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import welch_mfft_cases as WC

pytestmark = pytest.mark.gpu

CHUNK, BLOCK = B.WELCH_FFT_CHUNK, B.WELCH_BLOCK
SENTINEL = 12345.5


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _v(p, L):
    w = bhw.window(p, L).cpu().numpy()
    return np.ldexp(w.astype(np.float32), -(p.dat_width - 1)).astype(np.float32)


def _signal(torch, nb, T, seed):
    """(B, T) float32 on the device: noise of 1000, two tones 120 dB apart and an offset."""
    g = torch.Generator(device="cuda").manual_seed(2000 + seed)
    n = torch.arange(T, device="cuda", dtype=torch.float64)
    tones = 1e3 * torch.cos(2 * np.pi * 0.1234 * n) + 1e-3 * torch.cos(2 * np.pi * 0.31 * n + 1.0) + 250.0
    return (torch.randn((nb, T), device="cuda", generator=g, dtype=torch.float64) * 1000 + tones).float()


def _pad_axis(torch, t, axis, to):
    """t with +0.0 appended along `axis` up to a multiple of `to`.  Every term is a q >= +0.0 or a NaN and every sum starts from +0.0,
    so adding +0.0 changes no bit: a shorter last chunk (block) is the same sum."""
    n = t.shape[axis]
    extra = -n % to
    if not extra:
        return t
    shape = list(t.shape)
    shape[axis] = extra
    return torch.cat([t, torch.zeros(shape, dtype=t.dtype, device=t.device)], dim=axis)


def _restate(torch, Y, scale, n_fft, onesided):
    """include/bhw.h on the spectrum rows Y (B, F, K) complex64, in torch float64 on the device: three levels of explicit elementwise
    adds -- 16 frames of every chunk in ascending order, 16 chunks of every block in ascending order, the blocks in ascending order,
    each from +0.0 -- then (A * s_k).float().  The chunks (blocks) are independent chains, so one add serves all of them."""
    Y = Y if Y.dim() == 3 else Y.unsqueeze(0)
    re, im = Y.real.double(), Y.imag.double()
    q = re ** 2 + im ** 2                                              # both squares exact in binary64: one rounding
    nb, F, K = q.shape
    qc = _pad_axis(torch, q, 1, CHUNK).view(nb, -1, CHUNK, K)
    A_chunk = torch.zeros((nb, qc.shape[1], K), dtype=torch.float64, device=q.device)
    for i in range(CHUNK):
        A_chunk = A_chunk + qc[:, :, i, :]
    cb = _pad_axis(torch, A_chunk, 1, BLOCK // CHUNK).view(nb, -1, BLOCK // CHUNK, K)
    A_blk = torch.zeros((nb, cb.shape[1], K), dtype=torch.float64, device=q.device)
    for j in range(BLOCK // CHUNK):
        A_blk = A_blk + cb[:, :, j, :]
    A = torch.zeros((nb, K), dtype=torch.float64, device=q.device)
    for blk in range(A_blk.shape[1]):
        A = A + A_blk[:, blk, :]
    sk = torch.full((K,), float(scale), dtype=torch.float64, device=q.device)
    if onesided:
        sk[1:] = float(scale) * 2.0
        if n_fft % 2 == 0:
            sk[-1] = float(scale)
    return (A * sk).float()


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _ulps(a, b):
    """The largest distance in float32 ulps between two tensors of finite values >= +0.0 (their int32 views are monotonic)."""
    return int((_bits(a).long() - _bits(b).long()).abs().max())


def _kw(c):
    if c["detrend"]:
        return dict(win_length=c["L"], center=False, detrend=True)
    return dict(win_length=c["L"], center=bool(c["mode"]), pad_mode=c["mode"] or "reflect", detrend=False)


def _case_x(torch, c, seed=0):
    x = _signal(torch, c["B"], WC.frames_to_samples(c), seed)
    return x[0] if c["B"] == 1 and seed % 2 else x                   # a 1-D x now and then


# ---- the gate ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", WC.case_ids())
def test_word_for_word_equal_to_the_contract_on_stft_mixed_rows(torch, cid):
    c = WC.case(cid)
    p = WC.params(c["setup"])
    _, _, F, _ = WC.desc(c)
    x = _case_x(torch, c, seed=WC.case_ids().index(cid))
    n_fft, K = c["n_fft"], c["n_fft"] // 2 + 1
    Y = bhw.stft_mixed(p, x, n_fft, c["hop"], **_kw(c))
    assert Y.shape[-2:] == (F, K)
    with bhw.ResidentTable(p) as tab:
        d = WC.parse(WC.line(c, table=tab._live()))
        assert d["table"] and d["frames"] == F
        for onesided, scale in ((True, 1.0 / (3.7 * F)), (False, 0.37)):
            want = _restate(torch, Y, scale, n_fft, onesided)
            want = want[0] if x.dim() == 1 else want
            if c.get("padded"):
                buf = torch.full((c["B"], K + 5), SENTINEL, device="cuda")
                out = buf[:, :K] if x.dim() == 2 else buf[0, :K]
                got = bhw.welch_fft_mixed(p, x, n_fft, c["hop"], scale, onesided_doubling=onesided, out=out, **_kw(c))
                assert got.data_ptr() == buf.data_ptr() and bool((buf[:, K:] == SENTINEL).all()), "a gap was written"
            else:
                got = bhw.welch_fft_mixed(p, x, n_fft, c["hop"], scale, onesided_doubling=onesided, **_kw(c))
            assert got.dtype == torch.float32 and got.shape == want.shape
            differ = int((_bits(got) != _bits(want)).sum())
            print(f"{cid} onesided={onesided}: library {differ} differing words of {want.numel()}")
            assert _same_bits(got, want), (cid, "library", onesided, _ulps(got, want))
            tb = tab.welch_fft_mixed(p, x, n_fft, c["hop"], scale, onesided_doubling=onesided, **_kw(c))
            assert _same_bits(tb, want), (cid, "table", onesided, _ulps(tb, want))
            # the two-call route: welch_psd sums plain blocks of 256 frames
            two = bhw.welch_psd(Y, scale, nfft=n_fft, onesided=onesided)
            assert two.shape == got.shape and bool(torch.isfinite(two).all())
            ulps = _ulps(got, two)
            print(f"{cid} onesided={onesided}: F = {F}, against welch_psd(stft_mixed(...)): {ulps} ulp")
            assert ulps <= 1, (cid, ulps)
            if F <= CHUNK:                                             # the plain ascending sum: bit for bit
                assert ulps == 0 and _same_bits(got, two), cid


# ---- determinism, gaps, zeros, specials --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_fft,L,hop,F", [(96, 80, 24, 40), (400, 400, 160, 40), (4000, 4000, 1000, 20)])
def test_a_signal_alone_and_as_number_37_of_64_give_the_same_bits(torch, n_fft, L, hop, F):
    p = WC.params(0)
    x = _signal(torch, 64, (F - 1) * hop + n_fft, n_fft)
    kw = dict(win_length=L, detrend=False)
    P64 = bhw.welch_fft_mixed(p, x, n_fft, hop, 0.01, **kw)
    one = bhw.welch_fft_mixed(p, x[37], n_fft, hop, 0.01, **kw)
    assert one.shape == (n_fft // 2 + 1,) and _same_bits(one, P64[37])
    assert _same_bits(bhw.welch_fft_mixed(p, x[37:38], n_fft, hop, 0.01, **kw)[0], P64[37])
    with bhw.ResidentTable(p) as tab:
        assert _same_bits(tab.welch_fft_mixed(p, x, n_fft, hop, 0.01, **kw), P64)
        assert _same_bits(tab.welch_fft_mixed(p, x[37], n_fft, hop, 0.01, **kw), P64[37])


def test_sentinels_in_the_gaps_of_a_padded_out_and_behind_the_workspace_are_untouched(torch):
    c = WC.case("n50-3x17")
    p = WC.params(c["setup"])
    x = _case_x(torch, c)
    K = 26
    buf = torch.full((3, K + 7), SENTINEL, device="cuda")
    ws = torch.full((B.welch_mfft_workspace_bytes(WC.desc(c)[0]) // 8 + 3,), SENTINEL, dtype=torch.float64, device="cuda")
    got = bhw.welch_fft_mixed(p, x, 50, c["hop"], 0.5, out=buf[:, :K], workspace=ws, **_kw(c))
    assert got.data_ptr() == buf.data_ptr() and _same_bits(got, bhw.welch_fft_mixed(p, x, 50, c["hop"], 0.5, **_kw(c)))
    assert bool((buf[:, K:] == SENTINEL).all()) and bool((ws[-3:] == SENTINEL).all()), "a gap or the workspace's end was written"
    assert bool((ws[:-3] != SENTINEL).all()), "a chunk sum of the workspace was never written"
    with pytest.raises(ValueError, match="workspace"):
        bhw.welch_fft_mixed(p, x, 50, c["hop"], 0.5, workspace=ws[:ws.numel() - 4], **_kw(c))


@pytest.mark.parametrize("cid", ["n18-l13-detrend-2x70", "n200-l160-detrend-2x40", "n400-3x259", "n4050-detrend-1x35"])
def test_zeros_in_give_positive_zero_out(torch, cid):
    c = WC.case(cid)
    p = WC.params(c["setup"])
    x = torch.zeros((c["B"], WC.frames_to_samples(c)), device="cuda")
    P = bhw.welch_fft_mixed(p, x, c["n_fft"], c["hop"], 0.25, **_kw(c))
    assert bool((_bits(P) == 0).all()), cid                           # +0.0: not -0.0, not a denormal


@pytest.mark.parametrize("cid", ["n50-3x17", "n400-3x259", "n1536-2x18-form1"])
def test_one_nan_poisons_exactly_the_row_of_its_own_signal(torch, cid):
    c = WC.case(cid)
    p = WC.params(c["setup"])
    x = _case_x(torch, c)
    clean = bhw.welch_fft_mixed(p, x, c["n_fft"], c["hop"], 0.5, **_kw(c))
    assert bool(torch.isfinite(clean).all())
    bad = c["B"] - 1
    x[bad, x.shape[1] // 2] = float("nan")
    P = bhw.welch_fft_mixed(p, x, c["n_fft"], c["hop"], 0.5, **_kw(c))
    assert bool(torch.isnan(P[bad]).all()), cid
    keep = [b for b in range(c["B"]) if b != bad]
    assert _same_bits(P[keep], clean[keep]), cid


# ---- graph capture -----------------------------------------------------------------------------------------------------------------------

def _capture(torch, fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            res = fn()
    torch.cuda.current_stream().wait_stream(s)
    return graph, res


def test_welch_fft_mixed_is_captured_with_no_warm_call(torch):
    p = B.make_params(B.WIN_BH5, 13, 24)                               # a configuration no other test of this file has used
    n_fft, L, hop, nb, F = 400, 320, 160, 4, 299                      # two blocks: the kernel and both joins are in the graph
    T = (F - 1) * hop + n_fft
    x = _signal(torch, nb, T, 7)
    out = torch.full((nb, n_fft // 2 + 1), -1.0, device="cuda")
    s = B.make_stft(nb, T, F, hop, n_fft)
    ws = torch.empty(B.welch_mfft_workspace_bytes(s) // 8, dtype=torch.float64, device="cuda")
    kw = dict(win_length=L, out=out, workspace=ws)
    graph, P = _capture(torch, lambda: bhw.welch_fft_mixed(p, x, n_fft, hop, 1e-3, **kw))
    assert P.data_ptr() == out.data_ptr()
    x.copy_(_signal(torch, nb, T, 8) * 3.0 - 2.0)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(out.clone(), bhw.welch_fft_mixed(p, x, n_fft, hop, 1e-3, win_length=L)) and bool((out > 0).all())
    with bhw.ResidentTable(p) as tab:                                  # the from-table form on its first call
        out.fill_(-1.0)
        graph, P = _capture(torch, lambda: tab.welch_fft_mixed(p, x, n_fft, hop, 1e-3, **kw))
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(out.clone(), bhw.welch_fft_mixed(p, x, n_fft, hop, 1e-3, win_length=L))


def test_table_welch_fused_mixed_is_captured_after_one_warm_call_and_replayed_on_new_data(torch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    L, nfft, T, nb = 400, 400, 48000, 4                                # 298 segments
    F = 1 + (T - L) // 160
    x = _signal(torch, nb, T, 11)
    kw = dict(length=L, noverlap=240, nfft=nfft)
    with bhw.ResidentTable(p) as tab:
        f0, P0 = tab.welch_fused_mixed(p, x, 16000.0, **kw)            # the warm call reads the window sums
        out = torch.empty_like(P0)
        ws = torch.empty(B.welch_mfft_workspace_bytes(B.make_stft(nb, T, F, 160, nfft)) // 8, dtype=torch.float64, device="cuda")
        graph, (f, P) = _capture(torch, lambda: tab.welch_fused_mixed(p, x, 16000.0, out=out, workspace=ws, **kw))
        assert P.data_ptr() == out.data_ptr()
        x.copy_(_signal(torch, nb, T, 12) * 3.0 - 2.0)
        P.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        fe, Pe = tab.welch_fused_mixed(p, x, 16000.0, **kw)
        fl, Pl = bhw.welch_fused_mixed(p, x, 16000.0, **kw)
        assert _same_bits(P, Pe) and torch.equal(f, fe) and _same_bits(Pl, Pe) and bool((P > 0).all())
        assert torch.equal(f, torch.fft.rfftfreq(nfft, d=1.0 / 16000.0, dtype=torch.float64, device="cuda"))
        # the two-call route on the same segments with the same scale
        scale = B.welch_scale(tab.window_sums(p, L, f32=True), F, 16000.0, "density")
        Y = bhw.stft_mixed(p, x, nfft, 160, win_length=L, center=False, detrend=True)
        assert _ulps(Pe, bhw.welch_psd(Y, scale, nfft=nfft)) <= 1


def test_welch_fused_mixed_under_capture_needs_the_sums_and_the_axis_first(torch, monkeypatch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    x = torch.zeros((2, 4000), device="cuda")
    with bhw.ResidentTable(p) as tab:
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="window sums"):
            tab.welch_fused_mixed(p, x, length=397, nfft=400)
        monkeypatch.undo()
        tab.welch_fused_mixed(p, x, length=397, nfft=400)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        f1, _ = tab.welch_fused_mixed(p, x, length=397, nfft=400)      # cached: no read, no error
        with pytest.raises(RuntimeError, match="frequency axis"):
            tab.welch_fused_mixed(p, x, 8000.0, length=397, nfft=400)
        monkeypatch.undo()
        f2, _ = tab.welch_fused_mixed(p, x, 8000.0, length=397, nfft=400)
        assert f2 is not f1 and torch.equal(f2, torch.fft.rfftfreq(400, d=1.0 / 8000.0, dtype=torch.float64, device="cuda"))
        # keys of their own kind: they neither meet welch_fused's "freqs" keys nor count against its eight axes
        tab.welch_fused(p, x, 8000.0, length=397, nfft=512)
        for i in range(12):
            tab.welch_fused_mixed(p, x, 100.0 + i, length=397, nfft=400)
        assert sum(1 for k in tab._sums if k[0] == "freqs_mixed") <= 8
        assert sum(1 for k in tab._sums if k[0] == "freqs") == 1
        for i in range(8):
            tab.welch_fused(p, x, 200.0 + i, length=397, nfft=512)
        assert sum(1 for k in tab._sums if k[0] == "freqs_mixed") == 8 and sum(1 for k in tab._sums if k[0] == "freqs") == 8
    torch.cuda.synchronize()


# ---- end to end against the model --------------------------------------------------------------------------------------------------------

def _welch_ref64(x, v, fs, L, noverlap, nfft, detrend, scaling="density"):
    """scipy.signal.welch(x, fs, window=v, noverlap=noverlap, nfft=nfft, detrend=detrend, scaling=scaling) restated in NumPy float64
    (tests/test_gpu_welch.py's restatement, which that file holds against scipy itself)."""
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    hop = L - noverlap
    F = (x.shape[-1] - noverlap) // hop
    seg = x[..., np.arange(F)[:, None] * hop + np.arange(L)[None, :]]
    if detrend:
        seg = seg - seg.mean(axis=-1, keepdims=True)
    Y = np.fft.rfft(seg * v, n=nfft, axis=-1)
    scale = 1.0 / (fs * (v * v).sum()) if scaling == "density" else 1.0 / v.sum() ** 2
    P = (Y.real ** 2 + Y.imag ** 2) * scale
    P[..., 1:] *= 2.0
    if nfft % 2 == 0:
        P[..., -1] /= 2.0
    return np.fft.rfftfreq(nfft, 1.0 / fs), P.mean(axis=-2)


def _torch_route(torch, x, v, fs, L, noverlap, nfft):
    """The torch-only float32 route: unfold, subtract mean, multiply, rfft, abs() ** 2, mean."""
    seg = x.unfold(-1, L, L - noverlap)
    seg = (seg - seg.mean(-1, keepdim=True)) * v
    P = (torch.fft.rfft(seg, n=nfft).abs() ** 2).mean(-2) * (1.0 / (fs * (v * v).sum()))
    P[..., 1:] *= 2.0
    if nfft % 2 == 0:
        P[..., -1] /= 2.0
    return P


def _test_signal(T, seed):
    """White noise, two tones 120 dB apart and a DC offset: test_gpu_welch_fft.py's signal."""
    rng = np.random.default_rng(seed)
    n = np.arange(T, dtype=np.float64)
    x = np.cos(2 * np.pi * 0.1234 * n) + 1e-6 * np.cos(2 * np.pi * 0.31 * n + 1.0) + 1e-4 * rng.standard_normal(T) + 0.5
    return x.astype(np.float32)


def _rel_err(P, ref):
    return float(np.abs(np.asarray(P, dtype=np.float64) - ref).max() / ref.max())


def test_the_restatement_is_scipys(torch):
    signal = pytest.importorskip("scipy.signal")
    p = B.make_params(B.WIN_BH7, 16, 32)
    x = _test_signal(30000, 3).astype(np.float64)
    for L, nov, nfft in ((400, 240, 400), (1000, 500, 1000)):
        v = _v(p, L).astype(np.float64)
        f0, P0 = signal.welch(x, 2.0, window=v, noverlap=nov, nfft=nfft, detrend="constant", scaling="density")
        f1, P1 = _welch_ref64(x, v, 2.0, L, nov, nfft, True)
        assert np.allclose(f0, f1, rtol=0, atol=1e-15) and np.abs(P0 - P1).max() <= 1e-12 * P0.max(), L


@pytest.mark.parametrize("L,noverlap,nfft", [(400, 240, 400), (1000, 500, 1000)])
def test_end_to_end_within_twice_the_torch_route(torch, L, noverlap, nfft):
    """test_gpu_welch_fft.py's end-to-end signal (white noise, two tones 120 dB apart, a DC offset, T = 200 000) against the float64
    restatement of scipy.signal.welch; the yardstick is the error of the torch-only float32 route on the same GPU,
    max |dPxx| / max Pxx, and the bound twice the yardstick: the project's standing bound."""
    p = B.make_params(B.WIN_BH7, 16, 32)
    xh = _test_signal(200000, 5)
    x = torch.from_numpy(xh).cuda()
    vh = _v(p, L)
    fr, ref = _welch_ref64(xh, vh, 1.0, L, noverlap, nfft, True)
    f, P = bhw.welch_fused_mixed(p, x, 1.0, length=L, noverlap=noverlap, nfft=nfft)
    with bhw.ResidentTable(p) as tab:
        ft, Pt = tab.welch_fused_mixed(p, x, 1.0, length=L, noverlap=noverlap, nfft=nfft)
    assert _same_bits(P, Pt) and torch.equal(f, ft)
    assert f.dtype == torch.float64 and np.allclose(f.cpu().numpy(), fr, rtol=0, atol=1e-15)
    yard = _rel_err(_torch_route(torch, x, torch.from_numpy(vh).cuda(), 1.0, L, noverlap, nfft).cpu().numpy(), ref)
    err = _rel_err(P.cpu().numpy(), ref)
    print(f"welch_fused_mixed end to end L={L} nfft={nfft} hop={L - noverlap}: welch_fused_mixed {err:.3e}, "
          f"torch-only route {yard:.3e}, ratio {err / yard:.3f}")
    assert err <= 2.0 * yard, (err, yard)
    _, refs = _welch_ref64(xh, vh, 1.0, L, noverlap, nfft, True, "spectrum")
    _, Ps = bhw.welch_fused_mixed(p, torch.stack([x, x]), 1.0, length=L, noverlap=noverlap, nfft=nfft, scaling="spectrum")
    assert Ps.shape == (2, nfft // 2 + 1) and _same_bits(Ps[0], Ps[1]) and _rel_err(Ps[0].cpu().numpy(), refs) <= 2.0 * yard


# ---- Python errors -----------------------------------------------------------------------------------------------------------------------

def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    x = torch.zeros((2, 1000), device="cuda")
    xc = torch.zeros((2, 1000), dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError, match="welch_fft_iq"):
        bhw.welch_fft_mixed(p, xc, 48, 16, 1.0)
    with pytest.raises(ValueError, match="welch_fft_iq"):
        bhw.welch_fused_mixed(p, xc, length=48)
    for n in (16, 64, 4096):
        with pytest.raises(ValueError, match=r"power of two: welch_fft "):
            bhw.welch_fft_mixed(p, x, n, 16, 1.0, win_length=8)
    with pytest.raises(ValueError, match=r"power of two: welch_fft "):
        bhw.welch_fused_mixed(p, x, length=64)
    with pytest.raises(ValueError, match=r"power of two: welch_fft "):
        bhw.welch_fused_mixed(p, x, length=60, nfft=128)
    with bhw.ResidentTable(p) as tab:
        with pytest.raises(ValueError, match=r"power of two: welch_fft "):
            tab.welch_fft_mixed(p, x, 64, 16, 1.0)
        with pytest.raises(ValueError, match="welch_fft_iq"):
            tab.welch_fused_mixed(p, xc, length=48)
    for n in (14, 22, 70, 4098):
        with pytest.raises(ValueError, match="2\\^a"):
            bhw.welch_fft_mixed(p, x, n, 16, 1.0, win_length=8)
    # the other fronts refuse or route exactly as before
    for call in (lambda: bhw.welch_fft(p, x, 48, 16, 1.0, win_length=8), lambda: bhw.welch_fused(p, x, length=60),
                 lambda: bhw.welch_fused(p, x, length=60, nfft=100)):
        with pytest.raises(ValueError, match="power of two in 16..4096"):
            call()
    with pytest.raises(ValueError, match="real float32"):
        bhw.welch_fft(p, xc, 64, 16, 1.0)
    with pytest.raises(ValueError):
        bhw.welch_fft_iq(p, xc, 48, 16, 1.0)
    with pytest.raises(ValueError, match="'torch' or 'fused'"):
        bhw.welch(p, x, length=48, fft="mixed")
    with pytest.raises(ValueError, match="power of two in 16..4096"):
        bhw.welch(p, x, length=48, fft="fused")                        # no route to the mixed-radix kernel through fft=
    with pytest.raises(TypeError):
        bhw.welch_fused_mixed(p, x, length=48, return_onesided=False)
    with pytest.raises(TypeError):
        bhw.welch_fused_mixed(p, x, length=48, average="median")
    with pytest.raises(TypeError):
        bhw.welch_fft_mixed(p, x, 48, 16, 1.0, fbank=None)
    with pytest.raises(ValueError, match="detrend"):
        bhw.welch_fused_mixed(p, x, length=48, detrend="linear")
    with pytest.raises(ValueError, match="scaling"):
        bhw.welch_fused_mixed(p, x, length=48, scaling="power")
    with pytest.raises(ValueError, match="noverlap"):
        bhw.welch_fused_mixed(p, x, length=48, noverlap=48)
    with pytest.raises(ValueError, match="nfft"):
        bhw.welch_fused_mixed(p, x, length=48, nfft=40)
    with pytest.raises(ValueError, match="zero segments"):
        bhw.welch_fused_mixed(p, x[:, :40], length=48)
    with pytest.raises(ValueError, match="zero frames"):
        bhw.welch_fft_mixed(p, x[:, :40], 48, 16, 1.0)
    with pytest.raises(ValueError, match="hop"):
        bhw.welch_fft_mixed(p, x, 48, 0, 1.0)
    with pytest.raises(ValueError, match="center=False"):
        bhw.welch_fft_mixed(p, x, 48, 16, 1.0, center=True, detrend=True)
    with pytest.raises(ValueError, match="pad_mode"):
        bhw.welch_fft_mixed(p, x, 48, 16, 1.0, center=True, pad_mode="edge")
    with pytest.raises(ValueError, match="CUDA"):
        bhw.welch_fft_mixed(p, x.cpu(), 48, 16, 1.0)
    with pytest.raises(ValueError, match="CUDA"):
        bhw.welch_fused_mixed(p, x.cpu(), length=48)
    with pytest.raises(ValueError, match="out must be"):
        bhw.welch_fft_mixed(p, x, 48, 16, 1.0, out=torch.zeros((2, 24), device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        bhw.welch_fft_mixed(p, x, 48, 16, 1.0, out=torch.zeros((2, 25), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="workspace"):
        bhw.welch_fft_mixed(p, x, 48, 16, 1.0, workspace=torch.zeros(8, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="workspace"):
        bhw.welch_fft_mixed(p, x, 48, 16, 1.0, workspace=torch.zeros(100000, dtype=torch.float32, device="cuda"))
    with pytest.raises(B.BhwError, match="not finite"):
        bhw.welch_fft_mixed(p, x, 48, 16, float("inf"))
    # a centred, reflect-padded call is fine, and a 1-D x gives a 1-D P
    assert bhw.welch_fft_mixed(p, x[0], 48, 16, 1.0, center=True).shape == (25,)
