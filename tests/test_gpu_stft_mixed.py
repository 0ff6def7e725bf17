"""The mixed-radix fused window + FFT kernel on the GPU (bhw_stft_mfft_f32_* through bhw.stft_mixed, bhw.spectrogram_mixed and their
ResidentTable forms): n_fft even 2^a 3^b 5^c that is no power of two -- 400, 480, 1000, 1200, ...

Accuracy is the gate, word for word that of test_gpu_stft_fft.py: for every case of tests/stft_mfft_cases.py the reference is
numpy.fft.rfft in float64 of the float32 rows (restated by the NumPy references of test_gpu_stft.py and test_gpu_welch.py, which the
parent's stft_frames / welch_frames rows must equal bit for bit first), the metric the largest relative l2 error of a spectrum row, the
yardstick torch.fft.rfft on the same GPU over the parent's rows, and the bound twice the yardstick's error under a cap of
2^-24 * log2(n_fft).  The FFT is not pinned bit for bit; everything around it is: the power and bank rows are the values computed on
the host from stft_mixed of the same call, and the row, slot, stride, route, IEEE and capture properties are held word for word."""
import math

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from test_gpu_stft import _frames_ref, _same
from test_gpu_welch import _segments_ref, _welch_ref64, _test_signal, _rel_err
from test_gpu_welch import _torch_route as _welch_torch_route
from test_gpu_stft_fft import _v, _case_signal, _row_errors, _bits
from test_gpu_spectrogram import _power_ref, _bank_ref

import stft_mfft_cases as MC

pytestmark = pytest.mark.gpu

SENTINEL = 12345.5


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_BANKS = {}


def _mel(torch, n_fft):
    """(dense weights, device FilterBank) of bhw.mel_weights(n_fft, 80, 16000), built once (the upload synchronises)."""
    if n_fft not in _BANKS:
        w = bhw.mel_weights(n_fft, MC.BANK_FILTERS, 16000)
        _BANKS[n_fft] = (w, bhw.FilterBank(w, device="cuda"))
    return _BANKS[n_fft]


def _kw(c):
    """The keywords of bhw.stft_mixed / stft_frames for a case."""
    if c["detrend"]:
        return dict(win_length=c["L"], center=False)
    return dict(win_length=c["L"], center=bool(c["mode"]), pad_mode=c["mode"] or "reflect")


def _rows_ref(c, xh, v):
    """The float32 rows (B, F, n_fft) the transform must see, by the restatements of the frames and segments tests."""
    _, L, frames, col0, pad, det = MC.desc(c)
    if det:
        y = _segments_ref(xh[:, :, None], v, c["n_fft"], c["hop"], True)
    else:
        y = _frames_ref(xh[:, :, None], v, c["n_fft"], c["hop"], col0, pad, c["mode"] or "constant")
    assert y.shape[1] == frames
    return y[..., 0]


def _parent_rows(torch, p, c, x):
    """The rows the parent's calls write for the case (packed); those calls take any n_fft."""
    if c["detrend"]:
        return bhw.welch_frames(p, x, c["L"], c["hop"], nfft=c["n_fft"], detrend="constant")
    return bhw.stft_frames(p, x, c["n_fft"], c["hop"], **_kw(c))


def _call(torch, p, c, x, table=None, out=None):
    fn = bhw.stft_mixed if table is None else table.stft_mixed
    return fn(p, x, c["n_fft"], c["hop"], detrend=bool(c["detrend"]), out=out, **_kw(c))


def _spec(torch, p, c, x, fb, table=None, out=None):
    fn = bhw.spectrogram_mixed if table is None else table.spectrogram_mixed
    return fn(p, x, c["n_fft"], c["hop"], detrend=bool(c["detrend"]), fbank=fb, out=out, **_kw(c))


def _padded_io(torch, c, xh):
    """x as rows of a wider buffer and a spectrum buffer with gaps behind every row and signal, both filled with a sentinel."""
    _, _, frames, _, _, _ = MC.desc(c)
    nb, T, K = c["B"], c["T"], c["n_fft"] // 2 + 1
    xbuf = torch.full((nb, T + 5), SENTINEL, device="cuda")
    xbuf[:, :T] = torch.from_numpy(xh).cuda()
    ys = K + 3                                                         # complex elements: 2K + 6 floats
    ybuf = torch.full((nb, frames * ys + 5), complex(SENTINEL, -SENTINEL), dtype=torch.complex64, device="cuda")
    out = ybuf[:, :frames * ys].view(nb, frames, ys)[:, :, :K]
    return xbuf[:, :T], ybuf, out


def _spectrum_gaps_intact(torch, ybuf, nb, frames, K):
    gaps = torch.ones_like(ybuf, dtype=torch.bool)
    gaps[:, :frames * (K + 3)].view(nb, frames, K + 3)[:, :, :K] = False
    return bool((torch.view_as_real(ybuf[gaps]) == torch.tensor([SENTINEL, -SENTINEL], device="cuda")).all())


def _padded_rows(torch, nb, frames, W):
    """A float32 buffer with gaps of 5 behind every row and 7 behind every signal (odd: no evenness rule), full of sentinels."""
    ys = W + 5
    buf = torch.full((nb, frames * ys + 7), SENTINEL, device="cuda")
    return buf, buf[:, :frames * ys].view(nb, frames, ys)[:, :, :W]


def _row_gaps_intact(torch, buf, nb, frames, W):
    gaps = torch.ones_like(buf, dtype=torch.bool)
    gaps[:, :frames * (W + 5)].view(nb, frames, W + 5)[:, :, :W] = False
    return bool((buf[gaps] == SENTINEL).all())


def _fbits(t):
    return t.contiguous().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("cid", MC.case_ids())
def test_accuracy_within_twice_rocfft_on_the_same_rows_and_the_named_form(torch, cid):
    c = MC.case(cid)
    p = MC.params(c["setup"])
    form = c.get("form", "spectrum")
    xh = _case_signal(c)
    v = _v(p, c["L"])
    rows = _rows_ref(c, xh, v)
    x = torch.from_numpy(xh).cuda()
    parent = _parent_rows(torch, p, c, x)
    assert _same(parent.cpu().numpy(), rows), "the parent's rows are the restated rows"
    yard = _row_errors(torch.fft.rfft(parent, dim=-1).cpu().numpy(), rows)
    nb, frames, K = c["B"], rows.shape[1], c["n_fft"] // 2 + 1
    cs = dict(c, form="spectrum")
    if c.get("padded"):
        xv, ybuf, out = _padded_io(torch, cs, xh)
        Y = _call(torch, p, c, xv, out=out)
        assert Y.data_ptr() == out.data_ptr() and _spectrum_gaps_intact(torch, ybuf, nb, frames, K), "a gap was written"
    else:
        xv = x
        Y = _call(torch, p, c, x)
    assert Y.dtype == torch.complex64 and tuple(Y.shape) == rows.shape[:2] + (K,)
    w, fb = _mel(torch, c["n_fft"]) if form == "bank" else (None, None)
    with bhw.ResidentTable(p) as tab:
        d = MC.parse(MC.line(cs, table=tab._live()))
        assert d["table"] and "k_stft_mfft_table" in d["kernels"], d["line"]
        Yt = _call(torch, p, c, x, table=tab)
        Pt = _spec(torch, p, c, x, fb, table=tab) if form != "spectrum" else None
        torch.cuda.synchronize()
    Yh = Y.cpu().numpy()
    assert _same(torch.view_as_real(Yt).cpu().numpy(), np.ascontiguousarray(Yh).view(np.float32).reshape(Yh.shape + (2,))), "library against table"
    err = _row_errors(Yh, rows)
    cap = 2.0 ** -24 * math.log2(c["n_fft"])
    print(f"stft mixed {cid}: n_fft {c['n_fft']} L {c['L']} rows {rows.shape[0] * rows.shape[1]}: fused {err:.3e}, torch.fft.rfft on the parent's rows "
          f"{yard:.3e}, ratio {err / yard:.3f}, cap {cap:.3e}, fused / cap {err / cap:.3f}")
    assert err <= 2.0 * yard, (cid, err, yard)
    assert err <= cap, (cid, err, cap)
    # the purely real bins: +0.0, not -0.0
    im = np.ascontiguousarray(Yh.imag).view(np.uint32)
    assert not im[..., 0].any() and not im[..., -1].any()
    if form == "spectrum":
        return
    # the named form, bit for bit the values computed on the host from stft_mixed of the same call
    want = _power_ref(Yh).reshape(-1, K)
    W = K
    if form == "bank":
        assert (fb.filters, fb.bins) == (MC.BANK_FILTERS, K)
        want, widths = _bank_ref(want, w)
        W = fb.filters
    if c.get("padded"):
        buf, out = _padded_rows(torch, nb, frames, W)
        got = _spec(torch, p, c, xv, fb, out=out)
        assert got.data_ptr() == out.data_ptr() and _row_gaps_intact(torch, buf, nb, frames, W), "a gap was written"
    else:
        got = _spec(torch, p, c, x, fb)
    assert got.dtype == torch.float32 and tuple(got.shape) == (nb, frames, W)
    gh = _fbits(got).reshape(-1, W)
    assert np.array_equal(_fbits(Pt).reshape(-1, W), gh), "library against table"
    bad = np.flatnonzero((gh != want.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (cid, bad[:5], gh[bad[:1]], want.view(np.uint32)[bad[:1]])
    if form == "bank":
        assert not gh[:, np.flatnonzero(widths == 0)].any(), "an empty filter gives +0.0"


def test_whisper_front_end_power_and_bank_bit_for_bit(torch):
    """400 / 160 / 80 mel at 16 kHz with the bank bhw.FilterBank(bhw.mel_weights(400, 80, 16000)): power and bank rows from the
    spectrum of the same call, library and table, centred and as detrended Welch segments."""
    p = B.make_params(B.WIN_HANN, 10, 16)
    w, fb = _mel(torch, 400)
    rng = np.random.default_rng(21)
    x = torch.from_numpy((rng.standard_normal((3, 8000)) * 300 + 2).astype(np.float32)).cuda()
    with bhw.ResidentTable(p) as tab:
        for kw in (dict(), dict(center=False, detrend=True, win_length=320)):
            Y = bhw.stft_mixed(p, x, 400, 160, **kw)
            P = _power_ref(Y.cpu().numpy()).reshape(-1, 201)
            M, _ = _bank_ref(P, w)
            for src in (bhw, tab):
                assert np.array_equal(_fbits(src.spectrogram_mixed(p, x, 400, 160, **kw)).reshape(-1, 201), P.view(np.uint32))
                got = src.spectrogram_mixed(p, x, 400, 160, fbank=fb, **kw)
                assert tuple(got.shape) == (3, Y.shape[1], 80)
                assert np.array_equal(_fbits(got).reshape(-1, 80), M.view(np.uint32))
            one = bhw.spectrogram_mixed(p, x[1], 400, 160, fbank=fb, **kw)
            assert one.dim() == 2 and torch.equal(one, got[1])
        torch.cuda.synchronize()


@pytest.mark.parametrize("cid", ["n18-l13-detrend", "n30-l24-constant-power", "n400-reflect-bank", "n1000-detrend", "n4050-reflect"])
def test_a_row_depends_on_nothing_but_itself(torch, cid):
    """The same signal alone and as signal 37 of a batch of 64; its later rows as the first rows of a shifted copy (another slot of the
    workgroup and another group: rows per workgroup are a function of n_fft alone in this plan, so a row changes class by changing its
    place) -- every frame where there is no padding, the frames no padding reaches where there is; packed against padded strides, the
    sentinels of the gaps intact.  Word for word."""
    c = dict(MC.case(cid), B=1, form="spectrum")
    p = MC.params(c["setup"])
    T = min(c["T"], 6 * c["n_fft"] + 40 * c["hop"]) if c["hop"] < c["n_fft"] else c["T"]
    c["T"] = T
    rng = np.random.default_rng(7)
    xh = (rng.standard_normal((64, T)) * 100 + 3).astype(np.float32)
    x = torch.from_numpy(xh).cuda()
    alone = _call(torch, p, c, x[37:38].clone())
    batch = _call(torch, p, dict(c, B=64), x)
    assert np.array_equal(_bits(torch, alone[0]), _bits(torch, batch[37]))
    if c["detrend"] or not c["mode"]:                                  # no padding: frame f + 3 of x is frame f of x[3 * hop:]
        shifted = _call(torch, p, dict(c, T=T - 3 * c["hop"]), x[37:38, 3 * c["hop"]:].clone())
        assert shifted.shape[1] == alone.shape[1] - 3
        assert np.array_equal(_bits(torch, shifted[0]), _bits(torch, alone[0, 3:]))
    else:                                                              # centred: the same holds for the frames no padding reaches
        n, hop, pad = c["n_fft"], c["hop"], c["n_fft"] // 2
        shifted = _call(torch, p, dict(c, T=T - 3 * hop), x[37:38, 3 * hop:].clone())
        inner = [f for f in range(shifted.shape[1]) if f * hop - pad >= 0 and f * hop - pad + n <= T - 3 * hop]
        assert len(inner) >= 4
        assert np.array_equal(_bits(torch, shifted[0, inner]), _bits(torch, alone[0, [f + 3 for f in inner]]))
    cp = dict(c, B=5, padded=True)
    xv, ybuf, out = _padded_io(torch, cp, xh[35:40])
    _call(torch, p, cp, xv, out=out)
    assert np.array_equal(_bits(torch, out[2]), _bits(torch, alone[0]))
    assert _spectrum_gaps_intact(torch, ybuf, 5, out.shape[1], out.shape[2]), "a gap was written"
    with bhw.ResidentTable(p) as tab:
        assert np.array_equal(_bits(torch, _call(torch, p, c, x[37:38].clone(), table=tab)), _bits(torch, alone))
        torch.cuda.synchronize()


def test_zero_signal_gives_zeros_and_a_nan_reaches_only_its_rows(torch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    n_fft, L, hop, T = 400, 320, 160, 8000
    z = bhw.stft_mixed(p, torch.zeros((2, T), device="cuda"), n_fft, hop, win_length=L)
    assert not bool(torch.view_as_real(z).ne(0).any())
    assert not bool(bhw.spectrogram_mixed(p, torch.zeros((2, T), device="cuda"), n_fft, hop, win_length=L).ne(0).any())
    rng = np.random.default_rng(3)
    xh = (rng.standard_normal((3, T)) * 10 + 1).astype(np.float32)
    for detrend in (False, True):
        kw = dict(win_length=L, center=False, detrend=detrend)
        clean = bhw.stft_mixed(p, torch.from_numpy(xh).cuda(), n_fft, hop, **kw)
        cleanp = bhw.spectrogram_mixed(p, torch.from_numpy(xh).cuda(), n_fft, hop, **kw)
        for bad in (np.nan, np.inf):
            xn = xh.copy()
            t0 = 4000
            xn[1, t0] = bad
            got = bhw.stft_mixed(p, torch.from_numpy(xn).cuda(), n_fft, hop, **kw)
            gotp = bhw.spectrogram_mixed(p, torch.from_numpy(xn).cuda(), n_fft, hop, **kw)
            frames = clean.shape[1]
            col0 = 0 if detrend else (n_fft - L) // 2
            hit = np.zeros((3, frames), dtype=bool)
            for f in range(frames):
                hit[1, f] = f * hop + col0 <= t0 < f * hop + col0 + L
            assert hit.sum() in (2, 3)
            finite = torch.isfinite(torch.view_as_real(got)).all(-1).all(-1).cpu().numpy()
            assert np.array_equal(~finite, hit), (detrend, bad)
            assert np.array_equal(_bits(torch, got)[~hit], _bits(torch, clean)[~hit])
            assert np.array_equal(~torch.isfinite(gotp).all(-1).cpu().numpy(), hit), (detrend, bad)
            assert np.array_equal(_fbits(gotp)[~hit], _fbits(cleanp)[~hit])


def test_graph_capture(torch):
    """The from-table calls captured with NO warm call, and the library calls (no bhw_prepare_device); replayed on new data, the
    results equal eager calls."""
    p = B.make_params(B.WIN_BH4, 12, 24)
    n_fft, hop, T, nb = 400, 160, 16000, 4
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((nb, T), device="cuda", generator=g) + 5.0
    _, fb = _mel(torch, n_fft)                                          # built (and synchronised) before the capture
    with bhw.ResidentTable(p) as tab:
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                outs = [tab.stft_mixed(p, x, n_fft, hop), tab.spectrogram_mixed(p, x, n_fft, hop), tab.spectrogram_mixed(p, x, n_fft, hop, fbank=fb),
                        bhw.stft_mixed(p, x, n_fft, hop), bhw.spectrogram_mixed(p, x, n_fft, hop), bhw.spectrogram_mixed(p, x, n_fft, hop, fbank=fb)]
        torch.cuda.current_stream().wait_stream(s)
        x.copy_(torch.randn((nb, T), device="cuda", generator=g) * 3.0 - 2.0)
        for o in outs:
            o.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        eager = [tab.stft_mixed(p, x, n_fft, hop), tab.spectrogram_mixed(p, x, n_fft, hop), tab.spectrogram_mixed(p, x, n_fft, hop, fbank=fb)]
        for o, e in zip(outs, eager + eager):
            a, b = (torch.view_as_real(u) if u.is_complex() else u for u in (o, e))
            assert torch.equal(a, b)
        assert tuple(outs[0].shape) == (nb, 1 + T // hop, 201) and tuple(outs[2].shape) == (nb, 1 + T // hop, 80)
        assert bool((outs[1] >= 0).all()) and bool((outs[2] >= 0).all())
        torch.cuda.synchronize()


def test_against_torch_stft(torch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn((3, 5000), device="cuda", generator=g)
    for n_fft, L, hop, center, mode in ((400, 400, 160, True, "reflect"), (480, 400, 120, True, "reflect"), (96, 80, 24, False, "reflect")):
        v = bhw.window(p, L, dtype=torch.float32)
        want = torch.stft(x, n_fft, hop, L, window=v, center=center, pad_mode=mode, return_complex=True)
        got = bhw.stft_mixed(p, x, n_fft, hop, win_length=L, center=center, pad_mode=mode).transpose(-1, -2)
        assert got.shape == want.shape
        assert float((got - want).abs().max() / want.abs().max()) < 1e-5
        one = bhw.stft_mixed(p, x[1], n_fft, hop, win_length=L, center=center, pad_mode=mode)
        assert one.dim() == 2 and torch.equal(torch.view_as_real(one), torch.view_as_real(got.transpose(-1, -2)[1]))


def test_composed_welch_against_the_default_route(torch):
    """welch_psd(stft_mixed(..., detrend=True, center=False), scale, nfft=400) is the fused Welch estimate at nperseg = nfft = 400:
    against bhw.welch(p, x, length=400) on the default route and the float64 restatement of scipy.signal.welch, by _rel_err, within
    twice the torch-only float32 route's error -- the bound of test_gpu_stft_fft.py for fft="fused"."""
    p = B.make_params(B.WIN_BH7, 16, 32)
    L, noverlap, nfft = 400, 240, 400
    xh = _test_signal(200000, 5)
    x = torch.from_numpy(xh).cuda()
    vh = _v(p, L)
    fr, ref = _welch_ref64(xh, vh, 1.0, L, noverlap, nfft, True)
    f, Pd = bhw.welch(p, x, 1.0, length=L, noverlap=noverlap)
    assert np.allclose(f.cpu().numpy(), fr, rtol=0, atol=1e-15)
    with bhw.ResidentTable(p) as tab:
        outs = []
        for src in (bhw, tab):
            Y = src.stft_mixed(p, x, nfft, L - noverlap, win_length=L, center=False, detrend=True)
            scale = B.welch_scale(bhw.window_sums(p, L, f32=True), Y.shape[-2], 1.0, "density")
            outs.append(bhw.welch_psd(Y, scale, nfft=nfft))
        torch.cuda.synchronize()
    P = outs[0]
    assert torch.equal(P, outs[1]) and tuple(P.shape) == tuple(Pd.shape) == (nfft // 2 + 1,)
    yard = _rel_err(_welch_torch_route(torch, x, torch.from_numpy(vh).cuda(), 1.0, L, noverlap, nfft).cpu().numpy(), ref)
    err = _rel_err(P.cpu().numpy(), ref)
    base = _rel_err(Pd.cpu().numpy(), ref)
    gap = _rel_err(P.cpu().numpy(), Pd.cpu().numpy().astype(np.float64))
    print(f"composed welch L={L} nfft={nfft} hop={L - noverlap}: stft_mixed + welch_psd {err:.3e}, bhw.welch default route {base:.3e}, torch-only route "
          f"{yard:.3e}, ratio {err / yard:.3f}, against the default route {gap:.3e}")
    assert err <= 2.0 * yard, (err, yard)
    assert gap <= 2.0 * yard, (gap, yard)


def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    x = torch.zeros((2, 4000), device="cuda")
    xc = torch.zeros((2, 4000), dtype=torch.complex64, device="cuda")
    for fn in (bhw.stft_mixed, bhw.spectrogram_mixed):
        with pytest.raises(ValueError, match="real float32"):
            fn(p, xc, 400, 160)
        with pytest.raises(ValueError, match=r"power of two: bhw\.stft"):
            fn(p, x, 512, 160)
        with pytest.raises(ValueError, match=r"power of two: bhw\.stft"):
            fn(p, x, 8, 4)
        for n in (405, 420, 14, 4500):
            with pytest.raises(ValueError, match=r"even 2\^a·3\^b·5\^c in 16\.\.4095"):
                fn(p, x, n, 16, win_length=8)
        with pytest.raises(ValueError, match="center=False"):
            fn(p, x, 400, 160, detrend=True)
        with pytest.raises(ValueError, match="pad_mode"):
            fn(p, x, 400, 160, pad_mode="edge")
        with pytest.raises(ValueError, match="CUDA tensor"):
            fn(p, x.cpu(), 400, 160)
    with pytest.raises(ValueError, match="out must be"):
        bhw.stft_mixed(p, x, 400, 160, out=torch.zeros((2, 26, 201), device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        bhw.spectrogram_mixed(p, x, 400, 160, out=torch.zeros((2, 26, 201), dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError, match="FilterBank"):
        bhw.spectrogram_mixed(p, x, 400, 160, fbank=bhw.mel_weights(400, 80, 16000))
    with pytest.raises(ValueError, match="257 bins"):
        bhw.spectrogram_mixed(p, x, 400, 160, fbank=_mel(torch, 512)[1])
    # the power-of-two calls still refuse these sizes
    with pytest.raises(ValueError, match="power of two"):
        bhw.stft(p, x, 400, 160)
    with pytest.raises(ValueError, match="power of two"):
        bhw.spectrogram(p, x, 400, 160)
    with pytest.raises(ValueError, match="power of two"):
        bhw.welch(p, x, length=400, fft="fused")
    with bhw.ResidentTable(p) as tab:
        with pytest.raises(ValueError, match=r"power of two: bhw\.stft"):
            tab.stft_mixed(p, x, 512, 160)
        assert tuple(tab.stft_mixed(p, x, 400, 160).shape) == (2, 26, 201)
        torch.cuda.synchronize()
