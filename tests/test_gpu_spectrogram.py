"""The fused spectrogram on the GPU (bhw_spectrogram_f32_* through bhw.spectrogram and ResidentTable.spectrogram).

The gate is exact.  A power row is defined on the bits of the bins bhw.stft writes, so for every case of tests/spectrogram_cases.py
the output is compared word for word with fl32(re^2 + im^2) computed in numpy float64 from bhw.stft of the same call on the same GPU;
a bank row with the ascending binary64 loop over those powers and the bank's float32 weights.  The FFT's accuracy is gated where the
FFT is (test_gpu_stft_fft.py) and only the end-to-end test below looks at it again, against the torch route under the project's
yardstick: at most twice the torch route's error on the same GPU."""
import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from blackman_harris_win_amd.selector import fbank_bands

import spectrogram_cases as SC

pytestmark = pytest.mark.gpu

SENTINEL = 12345.5


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _signal(nb, T, seed=0):
    """(nb, T) float32: noise of 1000 + tones of 1e3 and 1e-3 + an offset."""
    rng = np.random.default_rng(2000 + seed)
    n = np.arange(T, dtype=np.float64)
    x = rng.standard_normal((nb, T)) * 1000 + 1e3 * np.cos(2 * np.pi * 0.1234 * n) + 1e-3 * np.cos(2 * np.pi * 0.31 * n + 1.0) + 250.0
    return x.astype(np.float32)


def _kw(c):
    if c["detrend"]:
        return dict(win_length=c["L"], center=False, detrend=True)
    return dict(win_length=c["L"], center=bool(c["mode"]), pad_mode=c["mode"] or "reflect")


def _power_ref(Yh):
    """fl32((double) re * re + (double) im * im) of a complex64 array: both squares exact in float64, one rounding, one rounding."""
    re, im = Yh.real.astype(np.float64), Yh.imag.astype(np.float64)
    return (re * re + im * im).astype(np.float32)


def _bank_ref(P, w):
    """The contract's sum for every row of P (R, K) float32 through the dense bank w: per filter over its band in ascending i, in
    float64 from +0.0 (each product of two float32 is exact in float64, so `acc += p * w` rounds once, as a fused multiply-add does).
    One Python loop over i, vectorised over rows and filters."""
    first, offset, weight = fbank_bands(w)
    first, offset = first.astype(np.int64), offset.astype(np.int64)
    c = np.diff(offset)
    P64, w64 = P.astype(np.float64), weight.astype(np.float64)
    acc = np.zeros((P.shape[0], w.shape[1]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(int(c.max()) if c.size else 0):
            act = np.flatnonzero(c > i)
            acc[:, act] += P64[:, first[act] + i] * w64[offset[act] + i][None, :]
        return acc.astype(np.float32), c


def _bits(t):
    return t.contiguous().cpu().numpy().view(np.uint32)


def _padded_out(torch, nb, frames, W):
    """A float32 buffer with gaps of 3 behind every row and 7 behind every signal, full of sentinels, and the (nb, frames, W) view."""
    ys = W + 3
    buf = torch.full((nb, frames * ys + 7), SENTINEL, device="cuda")
    return buf, buf[:, :frames * ys].view(nb, frames, ys)[:, :, :W]


def _gaps_intact(torch, buf, nb, frames, W):
    gaps = torch.ones_like(buf, dtype=torch.bool)
    gaps[:, :frames * (W + 3)].view(nb, frames, W + 3)[:, :, :W] = False
    return bool((buf[gaps] == SENTINEL).all())


_FBANKS = {}


def _fbank(c):
    """The device FilterBank of a case (built once per bank: the upload synchronises)."""
    w = SC.bank(c)
    if w is None:
        return None
    key = (c["n_fft"], c["bank"])
    if key not in _FBANKS:
        _FBANKS[key] = bhw.FilterBank(w, device="cuda")
    return _FBANKS[key]


@pytest.mark.parametrize("cid", SC.case_ids())
def test_bit_for_bit_from_the_stft_of_the_same_call(torch, cid):
    c = SC.case(cid)
    p = SC.params(c["setup"])
    w, fb = SC.bank(c), _fbank(c)
    nb, W = c["B"], SC.width(c)
    xh = _signal(nb, c["T"])
    if c.get("padded"):
        xbuf = torch.full((nb, c["T"] + 5), SENTINEL, device="cuda")
        xbuf[:, :c["T"]] = torch.from_numpy(xh).cuda()
        x = xbuf[:, :c["T"]]
    else:
        x = torch.from_numpy(xh).cuda()
    Y = bhw.stft(p, x, c["n_fft"], c["hop"], **_kw(c))
    frames, K = Y.shape[1], Y.shape[2]
    assert frames == SC.desc(c)[2] and K == c["n_fft"] // 2 + 1
    want = _power_ref(Y.cpu().numpy()).reshape(-1, K)
    if w is not None:
        assert (fb.filters, fb.bins, np.array_equal(fb.dense(), w)) == (W, K, True)
        want, widths = _bank_ref(want, w)
    if c.get("padded"):
        buf, out = _padded_out(torch, nb, frames, W)
        got = bhw.spectrogram(p, x, c["n_fft"], c["hop"], fbank=fb, out=out, **_kw(c))
        assert got.data_ptr() == out.data_ptr() and _gaps_intact(torch, buf, nb, frames, W), "a gap was written"
    else:
        got = bhw.spectrogram(p, x, c["n_fft"], c["hop"], fbank=fb, **_kw(c))
    assert got.dtype == torch.float32 and tuple(got.shape) == (nb, frames, W)
    with bhw.ResidentTable(p) as tab:
        d = SC.parse(SC.line(c, table=tab._live()))
        assert d["table"] and "k_spectrogram_table" in d["kernels"], d["line"]
        gt = tab.spectrogram(p, x, c["n_fft"], c["hop"], fbank=fb, **_kw(c))
        torch.cuda.synchronize()
    gh = _bits(got).reshape(-1, W)
    assert np.array_equal(_bits(gt).reshape(-1, W), gh), "library against table"
    bad = np.flatnonzero((gh != want.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (cid, bad[:5], gh[bad[:1]], want.view(np.uint32)[bad[:1]])
    if w is not None:
        empty = np.flatnonzero(widths == 0)
        assert not gh[:, empty].any(), "an empty filter gives +0.0"
        if "the identity bank" in c["classes"]:
            assert np.array_equal(_bits(bhw.spectrogram(p, x, c["n_fft"], c["hop"], **_kw(c))).reshape(-1, K), gh)


@pytest.mark.parametrize("n_fft,hop,L,filters", [(64, 16, 49, 10), (2048, 512, 2048, 128)])
def test_a_row_depends_on_nothing_but_itself(torch, n_fft, hop, L, filters):
    """A signal alone, as signal 37 of 64, shifted by three hops (another slot and another group), into padded strides, and library
    against table: equal rows word for word, in both modes."""
    p = B.make_params(B.WIN_BH7, 12, 32)
    T = 6 * n_fft + 40 * hop
    rng = np.random.default_rng(7)
    xh = (rng.standard_normal((64, T)) * 100 + 3).astype(np.float32)
    x = torch.from_numpy(xh).cuda()
    fbm = bhw.FilterBank(bhw.mel_weights(n_fft, filters, 16000), device="cuda")
    kw = dict(win_length=L, center=False)
    for fb in (None, fbm):
        W = n_fft // 2 + 1 if fb is None else filters
        alone = bhw.spectrogram(p, x[37:38].clone(), n_fft, hop, fbank=fb, **kw)
        batch = bhw.spectrogram(p, x, n_fft, hop, fbank=fb, **kw)
        assert np.array_equal(_bits(alone[0]), _bits(batch[37]))
        shifted = bhw.spectrogram(p, x[37:38, 3 * hop:].clone(), n_fft, hop, fbank=fb, **kw)   # frame f + 3 of x is frame f of x[3 * hop:]
        assert shifted.shape[1] == alone.shape[1] - 3
        assert np.array_equal(_bits(shifted[0]), _bits(alone[0, 3:]))
        frames = alone.shape[1]
        buf, out = _padded_out(torch, 5, frames, W)
        bhw.spectrogram(p, x[35:40], n_fft, hop, fbank=fb, out=out, **kw)
        assert np.array_equal(_bits(out[2]), _bits(alone[0])) and _gaps_intact(torch, buf, 5, frames, W)
        one = bhw.spectrogram(p, x[37], n_fft, hop, fbank=fb, **kw)
        assert one.dim() == 2 and np.array_equal(_bits(one), _bits(alone[0]))
        with bhw.ResidentTable(p) as tab:
            assert np.array_equal(_bits(tab.spectrogram(p, x[37:38].clone(), n_fft, hop, fbank=fb, **kw)), _bits(alone))
            torch.cuda.synchronize()


def test_zeros_give_zeros_and_a_nan_reaches_only_its_rows(torch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    n_fft, L, hop, T = 256, 200, 80, 4000
    w = bhw.mel_weights(n_fft, 80, 16000)                          # two empty filters
    fb = bhw.FilterBank(w, device="cuda")
    empty = np.flatnonzero(np.diff(fbank_bands(w)[1].astype(np.int64)) == 0)
    assert empty.size == 2
    for f in (None, fb):
        z = bhw.spectrogram(p, torch.zeros((2, T), device="cuda"), n_fft, hop, win_length=L, fbank=f)
        assert not _bits(z).any(), "zeros in give +0.0 out"
    rng = np.random.default_rng(3)
    xh = (rng.standard_normal((3, T)) * 10 + 1).astype(np.float32)
    for detrend in (False, True):
        kw = dict(win_length=L, center=False, detrend=detrend)
        for f in (None, fb):
            clean = bhw.spectrogram(p, torch.from_numpy(xh).cuda(), n_fft, hop, fbank=f, **kw)
            for bad in (np.nan, np.inf):
                xn = xh.copy()
                t0 = 2000
                xn[1, t0] = bad
                got = bhw.spectrogram(p, torch.from_numpy(xn).cuda(), n_fft, hop, fbank=f, **kw)
                frames = clean.shape[1]
                col0 = 0 if detrend else (n_fft - L) // 2
                hit = np.zeros((3, frames), dtype=bool)
                for fr in range(frames):
                    hit[1, fr] = fr * hop + col0 <= t0 < fr * hop + col0 + L
                assert hit.sum() in (2, 3)
                gh = got.cpu().numpy()
                cols = np.ones(gh.shape[-1], dtype=bool)
                if f is not None:
                    cols[empty] = False
                    assert not _bits(got)[..., empty].any(), "the empty filters of a non-finite row stay +0.0"
                assert np.array_equal(~np.isfinite(gh[..., cols]).all(-1), hit), (detrend, bad)
                assert not np.isfinite(gh[hit][:, cols]).any(), "every bin of a row under a NaN or an infinity is non-finite"
                assert np.array_equal(_bits(got)[~hit], _bits(clean)[~hit])


def _row_err(got, ref):
    """max over rows of |got - ref|_2 / |ref|_2"""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1, ref.shape[-1]), ref.reshape(-1, ref.shape[-1])
    return float((np.sqrt(((got - ref) ** 2).sum(-1)) / np.sqrt((ref ** 2).sum(-1))).max())


@pytest.mark.parametrize("L,n_fft,hop,n_mels", [(400, 512, 160, 80), (64, 64, 16, 10)])
def test_end_to_end_within_twice_the_torch_route(torch, L, n_fft, hop, n_mels):
    """Against torch.stft(...).abs() ** 2 times the dense bank: shape, layout after transposing, values.  Metric: the largest relative
    l2 error of a row against a float64 numpy reference of the float32 rows (the windowed frames stft_frames writes, transformed,
    squared and folded in float64); bound: twice the same figure for the torch route on the same GPU.
    Measured on an MI355X: see DESIGN.md section 20."""
    p = B.make_params(B.WIN_BH7, 12, 32)
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn((3, 16000), device="cuda", generator=g) * 100 + 5
    mel = bhw.mel_weights(n_fft, n_mels, 16000)
    bank_dev = torch.from_numpy(mel).cuda()
    v = bhw.window(p, L, dtype=torch.float32)
    S = torch.stft(x, n_fft, hop, L, window=v, center=True, pad_mode="reflect", return_complex=True)
    want_pow = S.abs() ** 2                                                      # (B, K, F)
    want_mel = torch.matmul(want_pow.transpose(-1, -2), bank_dev).transpose(-1, -2)   # (B, n_mels, F)
    fb = bhw.FilterBank(mel, device="cuda")
    got_pow = bhw.spectrogram(p, x, n_fft, hop, win_length=L)
    got_mel = bhw.spectrogram(p, x, n_fft, hop, win_length=L, fbank=fb)
    assert got_pow.transpose(-1, -2).shape == want_pow.shape and got_mel.transpose(-1, -2).shape == want_mel.shape
    assert got_pow.is_contiguous() and got_mel.is_contiguous() and got_mel.dtype == torch.float32
    rows = bhw.stft_frames(p, x, n_fft, hop, win_length=L).cpu().numpy().astype(np.float64)
    ref_pow = np.abs(np.fft.rfft(rows, axis=-1)) ** 2                            # (B, F, K)
    ref_mel = ref_pow @ mel.astype(np.float64)
    for name, got, want, ref in (("power", got_pow, want_pow, ref_pow), ("mel", got_mel, want_mel, ref_mel)):
        err = _row_err(got.cpu().numpy(), ref)
        yard = _row_err(want.transpose(-1, -2).cpu().numpy(), ref)
        print(f"spectrogram end to end {L} / {n_fft} / {hop}, {n_mels} mels, {name}: fused {err:.3e}, torch route {yard:.3e}, ratio {err / yard:.3f}")
        assert err <= 2.0 * yard, (name, err, yard)
    one = bhw.spectrogram(p, x[1], n_fft, hop, win_length=L, fbank=fb)
    assert one.dim() == 2 and torch.equal(one, got_mel[1])


def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    x = torch.zeros((2, 4000), device="cuda")
    xc = torch.zeros((2, 4000), dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError, match="real float32"):
        bhw.spectrogram(p, xc, 64, 16)
    with pytest.raises(ValueError, match="power of two"):
        bhw.spectrogram(p, x, 100, 16)
    with pytest.raises(ValueError, match="power of two"):
        bhw.spectrogram(p, x, 8, 4)
    with pytest.raises(ValueError, match="center=False"):
        bhw.spectrogram(p, x, 64, 16, detrend=True)
    fb = bhw.FilterBank(bhw.mel_weights(128, 10, 16000), device="cuda")
    assert (fb.filters, fb.bins) == (10, 65) and fb.weights > 0 and fb.dense().shape == (65, 10)
    with pytest.raises(ValueError, match="65 bins"):
        bhw.spectrogram(p, x, 64, 16, fbank=fb)
    with pytest.raises(ValueError, match="FilterBank"):
        bhw.spectrogram(p, x, 64, 16, fbank=torch.zeros((33, 10), device="cuda"))
    with pytest.raises(ValueError, match="CUDA device"):
        bhw.FilterBank(bhw.mel_weights(64, 10, 16000), device="cpu")
    if torch.cuda.device_count() > 1:
        other = bhw.FilterBank(bhw.mel_weights(64, 10, 16000), device="cuda:1")
        with pytest.raises(ValueError, match="the filter bank is on"):
            bhw.spectrogram(p, x, 64, 16, fbank=other)
    else:                                                                        # one device: a bank that claims another one
        other = bhw.FilterBank(bhw.mel_weights(64, 10, 16000), device="cuda")
        other.device = torch.device("cuda", 1)
        with pytest.raises(ValueError, match="the filter bank is on"):
            bhw.spectrogram(p, x, 64, 16, fbank=other)
    with pytest.raises(ValueError, match="out must be"):
        bhw.spectrogram(p, x, 64, 16, out=torch.zeros((2, 10, 33), device="cuda"))
    frames = 1 + 4000 // 16
    with pytest.raises(ValueError, match="out must be"):
        bhw.spectrogram(p, x, 64, 16, out=torch.zeros((2, frames, 33), dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        bhw.spectrogram(p, x, 64, 16, out=torch.zeros((2, 33, frames), device="cuda").transpose(-1, -2))
    ok = bhw.spectrogram(p, x, 64, 16, out=torch.ones((2, frames, 33), device="cuda"))
    assert not bool(ok.ne(0).any())
    torch.cuda.synchronize()


def test_graph_capture(torch):
    """ResidentTable.spectrogram and bhw.spectrogram captured with no warm call, with a bank and without; replayed on new data, the
    result equals an eager call."""
    p = B.make_params(B.WIN_BH4, 12, 24)
    L, n_fft, hop, T, nb = 400, 512, 160, 16000, 4
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((nb, T), device="cuda", generator=g) + 5.0
    fb = bhw.FilterBank(bhw.mel_weights(n_fft, 80, 16000), device="cuda")         # built (and synchronised) before the capture
    with bhw.ResidentTable(p) as tab:
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                outs = [tab.spectrogram(p, x, n_fft, hop, win_length=L), tab.spectrogram(p, x, n_fft, hop, win_length=L, fbank=fb),
                        bhw.spectrogram(p, x, n_fft, hop, win_length=L), bhw.spectrogram(p, x, n_fft, hop, win_length=L, fbank=fb)]
        torch.cuda.current_stream().wait_stream(s)
        x.copy_(torch.randn((nb, T), device="cuda", generator=g) * 3.0 - 2.0)
        for o in outs:
            o.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        eager = [tab.spectrogram(p, x, n_fft, hop, win_length=L), tab.spectrogram(p, x, n_fft, hop, win_length=L, fbank=fb)]
        for o, e in zip(outs, eager + eager):
            assert torch.equal(o, e) and bool((o >= 0).all())
        assert tuple(outs[1].shape) == (nb, 1 + T // hop, 80)
        torch.cuda.synchronize()
