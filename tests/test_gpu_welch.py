"""Welch's method around the FFT on the GPU (bhw_window_sums_* / bhw_welch_frames_f32_* / bhw_welch_psd_f32, bhw.welch): the window sums
against Python-int sums of the generated window; the segments without detrending bit for bit against the stft frames call, with
detrending bit for bit against a NumPy restatement of the order include/bhw.h writes down; the averaged periodogram bit for bit against
its NumPy restatement; graph capture; the Python errors; and bhw.welch end to end against a float64 restatement of scipy.signal.welch,
inside twice the error of the torch-only float32 route measured in the same run."""
import ctypes

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from test_gpu_stft import SETUPS, SPECIAL, _same

pytestmark = pytest.mark.gpu

BLOCK = B.WELCH_BLOCK
LENGTHS = (1, 2, 63, 64, 65, 400, 4096)
# (setup index, L, nfft, hop, C, batch, T): L < 64, L = 64 at hop = L, L not a multiple of 64 with nfft > L and B = 64, two channels,
# L = 4096 with hop above L, L above 4096 not a multiple of 64 in a longer row
FRAMINGS = [(1, 13, 13, 5, 1, 3, 100), (3, 64, 64, 64, 2, 1, 640), (0, 100, 128, 37, 1, 64, 500), (2, 400, 512, 160, 2, 3, 2000),
            (0, 4096, 4096, 5000, 1, 2, 20000), (4, 4100, 8192, 1000, 1, 1, 30000), (1, 1, 4, 1, 2, 64, 9), (4, 65, 65, 65, 1, 3, 400)]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _params(i):
    win, P, W, kw = SETUPS[i % len(SETUPS)]
    return B.make_params(win, P, W, **kw)


def _v(p, L):
    w = bhw.window(p, L).cpu().numpy()
    return np.ldexp(w.astype(np.float32), -(p.dat_width - 1)).astype(np.float32)


def _signal(rng, shape, special=True, offset=0.0):
    x = (rng.standard_normal(shape) * 1000 + offset).astype(np.float32)
    if special:
        flat = x.reshape(-1)
        idx = rng.choice(flat.size, size=min(flat.size // 4 + 1, 2 * len(SPECIAL)), replace=False)
        flat[idx] = np.resize(SPECIAL, len(idx))
    return x


def _to_torch(torch, x, C):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return torch.view_as_complex(t) if C == 2 else t.squeeze(-1)


def _from_torch(torch, y, C):
    return (torch.view_as_real(y) if C == 2 else y.unsqueeze(-1)).cpu().numpy()


# ---- the restatements, written from include/bhw.h ------------------------------------------------------------------------------------

def _mean_ref(seg):
    """seg (..., L) float32 -> m float32: 64 partial sums over j = i (mod 64) in ascending j, the butterfly s = 32 .. 1, S = P[0],
    m = fl32(S / L)."""
    L = seg.shape[-1]
    P = np.zeros(seg.shape[:-1] + (64,), dtype=np.float64)
    with np.errstate(all="ignore"):
        for j0 in range(0, L, 64):                                  # ascending j inside every residue class
            chunk = seg[..., j0:j0 + 64].astype(np.float64)
            P[..., :chunk.shape[-1]] = P[..., :chunk.shape[-1]] + chunk
        for s in (32, 16, 8, 4, 2, 1):
            P[..., :s] = P[..., :s] + P[..., s:2 * s]               # the right side is formed before any element is written
        return (P[..., 0] / np.float64(L)).astype(np.float32)


def _segments_ref(x, v, nfft, hop, detrend):
    """x (B, T, C) float32 -> (B, F, nfft, C): scipy's segments, y = fl32(fl32(x - m) * v) for j < L, +0.0 behind."""
    nb, T, C = x.shape
    L = len(v)
    F = 1 + (T - L) // hop
    idx = np.arange(F)[:, None] * hop + np.arange(L)[None, :]
    seg = x[:, idx, :]                                              # (B, F, L, C)
    y = np.zeros((nb, F, nfft, C), dtype=np.float32)
    with np.errstate(all="ignore"):
        if detrend:
            m = _mean_ref(np.moveaxis(seg, 2, -1))                  # (B, F, C)
            seg = (seg - m[:, :, None, :]).astype(np.float32)       # one binary32 subtraction
        y[:, :, :L, :] = seg * v[None, None, :, None]               # one binary32 multiply
    return y


def _psd_ref(Y, scale, nfft, onesided):
    """Y (B, F, K) complex64 -> (B, K) float32: q in binary64, ascending f inside blocks of BLOCK frames, the blocks in order."""
    nb, F, K = Y.shape
    with np.errstate(all="ignore"):
        re, im = Y.real.astype(np.float64), Y.imag.astype(np.float64)
        q = re * re + im * im                                       # both squares exact: one rounding
        A = np.zeros((nb, K))
        for f0 in range(0, F, BLOCK):
            Ab = np.zeros((nb, K))
            for f in range(f0, min(F, f0 + BLOCK)):
                Ab = Ab + q[:, f, :]
            A = A + Ab
        s = np.full(K, np.float64(scale))
        if onesided:
            s[1:] *= 2.0
            if nfft % 2 == 0:
                s[-1] = np.float64(scale)
        return (A * s).astype(np.float32)


def _int_sums(w, f32):
    u = [int(t) for t in (w.astype(np.float32).astype(np.int64) if f32 else w.astype(np.int64)).tolist()]
    return sum(u), sum(t * t for t in u)


# ---- window sums ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("setup", range(len(SETUPS)))
def test_window_sums_equal_python_int_sums(torch, setup):
    p = _params(setup)
    N = 1 << p.phi_width
    with bhw.ResidentTable(p) as tab:
        for L in sorted({t for t in LENGTHS + (N,) if t <= N}):
            w = bhw.window(p, L).cpu().numpy()
            for f32 in (False, True):
                s1, s2 = _int_sums(w, f32)
                got = bhw.window_sums(p, L, f32=f32)
                assert (got["s1"], got["s2"]) == (s1, s2), (setup, L, f32, got, s1, s2)
                tb = tab.window_sums(p, L, f32=f32)
                assert (tb["s1"], tb["s2"]) == (s1, s2), (setup, L, f32, "table")
                sh = p.dat_width - 1
                assert got["S1"] == s1 / 2.0 ** sh or abs(s1) >= 1 << 53
                assert got["coherent_gain"] == got["S1"] / L
                if s1:
                    assert got["enbw_bins"] == L * got["S2"] / (got["S1"] * got["S1"])


def test_window_sums_long_windows(torch):
    """A 2^26-point 32-bit window, where the sum of squares exceeds 2^64, and one odd length above 2^16, against chunked Python-int sums."""
    p = B.make_params(B.WIN_BH7, 26, 32)
    with bhw.ResidentTable(p) as tab:
        for L in (100003, 1 << 26):
            w = bhw.window(p, L).cpu().numpy()
            for f32 in (True, False):
                s1 = s2 = 0
                for c0 in range(0, L, 1 << 16):                     # each chunk's partial sums fit 64 bits; the total is a Python int
                    u = w[c0:c0 + (1 << 16)]
                    u = (u.astype(np.float32) if f32 else u).astype(np.int64)
                    q = (u * u).astype(np.uint64)
                    s1 += int(u.sum())
                    s2 += (int((q >> np.uint64(32)).sum()) << 32) + int((q & np.uint64(0xFFFFFFFF)).sum())
                got, tb = bhw.window_sums(p, L, f32=f32), tab.window_sums(p, L, f32=f32)
                assert (got["s1"], got["s2"]) == (s1, s2), (L, f32, got["s1"] - s1, got["s2"] - s2)
                assert (tb["s1"], tb["s2"]) == (s1, s2), (L, f32, "table")
                if L == 1 << 26:
                    assert s2 > 1 << 64


# ---- segments ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", range(len(FRAMINGS)))
def test_segments_without_detrending_are_the_stft_frames(torch, case):
    setup, L, nfft, hop, C, nb, T = FRAMINGS[case]
    p = _params(setup)
    rng = np.random.default_rng(100 + case)
    F = 1 + (T - L) // hop
    # the stft call wants every row's n_fft columns inside the signal: it sees nfft - L samples more than the Welch call, which is
    # handed the strided view x[:, :T] of the same buffer
    Tp = T + (nfft - L)
    xh = _signal(rng, (nb, Tp, C))
    xt = _to_torch(torch, xh, C)
    xw = xt[:, :T]
    got = bhw.welch_frames(p, xw, L, hop, nfft=nfft, detrend=False)
    assert got.shape == (nb, F, nfft)
    want = torch.full_like(got, 7.0)
    s = B.make_stft(nb, Tp, F, hop, nfft, channels=C, shift=p.dat_width - 1, x_stride=Tp * C)
    B.check(B.lib().bhw_stft_frames_f32_device(ctypes.byref(p), L, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                                               ctypes.byref(s), ctypes.c_void_p(xt.data_ptr()), ctypes.c_void_p(want.data_ptr())))
    torch.cuda.synchronize()
    assert _same(_from_torch(torch, got, C), _from_torch(torch, want, C)), case
    assert _same(_from_torch(torch, got, C), _segments_ref(xh[:, :T], _v(p, L), nfft, hop, False)), case
    if nfft == L:
        st = bhw.stft_frames(p, xw, L, hop, center=False)
        assert _same(_from_torch(torch, got, C), _from_torch(torch, st, C)), case
    with bhw.ResidentTable(p) as tab:
        assert _same(_from_torch(torch, tab.welch_frames(p, xw, L, hop, nfft=nfft, detrend=False), C), _from_torch(torch, got, C)), case


@pytest.mark.parametrize("case", range(len(FRAMINGS)))
def test_detrended_segments_equal_the_header_order(torch, case):
    setup, L, nfft, hop, C, nb, T = FRAMINGS[case]
    p = _params(setup)
    rng = np.random.default_rng(200 + case)
    v = _v(p, L)
    with bhw.ResidentTable(p) as tab:
        for variant in ("plain", "special", "offset", "strided"):
            Tbuf = T + 7 if variant == "strided" else T
            xh = _signal(rng, (nb, Tbuf, C), special=variant == "special", offset=1e6 if variant == "offset" else 0.0)
            x = _to_torch(torch, xh, C)[:, :T]
            want = _segments_ref(xh[:, :T], v, nfft, hop, True)
            got = bhw.welch_frames(p, x, L, hop, nfft=nfft)
            assert _same(_from_torch(torch, got, C), want), (case, variant)
            assert _same(_from_torch(torch, tab.welch_frames(p, x, L, hop, nfft=nfft), C), want), (case, variant, "table")
            # one signal of the batch alone: another plan, the same rows, the same bits
            one = bhw.welch_frames(p, x[nb // 2], L, hop, nfft=nfft)
            assert one.dim() == 2 and _same(_from_torch(torch, one, C), want[nb // 2]), (case, variant, "1-D")
        # a NaN poisons the rows (and the channel) that hold it and no other
        xh = _signal(rng, (nb, T, C), special=False)
        t0 = T // 2
        xh[0, t0, C - 1] = np.nan
        got = _from_torch(torch, bhw.welch_frames(p, _to_torch(torch, xh, C), L, hop, nfft=nfft), C)
        F = got.shape[1]
        holds = np.array([f * hop <= t0 < f * hop + L for f in range(F)])
        nan_rows = np.isnan(got).any(axis=2)                        # (B, F, C)
        want_rows = np.zeros_like(nan_rows)
        want_rows[0, :, C - 1] = holds
        assert np.array_equal(nan_rows, want_rows), case
        assert np.isnan(got[0, holds, :L, C - 1]).all(), case
    # a caller's workspace and output; the workspace too small
    x = _to_torch(torch, _signal(rng, (nb, T, C), special=False), C)
    F = 1 + (T - L) // hop
    ws = torch.empty(nb * F * C, dtype=torch.float32, device="cuda")
    out = torch.empty((nb, F, nfft), dtype=x.dtype, device="cuda")
    assert bhw.welch_frames(p, x, L, hop, nfft=nfft, out=out, workspace=ws) is out
    assert torch.equal(torch.view_as_real(out) if C == 2 else out,
                       torch.view_as_real(bhw.welch_frames(p, x, L, hop, nfft=nfft)) if C == 2 else bhw.welch_frames(p, x, L, hop, nfft=nfft))
    if nb * F * C > 1:
        with pytest.raises(ValueError, match="workspace"):
            bhw.welch_frames(p, x, L, hop, nfft=nfft, workspace=ws[:-1])


def test_mean_does_not_depend_on_the_plan(torch):
    """The same rows inside a B = 1 and a B = 64 call, from the library and from a table: the same bits."""
    p = _params(4)
    rng = np.random.default_rng(7)
    L, nfft, hop, T = 400, 512, 160, 16000
    xh = _signal(rng, (64, T, 1), special=False, offset=3e5)
    x = _to_torch(torch, xh, 1)
    with bhw.ResidentTable(p) as tab:
        y64 = bhw.welch_frames(p, x, L, hop, nfft=nfft)
        t64 = tab.welch_frames(p, x, L, hop, nfft=nfft)
        assert torch.equal(y64, t64)
        for b in (0, 17, 63):
            assert torch.equal(bhw.welch_frames(p, x[b:b + 1], L, hop, nfft=nfft)[0], y64[b])
            assert torch.equal(tab.welch_frames(p, x[b], L, hop, nfft=nfft), y64[b])
    assert _same(y64.cpu().numpy()[..., None], _segments_ref(xh, _v(p, L), nfft, hop, True))


# ---- averaged periodogram ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7])
@pytest.mark.parametrize("K", [1, 33, 257, 513])
def test_psd_equals_its_restatement(torch, F, K):
    rng = np.random.default_rng(F * 1000 + K)
    nb = 2
    # (nfft, onesided): even and odd nfft one-sided, and two-sided
    for nfft, onesided in ((2 * (K - 1) if K > 1 else 1, True), (2 * (K - 1) + 1, True), (K, False)):
        for strided in (False, True):
            Yh = (rng.standard_normal((nb, F, K + 3)) + 1j * rng.standard_normal((nb, F, K + 3))).astype(np.complex64) * np.float32(1e3)
            if strided and F * K > 4:                               # inf / NaN bins, huge and tiny magnitudes
                flat = Yh.reshape(-1).view(np.float32)
                idx = rng.choice(flat.size, size=8, replace=False)
                flat[idx] = np.array([np.inf, -np.inf, np.nan, 3e38, 1e-40, -0.0, 2e19, -2e19], dtype=np.float32)
            scale = 1.0 / (3.7 * F)
            Yd = torch.from_numpy(Yh).cuda()
            Y = Yd[..., :K] if strided else Yd[..., :K].contiguous()
            want = _psd_ref(Yh[..., :K], scale, nfft, onesided)
            got = bhw.welch_psd(Y, scale, nfft=nfft, onesided=onesided)
            assert got.shape == (nb, K) and _same(got.cpu().numpy(), want), (F, K, nfft, onesided, strided)
            one = bhw.welch_psd(Y[1], scale, nfft=nfft, onesided=onesided)
            assert one.shape == (K,) and _same(one.cpu().numpy(), want[1]), (F, K, nfft, "2-D")
            # a strided output: the gaps stay as they were
            big = torch.full((nb, K + 5), -3.0, device="cuda")
            assert bhw.welch_psd(Y, scale, nfft=nfft, onesided=onesided, out=big[:, :K]).data_ptr() == big.data_ptr()
            assert _same(big[:, :K].cpu().numpy(), want) and bool((big[:, K:] == -3.0).all()), (F, K, nfft, "gaps")


# ---- the chain -----------------------------------------------------------------------------------------------------------------------

def test_graph_capture_of_welch_from_a_table(torch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    L, nfft, T, nb = 400, 512, 48000, 4                              # 299 segments: two frame blocks
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((nb, T), device="cuda", generator=g) + 5.0
    with bhw.ResidentTable(p) as tab:
        tab.welch(p, x, 16000.0, length=L, noverlap=240, nfft=nfft)                        # the warm call reads the window sums
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                f, P = tab.welch(p, x, 16000.0, length=L, noverlap=240, nfft=nfft)
        torch.cuda.current_stream().wait_stream(s)
        x.copy_(torch.randn((nb, T), device="cuda", generator=g) * 3.0 - 2.0)                # new data in the captured input
        P.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        fe, Pe = tab.welch(p, x, 16000.0, length=L, noverlap=240, nfft=nfft)
        fl, Pl = bhw.welch(p, x, 16000.0, length=L, noverlap=240, nfft=nfft)
        assert torch.equal(P, Pe) and torch.equal(f, fe) and torch.equal(Pl, Pe) and bool((P > 0).all())


def test_welch_under_capture_needs_the_sums_read_first(torch, monkeypatch):
    """Before the sums of a (params, length, shift) have been read, a capturing stream gets an error instead of a synchronisation."""
    p = B.make_params(B.WIN_BH7, 12, 32)
    x = torch.zeros((2, 4000), device="cuda")
    with bhw.ResidentTable(p) as tab:
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="window sums"):
            tab.welch(p, x, length=399)
        monkeypatch.undo()
        tab.welch(p, x, length=399)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        tab.welch(p, x, length=399)                                 # cached: no read, no error
        monkeypatch.undo()
    torch.cuda.synchronize()


def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    x = torch.zeros((2, 1000), device="cuda")
    with pytest.raises(ValueError, match="detrend"):
        bhw.welch(p, x, length=64, detrend="linear")
    with pytest.raises(ValueError, match="detrend"):
        bhw.welch_frames(p, x, 64, 32, detrend="linear")
    with pytest.raises(ValueError, match="average"):
        bhw.welch(p, x, length=64, average="median")
    with pytest.raises(ValueError, match="scaling"):
        bhw.welch(p, x, length=64, scaling="power")
    with pytest.raises(ValueError, match="noverlap"):
        bhw.welch(p, x, length=64, noverlap=64)
    with pytest.raises(ValueError, match="nfft"):
        bhw.welch(p, x, length=64, nfft=63)
    with pytest.raises(ValueError, match="length"):
        bhw.welch(p, x, length=2048)                                # above 2^phi_width
    with pytest.raises(ValueError, match="zero segments"):
        bhw.welch(p, x[:, :50], length=64)
    with pytest.raises(ValueError, match=r"\(T,\) or \(B, T\)"):
        bhw.welch(p, x.reshape(2, 10, 100), length=64)
    with pytest.raises(ValueError, match="float32 or complex64"):
        bhw.welch(p, x.double(), length=64)
    with pytest.raises(ValueError, match="CUDA"):
        bhw.welch(p, x.cpu(), length=64)
    Y = torch.zeros((2, 5, 33), dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError, match="complex64"):
        bhw.welch_psd(Y.real.contiguous(), 1.0, nfft=64)
    with pytest.raises(ValueError, match="bins"):
        bhw.welch_psd(Y, 1.0, nfft=100)
    with pytest.raises(ValueError, match=r"\(frames, bins\)"):
        bhw.welch_psd(Y[0, 0], 1.0, nfft=64)
    with pytest.raises(ValueError, match="out must be"):
        bhw.welch_psd(Y, 1.0, nfft=64, out=torch.zeros((2, 32), device="cuda"))
    with pytest.raises(B.BhwError, match="not finite"):
        bhw.welch_psd(Y, float("inf"), nfft=64)
    with pytest.raises(ValueError, match="shift"):
        bhw.window_sums(p, 64, shift=63)
    taylor = B.make_params(B.WIN_HANN, 10, 16, sin_type=B.SIN_TAYLOR)
    with pytest.raises(B.BhwError):
        bhw.window_sums(taylor, 64)


# ---- end to end against the model ----------------------------------------------------------------------------------------------------

def _welch_ref64(x, v, fs, L, noverlap, nfft, detrend, scaling="density"):
    """scipy.signal.welch(x, fs, window=v, noverlap=noverlap, nfft=nfft, detrend=detrend, scaling=scaling) restated in NumPy float64."""
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
    """White noise, two tones 120 dB apart and a DC offset."""
    rng = np.random.default_rng(seed)
    n = np.arange(T, dtype=np.float64)
    x = np.cos(2 * np.pi * 0.1234 * n) + 1e-6 * np.cos(2 * np.pi * 0.31 * n + 1.0) + 1e-4 * rng.standard_normal(T) + 0.5
    return x.astype(np.float32)


def _rel_err(P, ref):
    return float(np.abs(np.asarray(P, dtype=np.float64) - ref).max() / ref.max())


def test_numpy_restatement_matches_scipy(torch):
    signal = pytest.importorskip("scipy.signal")
    p = B.make_params(B.WIN_BH7, 16, 32)
    x = _test_signal(50000, 3).astype(np.float64)
    for L, nov, nfft in ((4096, 2048, 4096), (400, 240, 512), (401, 100, 513)):
        v = _v(p, L).astype(np.float64)
        for detrend in ("constant", False):
            for scaling in ("density", "spectrum"):
                f0, P0 = signal.welch(x, 2.0, window=v, noverlap=nov, nfft=nfft, detrend=detrend, scaling=scaling)
                f1, P1 = _welch_ref64(x, v, 2.0, L, nov, nfft, bool(detrend), scaling)
                assert np.allclose(f0, f1, rtol=0, atol=1e-15)
                assert np.abs(P0 - P1).max() <= 1e-12 * P0.max(), (L, detrend, scaling)


@pytest.mark.parametrize("L,noverlap,nfft", [(4096, 2048, 4096), (400, 240, 512)])
def test_welch_end_to_end_within_twice_the_torch_route(torch, L, noverlap, nfft):
    """BH-7 at 32 bits on white noise + two tones 120 dB apart + a DC offset, T = 200 000.  The reference is the float64 restatement of
    scipy.signal.welch with the window given as the array v; the yardstick is the error of the torch-only float32 route against it on
    the same GPU, max |dPxx| / max Pxx.  bhw.welch must stay within 2x the yardstick: both routes share the float32 FFT's error,
    which dominates, and differ only in where they round around it.  Measured on an MI355X: see DESIGN.md section 15."""
    p = B.make_params(B.WIN_BH7, 16, 32)
    xh = _test_signal(200000, 5)
    x = torch.from_numpy(xh).cuda()
    vh = _v(p, L)
    fr, ref = _welch_ref64(xh, vh, 1.0, L, noverlap, nfft, True)
    f, P = bhw.welch(p, x, 1.0, length=L, noverlap=noverlap, nfft=nfft)
    with bhw.ResidentTable(p) as tab:
        ft, Pt = tab.welch(p, x, 1.0, length=L, noverlap=noverlap, nfft=nfft)
    assert torch.equal(P, Pt) and torch.equal(f, ft)
    assert f.dtype == torch.float64 and np.allclose(f.cpu().numpy(), fr, rtol=0, atol=1e-15)
    yard = _rel_err(_torch_route(torch, x, torch.from_numpy(vh).cuda(), 1.0, L, noverlap, nfft).cpu().numpy(), ref)
    err = _rel_err(P.cpu().numpy(), ref)
    print(f"welch end to end L={L} nfft={nfft} hop={L - noverlap}: bhw.welch {err:.3e}, torch-only route {yard:.3e}, ratio {err / yard:.3f}")
    assert err <= 2.0 * yard, (err, yard)
    # what detrending is for: with the offset left in, the window's main lobe carries it into the low bins
    _, Pn = bhw.welch(p, x, 1.0, length=L, noverlap=noverlap, nfft=nfft, detrend=False)
    low = slice(1, 4)
    ratio = float((Pn.cpu().numpy()[low] / ref[low]).min())
    print(f"  bins 1..3 without detrending: at least {ratio:.3e} times the detrended reference")
    assert ratio > 1e3
    assert float(np.abs(P.cpu().numpy()[low] - ref[low]).max() / ref.max()) <= 2.0 * yard
    # the spectrum scaling and a batch of two
    _, refs = _welch_ref64(xh, vh, 1.0, L, noverlap, nfft, True, "spectrum")
    _, Ps = bhw.welch(p, torch.stack([x, x]), 1.0, length=L, noverlap=noverlap, nfft=nfft, scaling="spectrum")
    assert Ps.shape == (2, nfft // 2 + 1) and torch.equal(Ps[0], Ps[1]) and _rel_err(Ps[0].cpu().numpy(), refs) <= 2.0 * yard


def test_welch_two_sided_complex(torch):
    """complex64 input: the two-sided spectrum over fft's bins, return_onesided ignored as scipy does."""
    p = B.make_params(B.WIN_BH4, 14, 24)
    rng = np.random.default_rng(21)
    T, L, nov, nfft = 20000, 300, 100, 512
    xh = (rng.standard_normal(T) + 1j * rng.standard_normal(T) + (0.3 - 0.2j)).astype(np.complex64)
    v = _v(p, L).astype(np.float64)
    hop = L - nov
    F = (T - nov) // hop
    seg = xh.astype(np.complex128)[np.arange(F)[:, None] * hop + np.arange(L)[None, :]]
    seg = seg - seg.mean(axis=-1, keepdims=True)
    Yr = np.fft.fft(seg * v, n=nfft, axis=-1)
    ref = (np.abs(Yr) ** 2).mean(axis=0) / (4.0 * (v * v).sum())
    f, P = bhw.welch(p, torch.from_numpy(xh).cuda(), 4.0, length=L, noverlap=nov, nfft=nfft, return_onesided=True)
    assert P.shape == (nfft,) and np.allclose(f.cpu().numpy(), np.fft.fftfreq(nfft, 0.25), rtol=0, atol=1e-12)
    # a float32 FFT of 512 points against float64: 2^-24 per rounding, log2(512) = 9 butterfly stages, the square doubling it -- some
    # 1e-6 of the peak; 1e-5 says "the same spectrum", it is no contract
    assert _rel_err(P.cpu().numpy(), ref) < 1e-5
