"""The fused Welch PSD for I/Q input at a mixed-radix n_fft on the GPU (bhw_welch_cmfft_f32_* through bhw.welch_fft_iq_mixed,
bhw.welch_fused_iq_mixed and their ResidentTable forms).

The gate is exact.  include/bhw.h defines P on the float32 pairs bhw_stft_cmfft_f32_* writes: q = re^2 + im^2 in binary64, summed
over the frames in chunks of 16, the chunks of a block of 256 frames in order, then the blocks in order, times scale, rounded once.
For every case of tests/welch_cmfft_cases.py, library and table, shifted and not, P must equal that restated in torch float64 on
bhw.stft_iq_mixed of the same call, word for word: every step of the restatement is an IEEE elementwise operation, so there is no
tolerance.  Around it: the agreement with welch_psd(stft_iq_mixed(...), onesided=False) (bit for bit up to 16 frames, one float32 ulp
in every case), the shifted result as fftshift of the unshifted one (odd n_fft included), independence of the batch and the form,
untouched gaps, zeros, NaN containment, graph capture, the end-to-end accuracy bound against scipy.signal.welch restated in
complex128, and the Python errors."""
import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import welch_cmfft_cases as WM

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
    """(B, T) complex64 on the device: complex noise of 1000, two complex tones 120 dB apart (one at a negative frequency) and an
    offset in both parts."""
    g = torch.Generator(device="cuda").manual_seed(3000 + seed)
    n = torch.arange(T, device="cuda", dtype=torch.float64)
    tones = 1e3 * torch.exp(2j * np.pi * 0.1234 * n) + 1e-3 * torch.exp(-2j * np.pi * 0.31 * n + 1.0j) + (250.0 - 90.0j)
    noise = torch.randn((nb, T, 2), device="cuda", generator=g, dtype=torch.float64) * 1000
    return (torch.view_as_complex(noise) + tones).to(torch.complex64)


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


def _restate(torch, Y, scale):
    """include/bhw.h on the spectrum rows Y (B, F, n_fft) complex64, in torch float64 on the device: three levels of explicit
    elementwise adds -- 16 frames of every chunk in ascending order, 16 chunks of every block in ascending order, the blocks in
    ascending order, each from +0.0 -- then (A * scale).float().  The chunks (blocks) are independent chains, so one add serves all
    of them."""
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
    return (A * float(scale)).float()


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
    x = _signal(torch, c["B"], WM.frames_to_samples(c), seed)
    return x[0] if c["B"] == 1 and seed % 2 else x                   # a 1-D x now and then


# ---- the gate ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", WM.case_ids())
def test_word_for_word_equal_to_the_contract_on_stft_iq_mixed_rows(torch, cid):
    c = WM.case(cid)
    p = WM.params(c["setup"])
    _, _, F, _ = WM.desc(c)
    x = _case_x(torch, c, seed=WM.case_ids().index(cid))
    n = c["n_fft"]
    scale = 1.0 / (3.7 * F)
    Y = bhw.stft_iq_mixed(p, x, n, c["hop"], **_kw(c))                 # the rows the contract is stated on, bins in order
    assert Y.shape[-2:] == (F, n)
    want = _restate(torch, Y, scale)
    two = bhw.welch_psd(Y, scale, nfft=n, onesided=False)             # the route this call replaces
    two = two if two.dim() == 2 else two.unsqueeze(0)
    ulps = _ulps(want, two)
    print(f"{cid}: F = {F}, the contract against welch_psd(stft_iq_mixed(...), onesided=False): {ulps} ulp")
    assert ulps <= 1, (cid, ulps)
    if F <= CHUNK:
        assert _same_bits(want, two), cid                              # the plain ascending sum: bit for bit
    with bhw.ResidentTable(p) as tab:
        for shifted in (False, True):
            w = torch.fft.fftshift(want, dim=-1) if shifted else want  # a permutation of the columns: the same words
            w = w[0] if x.dim() == 1 else w
            d = WM.parse(WM.line(c, table=tab._live(), fftshift=shifted))
            assert d["table"] and d["frames"] == F and d["shifted"] == shifted
            if c.get("padded"):
                buf = torch.full((c["B"], n + 5), SENTINEL, device="cuda")
                out = buf[:, :n] if x.dim() == 2 else buf[0, :n]
                got = bhw.welch_fft_iq_mixed(p, x, n, c["hop"], scale, fftshift=shifted, out=out, **_kw(c))
                assert got.data_ptr() == buf.data_ptr() and bool((buf[:, n:] == SENTINEL).all()), "a gap was written"
            else:
                got = bhw.welch_fft_iq_mixed(p, x, n, c["hop"], scale, fftshift=shifted, **_kw(c))
            assert got.dtype == torch.float32 and got.shape == w.shape
            assert _same_bits(got, w), (cid, "library", shifted, _ulps(got, w))
            tb = tab.welch_fft_iq_mixed(p, x, n, c["hop"], scale, fftshift=shifted, **_kw(c))
            assert _same_bits(tb, w), (cid, "table", shifted, _ulps(tb, w))
            # within one float32 ulp of the two-call route in every case, and the same bits up to 16 frames
            t2 = torch.fft.fftshift(two, dim=-1) if shifted else two
            t2 = t2[0] if x.dim() == 1 else t2
            assert _ulps(got, t2) <= 1 and (F > CHUNK or _same_bits(got, t2)), cid


@pytest.mark.parametrize("cid", WM.SHIFTED)
def test_the_shifted_result_is_fftshift_of_the_unshifted_one(torch, cid):
    c = WM.case(cid)
    p = WM.params(c["setup"])
    x = _case_x(torch, c, seed=30)
    plain = bhw.welch_fft_iq_mixed(p, x, c["n_fft"], c["hop"], 0.125, **_kw(c))
    turned = bhw.welch_fft_iq_mixed(p, x, c["n_fft"], c["hop"], 0.125, fftshift=True, **_kw(c))
    assert _same_bits(turned, torch.fft.fftshift(plain, dim=-1)), cid
    # and it is what averaging the shifted rows gives
    Ys = bhw.stft_iq_mixed(p, x, c["n_fft"], c["hop"], fftshift=True, **_kw(c))
    w = _restate(torch, Ys, 0.125)
    assert _same_bits(turned, w[0] if x.dim() == 1 else w), cid


# ---- determinism, gaps, zeros, specials --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_fft,L,hop,F", [(60, 50, 16, 40), (400, 400, 160, 40), (2025, 2025, 512, 20)])
def test_a_signal_alone_and_as_number_5_of_8_give_the_same_bits(torch, n_fft, L, hop, F):
    p = WM.params(0)
    x = _signal(torch, 8, (F - 1) * hop + n_fft, n_fft)
    kw = dict(win_length=L, detrend=False)
    P8 = bhw.welch_fft_iq_mixed(p, x, n_fft, hop, 0.01, **kw)
    one = bhw.welch_fft_iq_mixed(p, x[5], n_fft, hop, 0.01, **kw)
    assert one.shape == (n_fft,) and _same_bits(one, P8[5])
    assert _same_bits(bhw.welch_fft_iq_mixed(p, x[5:6], n_fft, hop, 0.01, **kw)[0], P8[5])
    with bhw.ResidentTable(p) as tab:
        assert _same_bits(tab.welch_fft_iq_mixed(p, x, n_fft, hop, 0.01, **kw), P8)
        assert _same_bits(tab.welch_fft_iq_mixed(p, x[5], n_fft, hop, 0.01, **kw), P8[5])


def test_sentinels_in_the_gaps_of_a_padded_out_and_behind_the_workspace_are_untouched(torch):
    for cid in ("n60-3x17", "n400-3x259"):                            # one join launch; two, with block sums behind the chunk sums
        c = WM.case(cid)
        p = WM.params(c["setup"])
        x = _case_x(torch, c)
        n, nb = c["n_fft"], c["B"]
        buf = torch.full((nb, n + 7), SENTINEL, device="cuda")
        need = B.welch_cmfft_workspace_bytes(WM.desc(c)[0]) // 8
        assert need == WM.workspace_doubles(nb, c["F"], n)
        ws = torch.full((need + 3,), SENTINEL, dtype=torch.float64, device="cuda")
        got = bhw.welch_fft_iq_mixed(p, x, n, c["hop"], 0.5, fftshift=True, out=buf[:, :n], workspace=ws[:need], **_kw(c))
        assert got.data_ptr() == buf.data_ptr() and _same_bits(got, bhw.welch_fft_iq_mixed(p, x, n, c["hop"], 0.5, fftshift=True, **_kw(c)))
        assert bool((buf[:, n:] == SENTINEL).all()) and bool((ws[need:] == SENTINEL).all()), "a gap or the workspace's end was written"
        assert not bool((ws[:need] == SENTINEL).any()), "a chunk or block sum was not written"
        with pytest.raises(ValueError, match="workspace"):
            bhw.welch_fft_iq_mixed(p, x, n, c["hop"], 0.5, workspace=ws[:need - 1], **_kw(c))


@pytest.mark.parametrize("cid", ["n18-2x70", "n200-l160-detrend-2x40", "n400-3x259", "n2025-detrend-1x35"])
def test_zeros_in_give_positive_zero_out(torch, cid):
    c = WM.case(cid)
    p = WM.params(c["setup"])
    x = torch.zeros((c["B"], WM.frames_to_samples(c)), dtype=torch.complex64, device="cuda")
    for shifted in (False, True):
        P = bhw.welch_fft_iq_mixed(p, x, c["n_fft"], c["hop"], 0.25, fftshift=shifted, **_kw(c))
        assert bool((_bits(P) == 0).all()), cid                       # +0.0: not -0.0, not a denormal


@pytest.mark.parametrize("cid", ["n60-3x17", "n400-3x259", "n75-l60-detrend-2x33"])
def test_one_nan_poisons_exactly_the_row_of_its_own_signal(torch, cid):
    c = WM.case(cid)
    p = WM.params(c["setup"])
    x = _case_x(torch, c)
    clean = bhw.welch_fft_iq_mixed(p, x, c["n_fft"], c["hop"], 0.5, **_kw(c))
    assert bool(torch.isfinite(clean).all())
    bad = c["B"] - 1
    x[bad, x.shape[1] // 2] = complex(float("nan"), 0.0)              # one part of one sample
    P = bhw.welch_fft_iq_mixed(p, x, c["n_fft"], c["hop"], 0.5, **_kw(c))
    assert bool(torch.isnan(P[bad]).all()), cid
    keep = [b for b in range(c["B"]) if b != bad]
    assert _same_bits(P[keep], clean[keep]), cid


# ---- the scipy-shaped call ---------------------------------------------------------------------------------------------------------------

def test_welch_fused_iq_mixed_is_welch_fft_iq_mixed_with_the_scale_of_the_window_sums(torch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    hop, nb, fs = 150, 3, 30720.0
    # a window below nfft (detrended: the segments have it at column 0, as welch_fft_iq_mixed(detrend=True) does) and one that fills it
    for L, nfft, detrends in ((360, 400, ("constant",)), (400, 400, ("constant", False))):
        T = 20 * hop + L + 17                                         # 21 segments and a tail that no segment reaches
        x = _signal(torch, nb, T, 40)
        sums = bhw.window_sums(p, L, f32=True)
        axis = torch.fft.fftfreq(nfft, d=1.0 / fs, dtype=torch.float64, device="cuda")
        for scaling in ("density", "spectrum"):
            for detrend in detrends:
                for shifted in (False, True):
                    kw = dict(length=L, noverlap=L - hop, nfft=nfft, detrend=detrend, scaling=scaling, fftshift=shifted)
                    f, P = bhw.welch_fused_iq_mixed(p, x, fs, **kw)
                    want = bhw.welch_fft_iq_mixed(p, x, nfft, hop, B.welch_scale(sums, 21, fs, scaling), win_length=L,
                                                  detrend=detrend == "constant", fftshift=shifted)
                    assert P.shape == (nb, nfft) and _same_bits(P, want), (L, scaling, detrend, shifted)
                    assert f.dtype == torch.float64 and torch.equal(f, torch.fft.fftshift(axis) if shifted else axis)
                    assert bhw.welch_fused_iq_mixed(p, x, fs, **kw)[0] is f               # the cached axis is shared
    # nfft defaults to the length, noverlap to half of it; a 1-D x gives a 1-D Pxx
    f, P = bhw.welch_fused_iq_mixed(p, x[0], fs, length=360)
    frames = 1 + (x.shape[1] - 360) // 180
    assert P.shape == (360,) and f.shape == (360,)
    assert _same_bits(P, bhw.welch_fft_iq_mixed(p, x[0], 360, 180, B.welch_scale(bhw.window_sums(p, 360, f32=True), frames, fs, "density"),
                                                detrend=True))


def test_the_axes_of_the_two_iq_calls_are_cached_apart(torch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    x = torch.zeros((2, 4000), dtype=torch.complex64, device="cuda")
    with bhw.ResidentTable(p) as tab:
        f1, _ = tab.welch_fused_iq(p, x, length=397, nfft=512)
        fm, _ = tab.welch_fused_iq_mixed(p, x, length=397, nfft=400)
        assert f1.shape == (512,) and fm.shape == (400,)
        assert torch.equal(fm, torch.fft.fftfreq(400, d=1.0, dtype=torch.float64, device="cuda"))
        assert tab.welch_fused_iq_mixed(p, x, length=397, nfft=400)[0] is fm
        # a bounded number of axes of this kind, counted apart: a second (nfft, fs), and a twelfth, evict none of welch_fused_iq's
        f2, _ = tab.welch_fused_iq_mixed(p, x, 8000.0, length=397, nfft=600, fftshift=True)
        assert torch.equal(f2, torch.fft.fftshift(torch.fft.fftfreq(600, d=1.0 / 8000.0, dtype=torch.float64, device="cuda")))
        assert tab.welch_fused_iq(p, x, length=397, nfft=512)[0] is f1
        for i in range(12):
            tab.welch_fused_iq_mixed(p, x, 100.0 + i, length=397, nfft=400)
        assert sum(1 for k in tab._sums if k[0] == "freqs_iq_mixed") <= 8 and sum(1 for k in tab._sums if k[0] == "freqs_iq") == 1
        assert tab.welch_fused_iq(p, x, length=397, nfft=512)[0] is f1
        for i in range(12):
            tab.welch_fused_iq(p, x, 100.0 + i, length=397, nfft=512)
        assert sum(1 for k in tab._sums if k[0] == "freqs_iq_mixed") >= 1
    torch.cuda.synchronize()


# ---- graph capture -----------------------------------------------------------------------------------------------------------------------

def test_table_welch_fused_iq_mixed_is_captured_after_one_warm_call_and_replayed_on_new_data(torch):
    """One stream, one warm call (it reads the window sums and builds the axis), `out` and `workspace` given: the kernel and both join
    launches are in the graph."""
    p = B.make_params(B.WIN_BH7, 12, 32)
    L, nfft, T, nb = 360, 400, 48000, 4                               # 298 segments at hop 160: two blocks
    x = _signal(torch, nb, T, 11)
    kw = dict(length=L, noverlap=200, nfft=nfft, fftshift=True)
    frames = 1 + (T - L) // 160
    assert frames > BLOCK
    with bhw.ResidentTable(p) as tab:
        f0, P0 = tab.welch_fused_iq_mixed(p, x, 16000.0, **kw)
        out = torch.empty_like(P0)
        ws = torch.empty(B.welch_cmfft_workspace_bytes(B.make_stft(nb, T, frames, 160, nfft, channels=2)) // 8, dtype=torch.float64, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                f, P = tab.welch_fused_iq_mixed(p, x, 16000.0, out=out, workspace=ws, **kw)
        torch.cuda.current_stream().wait_stream(s)
        assert P.data_ptr() == out.data_ptr() and f is f0
        x.copy_(_signal(torch, nb, T, 12) * 3.0 - 2.0)
        P.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        fe, Pe = tab.welch_fused_iq_mixed(p, x, 16000.0, **kw)
        fl, Pl = bhw.welch_fused_iq_mixed(p, x, 16000.0, **kw)
        assert _same_bits(P, Pe) and torch.equal(f, fe) and _same_bits(Pl, Pe) and torch.equal(fl, fe) and bool((P > 0).all())


# ---- end to end against the model --------------------------------------------------------------------------------------------------------

def _rel_err(P, ref):
    return float(np.max(np.abs(P.astype(np.float64) - ref)) / np.max(ref))


def _scipy_welch_restated(xh, vh, fs, L, hop, nfft):
    """scipy.signal.welch(x, fs, window=v, nperseg=L, noverlap=L - hop, nfft=nfft, detrend="constant", return_onesided=False,
    scaling="density") step by step in float64 / complex128: the segments, each less its mean, times the window, the FFT at nfft, and
    the mean of |Y|^2 / (fs * sum v^2)."""
    F = 1 + (xh.shape[-1] - L) // hop
    idx = np.arange(F)[:, None] * hop + np.arange(L)[None, :]
    seg = xh[:, idx]                                                  # (B, F, L)
    seg = (seg - seg.mean(axis=-1, keepdims=True)) * vh
    Y = np.fft.fft(seg, n=nfft, axis=-1)
    return np.fft.fftfreq(nfft, 1.0 / fs), (Y.real ** 2 + Y.imag ** 2).mean(axis=1) / (fs * np.sum(vh * vh))


@pytest.mark.parametrize("L,noverlap,nfft,T", [(1000, 500, 1000, 120000), (1200, 768, 1536, 120000)])
def test_end_to_end_within_twice_the_torch_route_against_scipy(torch, L, noverlap, nfft, T):
    """Three signals of tones in noise against scipy.signal.welch restated in float64 / complex128 with the float32 window
    coefficients (the segments, the detrend, the window, the FFT and the mean, as scipy takes them; checked against scipy itself
    where it is installed).  The yardstick is the error of the torch-only float32 route on the same input (welch_frames ->
    torch.fft.fft -> welch_psd) against the same reference, max |dPxx| / max Pxx, and the bound twice the yardstick: the project's
    standing rule for its FFTs against the library FFT (tests/test_gpu_welch.py).  Measured on an MI355X: see DESIGN.md section 32."""
    p = B.make_params(B.WIN_BH7, 16, 32)
    fs = 23.04e6
    hop = L - noverlap
    x = _signal(torch, 3, T, 5)
    xh = x.cpu().numpy().astype(np.complex128)
    vh = _v(p, L).astype(np.float64)
    fr, ref = _scipy_welch_restated(xh, vh, fs, L, hop, nfft)
    try:
        from scipy import signal
    except ImportError:
        signal = None
    if signal is not None:
        fsp, Psp = signal.welch(xh, fs, window=vh, nperseg=L, noverlap=noverlap, nfft=nfft, detrend="constant", return_onesided=False, axis=-1)
        assert np.allclose(fsp, fr, rtol=0, atol=1e-6) and np.max(np.abs(Psp - ref)) <= 1e-12 * np.max(ref)
    f, P = bhw.welch_fused_iq_mixed(p, x, fs, length=L, noverlap=noverlap, nfft=nfft)
    with bhw.ResidentTable(p) as tab:
        ft, Pt = tab.welch_fused_iq_mixed(p, x, fs, length=L, noverlap=noverlap, nfft=nfft)
    assert _same_bits(P, Pt) and torch.equal(f, ft)
    assert f.dtype == torch.float64 and P.shape == (3, nfft) and np.allclose(f.cpu().numpy(), fr, rtol=0, atol=1e-6)
    # the torch-only float32 route
    F = 1 + (T - L) // hop
    scale = B.welch_scale(bhw.window_sums(p, L, f32=True), F, fs, "density")
    Yt = torch.fft.fft(bhw.welch_frames(p, x, L, hop, nfft=nfft, detrend="constant"))
    Py = bhw.welch_psd(Yt, scale, nfft=nfft, onesided=False)
    yard = _rel_err(Py.cpu().numpy(), ref)
    err = _rel_err(P.cpu().numpy(), ref)
    print(f"welch_fused_iq_mixed end to end L={L} nfft={nfft} hop={hop}: welch_fused_iq_mixed {err:.3e}, torch-only route {yard:.3e}, "
          f"ratio {err / yard:.3f}")
    assert err <= 2.0 * yard, (err, yard)
    fs_, Ps = bhw.welch_fused_iq_mixed(p, x, fs, length=L, noverlap=noverlap, nfft=nfft, fftshift=True)
    assert _same_bits(Ps, torch.fft.fftshift(P, dim=-1)) and np.allclose(fs_.cpu().numpy(), np.fft.fftshift(fr), rtol=0, atol=1e-6)


# ---- Python errors -----------------------------------------------------------------------------------------------------------------------

def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    x = torch.zeros((2, 1000), dtype=torch.complex64, device="cuda")
    xr = torch.zeros((2, 1000), device="cuda")
    # a power of two: the power-of-two I/Q calls take it
    for n in (64, 2048):
        with pytest.raises(ValueError, match=f"n_fft {n} is a power of two: welch_fft_iq / welch_fused_iq transform it"):
            bhw.welch_fft_iq_mixed(p, x, n, 16, 1.0, win_length=8)
    with pytest.raises(ValueError, match="welch_fft_iq / welch_fused_iq"):
        bhw.welch_fused_iq_mixed(p, x, length=64)
    with pytest.raises(ValueError, match="welch_fft_iq / welch_fused_iq"):
        bhw.welch_fused_iq_mixed(p, x, length=60, nfft=128)
    # real input: the real mixed-radix calls take it
    with pytest.raises(ValueError, match="welch_fft_mixed / welch_fused_mixed"):
        bhw.welch_fft_iq_mixed(p, xr, 60, 16, 1.0)
    with pytest.raises(ValueError, match="welch_fft_mixed / welch_fused_mixed"):
        bhw.welch_fused_iq_mixed(p, xr, length=60)
    with pytest.raises(ValueError, match="complex64 input, got torch.complex128"):
        bhw.welch_fft_iq_mixed(p, x.to(torch.complex128), 60, 16, 1.0)
    with pytest.raises(ValueError, match="complex64 input, got torch.complex128"):
        bhw.welch_fused_iq_mixed(p, x.to(torch.complex128), length=60)
    for n in (14, 21, 448):
        with pytest.raises(ValueError, match=rf"2\^a·3\^b·5\^c in 16..2047, got {n}"):
            bhw.welch_fft_iq_mixed(p, x, n, 16, 1.0, win_length=8)
    with pytest.raises(ValueError, match=r"2\^a·3\^b·5\^c in 16..2047, got 70"):
        bhw.welch_fused_iq_mixed(p, x, length=60, nfft=70)
    with pytest.raises(TypeError):
        bhw.welch_fused_iq_mixed(p, x, length=60, average="median")
    with pytest.raises(TypeError):
        bhw.welch_fused_iq_mixed(p, x, length=60, fft="fused")
    # the names that exist keep refusing these sizes in their own words
    with pytest.raises(ValueError, match="power of two in 16..2048"):
        bhw.welch_fft_iq(p, x, 60, 16, 1.0)
    with pytest.raises(ValueError, match="power of two in 16..2048"):
        bhw.welch_fused_iq(p, x, length=60)
    with pytest.raises(ValueError, match="welch_fft_iq / welch_fused_iq"):
        bhw.welch_fft_mixed(p, x, 60, 16, 1.0)
    with pytest.raises(ValueError, match="stft_iq / bhw.spectrogram_iq"):
        bhw.stft_iq_mixed(p, x, 64, 16)
    with pytest.raises(ValueError, match="'torch' or 'fused'"):
        bhw.welch(p, x, length=60, fft="iq_mixed")
    assert bhw.welch(p, x, length=60)[1].shape == (2, 60)
    # the rest of the argument checks are the power-of-two calls'
    with pytest.raises(ValueError, match="detrend"):
        bhw.welch_fused_iq_mixed(p, x, length=60, detrend="linear")
    with pytest.raises(ValueError, match="scaling"):
        bhw.welch_fused_iq_mixed(p, x, length=60, scaling="power")
    with pytest.raises(ValueError, match="noverlap"):
        bhw.welch_fused_iq_mixed(p, x, length=60, noverlap=60)
    with pytest.raises(ValueError, match="nfft"):
        bhw.welch_fused_iq_mixed(p, x, length=60, nfft=48)
    with pytest.raises(ValueError, match="zero segments"):
        bhw.welch_fused_iq_mixed(p, x[:, :50], length=60)
    with pytest.raises(ValueError, match="zero frames"):
        bhw.welch_fft_iq_mixed(p, x[:, :50], 60, 16, 1.0)
    with pytest.raises(ValueError, match="hop"):
        bhw.welch_fft_iq_mixed(p, x, 60, 0, 1.0)
    with pytest.raises(ValueError, match="center=False"):
        bhw.welch_fft_iq_mixed(p, x, 60, 16, 1.0, center=True, detrend=True)
    with pytest.raises(ValueError, match="pad_mode"):
        bhw.welch_fft_iq_mixed(p, x, 60, 16, 1.0, center=True, pad_mode="edge")
    with pytest.raises(ValueError, match="CUDA"):
        bhw.welch_fft_iq_mixed(p, x.cpu(), 60, 16, 1.0)
    with pytest.raises(ValueError, match="CUDA"):
        bhw.welch_fused_iq_mixed(p, x.cpu(), length=60)
    # a bad out or workspace
    with pytest.raises(ValueError, match="out must be"):
        bhw.welch_fft_iq_mixed(p, x, 60, 16, 1.0, out=torch.zeros((2, 31), device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        bhw.welch_fft_iq_mixed(p, x, 60, 16, 1.0, out=torch.zeros((2, 60), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        bhw.welch_fft_iq_mixed(p, x, 60, 16, 1.0, out=torch.zeros((2, 120), device="cuda")[:, ::2])
    with pytest.raises(ValueError, match="workspace"):
        bhw.welch_fft_iq_mixed(p, x, 60, 16, 1.0, workspace=torch.zeros(8, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="workspace"):
        bhw.welch_fft_iq_mixed(p, x, 60, 16, 1.0, workspace=torch.zeros(100000, dtype=torch.float32, device="cuda"))
    with pytest.raises(B.BhwError, match="not finite"):
        bhw.welch_fft_iq_mixed(p, x, 60, 16, float("inf"))
    # a centred, reflect-padded call is fine, and a 1-D x gives a 1-D P
    assert bhw.welch_fft_iq_mixed(p, x[0], 60, 16, 1.0, center=True).shape == (60,)
