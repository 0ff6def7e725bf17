"""The fused Welch PSD for I/Q input on the GPU (bhw_welch_cfft_f32_* through bhw.welch_fft_iq, bhw.welch_fused_iq and their
ResidentTable forms).

The gate is exact.  include/bhw.h defines P on the float32 pairs bhw_stft_cfft_f32_* writes: q = re^2 + im^2 in binary64, summed over
the frames in chunks of 16, the chunks of a block of 256 frames in order, then the blocks in order, times scale, rounded once.  For
every case of tests/welch_cfft_cases.py, library and table, shifted and not, P must equal that restated in torch float64 on
bhw.stft_iq of the same call, word for word: every step of the restatement is an IEEE elementwise operation, so there is no tolerance.
Around it: the agreement with welch_psd(stft_iq(...), onesided=False) (bit for bit up to 16 frames, one float32 ulp in every case),
the shifted result as fftshift of the unshifted one, independence of the batch and the form, untouched gaps, zeros, NaN containment,
graph capture, the end-to-end accuracy bound against scipy.signal.welch in complex128, and the Python errors."""
import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import welch_cfft_cases as WC

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
    g = torch.Generator(device="cuda").manual_seed(2000 + seed)
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
    x = _signal(torch, c["B"], WC.frames_to_samples(c), seed)
    return x[0] if c["B"] == 1 and seed % 2 else x                   # a 1-D x now and then


# ---- the gate ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", WC.case_ids())
def test_word_for_word_equal_to_the_contract_on_stft_iq_rows(torch, cid):
    c = WC.case(cid)
    p = WC.params(c["setup"])
    _, _, F, _ = WC.desc(c)
    x = _case_x(torch, c, seed=WC.case_ids().index(cid))
    n = c["n_fft"]
    scale = 1.0 / (3.7 * F)
    Y = bhw.stft_iq(p, x, n, c["hop"], **_kw(c))                       # the rows the contract is stated on, bins in order
    assert Y.shape[-2:] == (F, n)
    want = _restate(torch, Y, scale)
    two = bhw.welch_psd(Y, scale, nfft=n, onesided=False)             # the route this call replaces
    two = two if two.dim() == 2 else two.unsqueeze(0)
    ulps = _ulps(want, two)
    print(f"{cid}: F = {F}, the contract against welch_psd(stft_iq(...), onesided=False): {ulps} ulp")
    assert ulps <= 1, (cid, ulps)
    if F <= CHUNK:
        assert _same_bits(want, two), cid                              # the plain ascending sum: bit for bit
    with bhw.ResidentTable(p) as tab:
        for shifted in (False, True):
            w = torch.fft.fftshift(want, dim=-1) if shifted else want  # a permutation of the columns: the same words
            w = w[0] if x.dim() == 1 else w
            d = WC.parse(WC.line(c, table=tab._live(), fftshift=shifted))
            assert d["table"] and d["frames"] == F and d["shifted"] == shifted
            if c.get("padded"):
                buf = torch.full((c["B"], n + 5), SENTINEL, device="cuda")
                out = buf[:, :n] if x.dim() == 2 else buf[0, :n]
                got = bhw.welch_fft_iq(p, x, n, c["hop"], scale, fftshift=shifted, out=out, **_kw(c))
                assert got.data_ptr() == buf.data_ptr() and bool((buf[:, n:] == SENTINEL).all()), "a gap was written"
            else:
                got = bhw.welch_fft_iq(p, x, n, c["hop"], scale, fftshift=shifted, **_kw(c))
            assert got.dtype == torch.float32 and got.shape == w.shape
            assert _same_bits(got, w), (cid, "library", shifted, _ulps(got, w))
            tb = tab.welch_fft_iq(p, x, n, c["hop"], scale, fftshift=shifted, **_kw(c))
            assert _same_bits(tb, w), (cid, "table", shifted, _ulps(tb, w))
            # within one float32 ulp of the two-call route in every case, and the same bits up to 16 frames
            t2 = torch.fft.fftshift(two, dim=-1) if shifted else two
            t2 = t2[0] if x.dim() == 1 else t2
            assert _ulps(got, t2) <= 1 and (F > CHUNK or _same_bits(got, t2)), cid


@pytest.mark.parametrize("cid", WC.SHIFTED)
def test_the_shifted_result_is_fftshift_of_the_unshifted_one(torch, cid):
    c = WC.case(cid)
    p = WC.params(c["setup"])
    x = _case_x(torch, c, seed=30)
    plain = bhw.welch_fft_iq(p, x, c["n_fft"], c["hop"], 0.125, **_kw(c))
    turned = bhw.welch_fft_iq(p, x, c["n_fft"], c["hop"], 0.125, fftshift=True, **_kw(c))
    assert _same_bits(turned, torch.fft.fftshift(plain, dim=-1)), cid
    # and it is what averaging the shifted rows gives
    Ys = bhw.stft_iq(p, x, c["n_fft"], c["hop"], fftshift=True, **_kw(c))
    w = _restate(torch, Ys, 0.125)
    assert _same_bits(turned, w[0] if x.dim() == 1 else w), cid


# ---- determinism, gaps, zeros, specials --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_fft,L,hop,F", [(64, 50, 16, 40), (512, 400, 160, 40), (2048, 2048, 512, 20)])
def test_a_signal_alone_and_as_number_37_of_64_give_the_same_bits(torch, n_fft, L, hop, F):
    p = WC.params(0)
    x = _signal(torch, 64, (F - 1) * hop + n_fft, n_fft)
    kw = dict(win_length=L, detrend=False)
    P64 = bhw.welch_fft_iq(p, x, n_fft, hop, 0.01, **kw)
    one = bhw.welch_fft_iq(p, x[37], n_fft, hop, 0.01, **kw)
    assert one.shape == (n_fft,) and _same_bits(one, P64[37])
    assert _same_bits(bhw.welch_fft_iq(p, x[37:38], n_fft, hop, 0.01, **kw)[0], P64[37])
    with bhw.ResidentTable(p) as tab:
        assert _same_bits(tab.welch_fft_iq(p, x, n_fft, hop, 0.01, **kw), P64)
        assert _same_bits(tab.welch_fft_iq(p, x[37], n_fft, hop, 0.01, **kw), P64[37])


def test_sentinels_in_the_gaps_of_a_padded_out_and_behind_the_workspace_are_untouched(torch):
    for cid in ("n64-3x17", "n512-l400-3x259"):                        # one join launch; two, with block sums behind the chunk sums
        c = WC.case(cid)
        p = WC.params(c["setup"])
        x = _case_x(torch, c)
        n, nb = c["n_fft"], c["B"]
        buf = torch.full((nb, n + 7), SENTINEL, device="cuda")
        need = B.welch_cfft_workspace_bytes(WC.desc(c)[0]) // 8
        assert need == WC.workspace_doubles(nb, c["F"], n)
        ws = torch.full((need + 3,), SENTINEL, dtype=torch.float64, device="cuda")
        got = bhw.welch_fft_iq(p, x, n, c["hop"], 0.5, fftshift=True, out=buf[:, :n], workspace=ws[:need], **_kw(c))
        assert got.data_ptr() == buf.data_ptr() and _same_bits(got, bhw.welch_fft_iq(p, x, n, c["hop"], 0.5, fftshift=True, **_kw(c)))
        assert bool((buf[:, n:] == SENTINEL).all()) and bool((ws[need:] == SENTINEL).all()), "a gap or the workspace's end was written"
        assert not bool((ws[:need] == SENTINEL).any()), "a chunk or block sum was not written"
        with pytest.raises(ValueError, match="workspace"):
            bhw.welch_fft_iq(p, x, n, c["hop"], 0.5, workspace=ws[:need - 1], **_kw(c))


@pytest.mark.parametrize("cid", ["n16-2x70", "n256-l200-detrend-2x40", "n512-l400-3x259", "n2048-detrend-1x35"])
def test_zeros_in_give_positive_zero_out(torch, cid):
    c = WC.case(cid)
    p = WC.params(c["setup"])
    x = torch.zeros((c["B"], WC.frames_to_samples(c)), dtype=torch.complex64, device="cuda")
    for shifted in (False, True):
        P = bhw.welch_fft_iq(p, x, c["n_fft"], c["hop"], 0.25, fftshift=shifted, **_kw(c))
        assert bool((_bits(P) == 0).all()), cid                       # +0.0: not -0.0, not a denormal


@pytest.mark.parametrize("cid", ["n64-3x17", "n512-l400-3x259", "n128-l100-detrend-2x33"])
def test_one_nan_poisons_exactly_the_row_of_its_own_signal(torch, cid):
    c = WC.case(cid)
    p = WC.params(c["setup"])
    x = _case_x(torch, c)
    clean = bhw.welch_fft_iq(p, x, c["n_fft"], c["hop"], 0.5, **_kw(c))
    assert bool(torch.isfinite(clean).all())
    bad = c["B"] - 1
    x[bad, x.shape[1] // 2] = complex(float("nan"), 0.0)              # one part of one sample
    P = bhw.welch_fft_iq(p, x, c["n_fft"], c["hop"], 0.5, **_kw(c))
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


def test_welch_fft_iq_is_captured_with_no_warm_call(torch):
    p = B.make_params(B.WIN_BH4, 13, 24)                               # a configuration no other test of this file has used
    n_fft, L, hop, nb, F = 512, 400, 160, 4, 299                      # two blocks: the kernel and both joins are in the graph
    T = (F - 1) * hop + n_fft
    x = _signal(torch, nb, T, 7)
    out = torch.full((nb, n_fft), -1.0, device="cuda")
    s = B.make_stft(nb, T, F, hop, n_fft, channels=2)
    ws = torch.empty(B.welch_cfft_workspace_bytes(s) // 8, dtype=torch.float64, device="cuda")
    kw = dict(win_length=L, out=out, workspace=ws)
    graph, P = _capture(torch, lambda: bhw.welch_fft_iq(p, x, n_fft, hop, 1e-3, **kw))
    assert P.data_ptr() == out.data_ptr()
    x.copy_(_signal(torch, nb, T, 8) * 3.0 - 2.0)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(out.clone(), bhw.welch_fft_iq(p, x, n_fft, hop, 1e-3, win_length=L)) and bool((out > 0).all())
    with bhw.ResidentTable(p) as tab:                                  # the from-table form on its first call
        out.fill_(-1.0)
        graph, P = _capture(torch, lambda: tab.welch_fft_iq(p, x, n_fft, hop, 1e-3, **kw))
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(out.clone(), bhw.welch_fft_iq(p, x, n_fft, hop, 1e-3, win_length=L))


def test_table_welch_fused_iq_is_captured_after_one_warm_call_and_replayed_on_new_data(torch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    L, nfft, T, nb = 400, 512, 48000, 4                                # 299 segments
    x = _signal(torch, nb, T, 11)
    kw = dict(length=L, noverlap=240, nfft=nfft, fftshift=True)
    with bhw.ResidentTable(p) as tab:
        f0, P0 = tab.welch_fused_iq(p, x, 16000.0, **kw)               # the warm call reads the window sums and builds the axis
        out = torch.empty_like(P0)
        ws = torch.empty(B.welch_cfft_workspace_bytes(B.make_stft(nb, T, 299, 160, nfft, channels=2)) // 8, dtype=torch.float64, device="cuda")
        graph, (f, P) = _capture(torch, lambda: tab.welch_fused_iq(p, x, 16000.0, out=out, workspace=ws, **kw))
        assert P.data_ptr() == out.data_ptr() and f is f0
        x.copy_(_signal(torch, nb, T, 12) * 3.0 - 2.0)
        P.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        fe, Pe = tab.welch_fused_iq(p, x, 16000.0, **kw)
        fl, Pl = bhw.welch_fused_iq(p, x, 16000.0, **kw)
        assert _same_bits(P, Pe) and torch.equal(f, fe) and _same_bits(Pl, Pe) and torch.equal(fl, fe) and bool((P > 0).all())
        # against welch() of the same complex x (welch_frames + torch.fft + welch_psd): two float32 FFTs apart, so loosely
        fw, Pw = tab.welch(p, x, 16000.0, length=L, noverlap=240, nfft=nfft)
        assert torch.equal(torch.fft.fftshift(fw), fe)
        assert float((torch.fft.fftshift(Pw, dim=-1) - Pe).abs().max() / Pe.max()) < 1e-5


def test_welch_fused_iq_under_capture_needs_the_sums_and_the_axis_first(torch, monkeypatch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    x = torch.zeros((2, 4000), dtype=torch.complex64, device="cuda")
    xr = torch.zeros((2, 4000), device="cuda")
    with bhw.ResidentTable(p) as tab:
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="window sums"):
            tab.welch_fused_iq(p, x, length=397, nfft=512)
        monkeypatch.undo()
        f1, _ = tab.welch_fused_iq(p, x, length=397, nfft=512)
        fr, _ = tab.welch_fused(p, xr, length=397, nfft=512)           # the one-sided axis of the same (nfft, fs): another key
        assert fr.shape == (257,) and f1.shape == (512,) and torch.equal(f1, torch.fft.fftfreq(512, d=1.0, dtype=torch.float64, device="cuda"))
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        assert tab.welch_fused_iq(p, x, length=397, nfft=512)[0] is f1 and tab.welch_fused(p, xr, length=397, nfft=512)[0] is fr
        # the shifted axis and a second fs have not been built, and are never built inside a capture
        with pytest.raises(RuntimeError, match="frequency axis"):
            tab.welch_fused_iq(p, x, length=397, nfft=512, fftshift=True)
        with pytest.raises(RuntimeError, match="frequency axis"):
            tab.welch_fused_iq(p, x, 8000.0, length=397, nfft=512)
        monkeypatch.undo()
        f2, _ = tab.welch_fused_iq(p, x, 8000.0, length=397, nfft=512, fftshift=True)
        assert torch.equal(f2, torch.fft.fftshift(torch.fft.fftfreq(512, d=1.0 / 8000.0, dtype=torch.float64, device="cuda")))
        # a bounded number of two-sided axes, counted apart from welch_fused's
        for i in range(12):
            tab.welch_fused_iq(p, x, 100.0 + i, length=397, nfft=512)
        assert sum(1 for k in tab._sums if k[0] == "freqs_iq") <= 8 and sum(1 for k in tab._sums if k[0] == "freqs") == 1
        assert tab.welch_fused(p, xr, length=397, nfft=512)[0] is fr
    torch.cuda.synchronize()


# ---- end to end against the model --------------------------------------------------------------------------------------------------------

def _rel_err(P, ref):
    return float(np.max(np.abs(P.astype(np.float64) - ref)) / np.max(ref))


@pytest.mark.parametrize("L,noverlap,nfft,T", [(400, 240, 512, 160000), (2048, 1024, 2048, 200000)])
def test_end_to_end_within_twice_the_torch_route_against_scipy(torch, L, noverlap, nfft, T):
    """Three signals of tones in noise against scipy.signal.welch evaluated on the CPU in complex128 with the float32 window
    coefficients.  The yardstick is the error of the torch-only float32 route (welch(fft="torch") on the same complex x) against the
    same scipy result, max |dPxx| / max Pxx, and the bound twice the yardstick: the project's standing bound
    (tests/test_gpu_welch.py)."""
    from scipy import signal
    p = B.make_params(B.WIN_BH7, 16, 32)
    fs = 48000.0
    x = _signal(torch, 3, T, 5)
    xh = x.cpu().numpy().astype(np.complex128)
    vh = _v(p, L).astype(np.float64)
    fr, ref = signal.welch(xh, fs, window=vh, nperseg=L, noverlap=noverlap, nfft=nfft, detrend="constant", return_onesided=False, axis=-1)
    f, P = bhw.welch_fused_iq(p, x, fs, length=L, noverlap=noverlap, nfft=nfft)
    with bhw.ResidentTable(p) as tab:
        ft, Pt = tab.welch_fused_iq(p, x, fs, length=L, noverlap=noverlap, nfft=nfft)
    assert _same_bits(P, Pt) and torch.equal(f, ft)
    assert f.dtype == torch.float64 and P.shape == (3, nfft) and np.allclose(f.cpu().numpy(), fr, rtol=0, atol=1e-9)
    fy, Py = bhw.welch(p, x, fs, length=L, noverlap=noverlap, nfft=nfft, fft="torch")
    assert torch.equal(fy, f)
    yard = _rel_err(Py.cpu().numpy(), ref)
    err = _rel_err(P.cpu().numpy(), ref)
    print(f"welch_fused_iq end to end L={L} nfft={nfft} hop={L - noverlap}: welch_fused_iq {err:.3e}, torch-only route {yard:.3e}, "
          f"ratio {err / yard:.3f}")
    assert err <= 2.0 * yard, (err, yard)
    fs_, Ps = bhw.welch_fused_iq(p, x, fs, length=L, noverlap=noverlap, nfft=nfft, fftshift=True)
    assert _same_bits(Ps, torch.fft.fftshift(P, dim=-1)) and np.allclose(fs_.cpu().numpy(), np.fft.fftshift(fr), rtol=0, atol=1e-9)


# ---- Python errors -----------------------------------------------------------------------------------------------------------------------

def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    x = torch.zeros((2, 1000), dtype=torch.complex64, device="cuda")
    xr = torch.zeros((2, 1000), device="cuda")
    for bad in (xr, x.to(torch.complex128)):
        with pytest.raises(ValueError, match="complex64"):
            bhw.welch_fft_iq(p, bad, 64, 16, 1.0)
        with pytest.raises(ValueError, match="complex64"):
            bhw.welch_fused_iq(p, bad, length=64)
    for n in (48, 8, 4096):
        with pytest.raises(ValueError, match="power of two in 16..2048"):
            bhw.welch_fft_iq(p, x, n, 16, 1.0, win_length=8)
    with pytest.raises(ValueError, match="power of two in 16..2048"):
        bhw.welch_fused_iq(p, x, length=60)
    with pytest.raises(ValueError, match="power of two in 16..2048"):
        bhw.welch_fused_iq(p, x, length=60, nfft=100)
    with pytest.raises(TypeError):
        bhw.welch_fused_iq(p, x, length=64, average="median")
    # the names that exist keep refusing, or routing, complex input as before
    with pytest.raises(ValueError, match="real float32"):
        bhw.welch_fft(p, x, 64, 16, 1.0)
    with pytest.raises(ValueError, match="real float32"):
        bhw.welch_fused(p, x, length=64)
    with pytest.raises(ValueError, match="real float32"):
        bhw.welch(p, x, length=64, fft="fused")
    assert bhw.welch(p, x, length=64)[1].shape == (2, 64)
    with pytest.raises(ValueError, match="'torch' or 'fused'"):
        bhw.welch(p, x, length=64, fft="iq")
    with pytest.raises(ValueError, match="detrend"):
        bhw.welch_fused_iq(p, x, length=64, detrend="linear")
    with pytest.raises(ValueError, match="scaling"):
        bhw.welch_fused_iq(p, x, length=64, scaling="power")
    with pytest.raises(ValueError, match="noverlap"):
        bhw.welch_fused_iq(p, x, length=64, noverlap=64)
    with pytest.raises(ValueError, match="nfft"):
        bhw.welch_fused_iq(p, x, length=64, nfft=32)
    with pytest.raises(ValueError, match="zero segments"):
        bhw.welch_fused_iq(p, x[:, :50], length=64)
    with pytest.raises(ValueError, match="zero frames"):
        bhw.welch_fft_iq(p, x[:, :50], 64, 16, 1.0)
    with pytest.raises(ValueError, match="hop"):
        bhw.welch_fft_iq(p, x, 64, 0, 1.0)
    with pytest.raises(ValueError, match="center=False"):
        bhw.welch_fft_iq(p, x, 64, 16, 1.0, center=True, detrend=True)
    with pytest.raises(ValueError, match="pad_mode"):
        bhw.welch_fft_iq(p, x, 64, 16, 1.0, center=True, pad_mode="edge")
    with pytest.raises(ValueError, match="CUDA"):
        bhw.welch_fft_iq(p, x.cpu(), 64, 16, 1.0)
    with pytest.raises(ValueError, match="CUDA"):
        bhw.welch_fused_iq(p, x.cpu(), length=64)
    with pytest.raises(ValueError, match="out must be"):
        bhw.welch_fft_iq(p, x, 64, 16, 1.0, out=torch.zeros((2, 33), device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        bhw.welch_fft_iq(p, x, 64, 16, 1.0, out=torch.zeros((2, 64), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="workspace"):
        bhw.welch_fft_iq(p, x, 64, 16, 1.0, workspace=torch.zeros(8, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="workspace"):
        bhw.welch_fft_iq(p, x, 64, 16, 1.0, workspace=torch.zeros(100000, dtype=torch.float32, device="cuda"))
    with pytest.raises(B.BhwError, match="not finite"):
        bhw.welch_fft_iq(p, x, 64, 16, float("inf"))
    # a centred, reflect-padded call is fine, and a 1-D x gives a 1-D P
    assert bhw.welch_fft_iq(p, x[0], 64, 16, 1.0, center=True).shape == (64,)
