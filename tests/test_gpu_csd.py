"""Welch cross spectra on the GPU (bhw_welch_csd_f32, bhw.welch_csd / csd / coherence / transfer_function / cross_spectra): every output
bit for bit against a NumPy restatement of the arithmetic include/bhw.h writes down, for every single-output mask and the full mask;
P_xx and P_yy bit for bit against bhw.welch_psd; the broadcast of one X over many Y; the identities the arithmetic makes exact; graph
capture; the Python errors; and csd / coherence end to end against a float64 restatement of scipy.signal.csd / coherence, inside twice
the error of the torch-only float32 route measured in the same run."""
import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from test_gpu_stft import SPECIAL, _same

pytestmark = pytest.mark.gpu

BLOCK = B.WELCH_BLOCK
ALL = ("pxy", "pxx", "pyy", "coherence", "h1")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _f32(t):
    """A float32 or complex64 tensor / array as a float32 array (complex: interleaved pairs)."""
    a = np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t)
    return a.view(np.float32) if np.iscomplexobj(a) else a


def _same_out(got, want):
    return _same(_f32(got), _f32(want))


# ---- the restatement, written from include/bhw.h -------------------------------------------------------------------------------------

def _block_sum(t):
    """t (B, F, K) float64 -> (B, K): ascending f inside blocks of BLOCK frames from +0.0, then the block sums in order from +0.0."""
    nb, F, K = t.shape
    A = np.zeros((nb, K))
    for f0 in range(0, F, BLOCK):
        Ab = np.zeros((nb, K))
        for f in range(f0, min(F, f0 + BLOCK)):
            Ab = Ab + t[:, f, :]
        A = A + Ab
    return A


def _csd_ref(X, Y, scale, nfft, onesided):
    """X (B or 1, F, K), Y (B, F, K) complex64 -> the five outputs as the header writes them; every product of two float32 values is
    exact in binary64, so each term below is one rounding; nothing is fused."""
    nb, F, K = Y.shape
    with np.errstate(all="ignore"):
        xr, xi = X.real.astype(np.float64), X.imag.astype(np.float64)
        yr, yi = Y.real.astype(np.float64), Y.imag.astype(np.float64)
        if X.shape[0] != nb:
            xr, xi = np.broadcast_to(xr, (nb, F, K)), np.broadcast_to(xi, (nb, F, K))
        Sxx, Syy = _block_sum(xr * xr + xi * xi), _block_sum(yr * yr + yi * yi)
        Cre, Cim = _block_sum(xr * yr + xi * yi), _block_sum(xr * yi - xi * yr)
        s = np.full(K, np.float64(scale))
        if onesided:
            s[1:] *= 2.0
            if nfft % 2 == 0:
                s[-1] = np.float64(scale)
        pxy = np.empty((nb, K), dtype=np.complex64)
        pxy.real, pxy.imag = (Cre * s).astype(np.float32), (Cim * s).astype(np.float32)
        n, m = Cre * Cre, Cim * Cim
        num, den = n + m, Sxx * Syy
        h1 = np.empty((nb, K), dtype=np.complex64)
        h1.real, h1.imag = (Cre / Sxx).astype(np.float32), (Cim / Sxx).astype(np.float32)
        return {"pxy": pxy, "pxx": (Sxx * s).astype(np.float32), "pyy": (Syy * s).astype(np.float32),
                "coherence": (num / den).astype(np.float32), "h1": h1}


def _spectra(rng, nb, F, K, special, pad=3):
    """(nb, F, K + pad) complex64 on the host; with `special`, inf / NaN / huge / tiny / signed-zero parts of test_gpu_stft.SPECIAL."""
    Z = ((rng.standard_normal((nb, F, K + pad)) + 1j * rng.standard_normal((nb, F, K + pad))) * 1e3).astype(np.complex64)
    if special and F * K > 4:
        flat = Z.reshape(-1).view(np.float32)
        idx = rng.choice(flat.size, size=min(flat.size // 4 + 1, len(SPECIAL)), replace=False)
        flat[idx] = np.resize(SPECIAL, len(idx))
    return Z


# ---- bit-equality ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7])
@pytest.mark.parametrize("K", [1, 33, 257, 513])
def test_csd_equals_its_restatement(torch, F, K):
    """Every single-output mask and the full mask, one- and two-sided, packed and strided rows, with special values: bit-equal to the
    restatement (NaN by position), and a one-output call bit-equal to the same output of the full-mask call."""
    rng = np.random.default_rng(F * 1000 + K)
    nb = 2
    for nfft, onesided in ((2 * (K - 1) if K > 1 else 1, True), (2 * (K - 1) + 1, True), (K, False)):
        for strided in (False, True):
            Xh, Yh = _spectra(rng, nb, F, K, strided), _spectra(rng, nb, F, K, strided, pad=5)
            scale = 1.0 / (3.7 * F)
            Xd, Yd = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
            X, Y = (Xd[..., :K], Yd[..., :K]) if strided else (Xd[..., :K].contiguous(), Yd[..., :K].contiguous())
            want = _csd_ref(Xh[..., :K], Yh[..., :K], scale, nfft, onesided)
            full = bhw.welch_csd(X, Y, scale, nfft=nfft, onesided=onesided, outputs=ALL)
            assert tuple(full) == ALL
            for name in ALL:
                assert full[name].shape == (nb, K), name
                assert _same_out(full[name], want[name]), (F, K, nfft, onesided, strided, name, "full mask")
                one = bhw.welch_csd(X, Y, scale, nfft=nfft, onesided=onesided, outputs=(name,))
                assert tuple(one) == (name,) and _same_out(one[name], want[name]), (F, K, nfft, onesided, strided, name, "alone")
                assert _same_out(one[name], full[name]), (F, K, nfft, name, "alone against full")
            # 2-D operands: one signal
            one = bhw.welch_csd(X[1], Y[1], scale, nfft=nfft, onesided=onesided, outputs=ALL)
            for name in ALL:
                assert one[name].shape == (K,) and _same_out(one[name], want[name][1]), (F, K, nfft, name, "2-D")
            # strided outputs sharing one row stride: the gaps stay as they were
            bigs = {n: torch.full((nb, K + 5), -3.0, device="cuda", dtype=torch.complex64 if B.CSD_OUTPUTS[n][1] else torch.float32) for n in ALL}
            got = bhw.welch_csd(X, Y, scale, nfft=nfft, onesided=onesided, outputs=ALL, out={n: bigs[n][:, :K] for n in ALL})
            for name in ALL:
                assert got[name].data_ptr() == bigs[name].data_ptr()
                assert _same_out(bigs[name][:, :K], want[name]) and bool((bigs[name][:, K:] == -3.0).all()), (F, K, nfft, name, "gaps")


@pytest.mark.parametrize("shape", [(64, 300, 257), (3, 998, 129), (1, 2000, 2049), (64, 200, 257)])
def test_pxx_and_pyy_are_the_periodograms_of_welch_psd(torch, shape):
    """The existing call is the yardstick: P_xx / P_yy of any mask that holds them equal bhw.welch_psd of X / of Y on the same tensors."""
    nb, F, K = shape
    g = torch.Generator(device="cuda").manual_seed(F + K)
    X = torch.view_as_complex(torch.randn((nb, F, K, 2), device="cuda", generator=g) * 50.0)
    Y = torch.view_as_complex(torch.randn((nb, F, K, 2), device="cuda", generator=g) * 0.02 + 1.0)
    nfft, scale = 2 * (K - 1), 1.0 / (F * 17.0)
    Pxx, Pyy = bhw.welch_psd(X, scale, nfft=nfft), bhw.welch_psd(Y, scale, nfft=nfft)
    for outs in (("pxx",), ("pyy",), ("pxx", "pyy"), ("pxy", "pxx"), ALL):
        r = bhw.welch_csd(X, Y, scale, nfft=nfft, outputs=outs)
        if "pxx" in outs:
            assert torch.equal(r["pxx"], Pxx), (shape, outs)
        if "pyy" in outs:
            assert torch.equal(r["pyy"], Pyy), (shape, outs)
    two = bhw.welch_csd(X, Y, scale, nfft=K, onesided=False, outputs=("pxx", "pyy"))
    assert torch.equal(two["pxx"], bhw.welch_psd(X, scale, nfft=K, onesided=False))
    assert torch.equal(two["pyy"], bhw.welch_psd(Y, scale, nfft=K, onesided=False))


@pytest.mark.parametrize("F,K", [(1, 33), (200, 257), (BLOCK + 1, 65), (3 * BLOCK + 7, 513)])
def test_broadcast_x_equals_the_expanded_call(torch, F, K):
    """X (F, K) against Y (B, F, K): bit for bit the call on X.expand(B, ...).contiguous(), and the restatement."""
    rng = np.random.default_rng(F + 7 * K)
    nb = 5
    Xh, Yh = _spectra(rng, 1, F, K, True, pad=0), _spectra(rng, nb, F, K, True, pad=0)
    X, Y = torch.from_numpy(Xh[0]).cuda(), torch.from_numpy(Yh).cuda()
    nfft, scale = 2 * (K - 1), 0.37 / F
    want = _csd_ref(Xh, Yh, scale, nfft, True)
    for outs in (("pxy",), ALL):
        ex = bhw.welch_csd(X.expand(nb, F, K).contiguous(), Y, scale, nfft=nfft, outputs=outs)
        for Xb in (X, X.unsqueeze(0), X.expand(nb, F, K)):           # 2-D, one signal, and a stride-0 view (copied by the binding)
            bc = bhw.welch_csd(Xb, Y, scale, nfft=nfft, outputs=outs)
            for name in outs:
                assert bc[name].shape == (nb, K)
                assert _same_out(bc[name], ex[name]) and _same_out(bc[name], want[name]), (F, K, outs, name)
    assert "X broadcast" in B.describe_csd(B.make_csd(nb, F, K, nfft, scale, outputs=ALL, onesided=True, broadcast_x=True))


def test_identities_that_the_arithmetic_makes_exact(torch):
    """Each of these is exact by the arithmetic of include/bhw.h, not approximately true.
    (1) csd(X, X): re_f = xr * xr + xi * xi is xx_f, the periodogram's q_f, term by term, summed in the same order and scaled by the same
        s_k, so Re P_xy is bit-equal to welch_psd(X); im_f = xr * xi - xi * xr is the difference of one exact product with itself, +0
        in every frame (round to nearest), the sum of +0's from +0.0 is +0, and +0 times a positive scale is +0.
    (2) Swapping the operands: re_f is symmetric in (x, y) as real arithmetic of exact products with one rounding, im_f changes sign
        exactly (a - b = -(b - a) under round to nearest, except that 0 stays +0).  Sums of negated terms are negated sums, again up to the
        sign of a zero.  So P_yx == conj(P_xy) as values, and the coherence -- squares of C_re and C_im, and S_xx * S_yy commuted -- is
        bit-equal.
    (3) Coherence of (X, X): C_im = +0, so m = +0 and num = rn(C_re^2) + 0 = rn(S_xx^2), and den = rn(S_xx * S_xx) is the same rounded
        square; for finite non-zero data S_xx lies in [2^-298, 2^291), so the square neither overflows nor underflows to zero and
        num / den = 1 exactly.  An all-zero bin gives 0 / 0 = NaN."""
    g = torch.Generator(device="cuda").manual_seed(5)
    nb, F, K = 3, 2 * BLOCK + 9, 257
    nfft, scale = 512, 1.0 / (F * 3.0)
    X = torch.view_as_complex(torch.randn((nb, F, K, 2), device="cuda", generator=g) * 7.0)
    Y = torch.view_as_complex(torch.randn((nb, F, K, 2), device="cuda", generator=g) + 0.5)
    X[1, :, 40] = 0                                                  # an all-zero bin of one signal
    X[2, :, 41] *= 1e-19                                             # tiny and huge but finite bins
    X[2, :, 42] *= 1e15
    xx = bhw.welch_csd(X, X, scale, nfft=nfft, outputs=ALL)
    Pxx = bhw.welch_psd(X, scale, nfft=nfft)
    assert torch.equal(xx["pxy"].real, Pxx) and torch.equal(xx["pxx"], Pxx) and torch.equal(xx["pyy"], Pxx)
    im = xx["pxy"].imag.contiguous()
    assert bool((im == 0).all()) and bool((im.view(torch.int32) == 0).all())     # +0, bit for bit
    coh = xx["coherence"]
    zero = torch.zeros_like(coh, dtype=torch.bool)
    zero[1, 40] = True
    assert bool(torch.isnan(coh[zero]).all()) and bool((coh[~zero] == 1.0).all())
    assert bool((xx["h1"].real[~zero] == 1.0).all()) and bool((xx["h1"].imag[~zero] == 0).all())
    xy, yx = bhw.welch_csd(X, Y, scale, nfft=nfft, outputs=ALL), bhw.welch_csd(Y, X, scale, nfft=nfft, outputs=ALL)
    assert bool((yx["pxy"] == xy["pxy"].conj()).all())
    assert _same_out(yx["coherence"], xy["coherence"])
    assert torch.equal(yx["pxx"], xy["pyy"]) and torch.equal(yx["pyy"], xy["pxx"])
    c = xy["coherence"][~zero]
    assert bool((c >= 0).all()) and bool((c <= 1.0 + 1e-6).all())
    # the same through the chain: csd(x, x) against welch(x)
    p = B.make_params(B.WIN_BH7, 12, 32)
    x = torch.randn((2, 50000), device="cuda", generator=g) + 3.0
    f, Pw = bhw.welch(p, x, 2.0, length=400, noverlap=240, nfft=512)
    fc, Pc = bhw.csd(p, x, x, 2.0, length=400, noverlap=240, nfft=512)
    assert torch.equal(f, fc) and torch.equal(Pc.real, Pw) and bool((Pc.imag.contiguous().view(torch.int32) == 0).all())


def test_a_nan_poisons_its_own_bin_only(torch):
    g = torch.Generator(device="cuda").manual_seed(9)
    nb, F, K = 2, BLOCK + 40, 65
    X = torch.view_as_complex(torch.randn((nb, F, K, 2), device="cuda", generator=g))
    Y = torch.view_as_complex(torch.randn((nb, F, K, 2), device="cuda", generator=g))
    torch.view_as_real(Y)[1, BLOCK + 3, 17, 0] = float("nan")
    torch.view_as_real(X)[0, 5, 3, 1] = float("inf")
    r = bhw.welch_csd(X, Y, 0.1, nfft=128, outputs=ALL)
    bad = torch.zeros((nb, K), dtype=torch.bool, device="cuda")
    bad[1, 17] = True
    bad[0, 3] = True
    for name in ("pxy", "coherence", "h1"):
        t = r[name]
        fin = torch.isfinite(torch.view_as_real(t)).all(-1) if t.is_complex() else torch.isfinite(t)
        assert torch.equal(~fin, bad), name
    assert bool(torch.isfinite(r["pxx"][1]).all()) and bool(torch.isfinite(r["pyy"][0]).all())


# ---- the chain --------------------------------------------------------------------------------------------------------------------------

def test_graph_capture_of_cross_spectra_from_a_table(torch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    L, nfft, T, nb = 400, 512, 48000, 4                              # 299 segments: two frame blocks
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((T,), device="cuda", generator=g) + 5.0          # one excitation against four responses
    y = torch.randn((nb, T), device="cuda", generator=g) - 1.0
    kw = dict(length=L, noverlap=240, nfft=nfft)
    with bhw.ResidentTable(p) as tab:
        tab.cross_spectra(p, x, y, 16000.0, **kw)                    # the warm call reads the window sums
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                f, r = tab.cross_spectra(p, x, y, 16000.0, **kw)
        torch.cuda.current_stream().wait_stream(s)
        x.copy_(torch.randn((T,), device="cuda", generator=g) * 3.0 - 2.0)               # new data in the captured inputs
        y.copy_(0.5 * x + torch.randn((nb, T), device="cuda", generator=g))
        for t in r.values():
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        fe, re = tab.cross_spectra(p, x, y, 16000.0, **kw)
        fl, rl = bhw.cross_spectra(p, x, y, 16000.0, **kw)
        assert tuple(r) == ALL and torch.equal(f, fe) and torch.equal(f, fl)
        for name in ALL:
            assert r[name].shape == (nb, nfft // 2 + 1)
            assert _same_out(r[name], re[name]) and _same_out(rl[name], re[name]), name
        assert bool((r["pxx"] > 0).all()) and bool((r["coherence"] > 0).all())
        # the one-output calls are the same pass with another mask
        assert _same_out(tab.csd(p, x, y, 16000.0, **kw)[1], re["pxy"])
        assert _same_out(tab.coherence(p, x, y, 16000.0, **kw)[1], re["coherence"])
        assert _same_out(tab.transfer_function(p, x, y, 16000.0, **kw)[1], re["h1"])
        assert _same_out(bhw.coherence(p, x, y, 16000.0, **kw)[1], re["coherence"])
        assert _same_out(bhw.transfer_function(p, x, y, 16000.0, **kw)[1], re["h1"])
        assert torch.equal(re["pyy"], tab.welch(p, y, 16000.0, **kw)[1])
        assert torch.equal(re["pxx"][2], tab.welch(p, x, 16000.0, **kw)[1])


def test_cross_spectra_under_capture_needs_the_sums_read_first(torch, monkeypatch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    x = torch.zeros((2, 4000), device="cuda")
    with bhw.ResidentTable(p) as tab:
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="window sums"):
            tab.cross_spectra(p, x, x, length=397)
        monkeypatch.undo()
        tab.cross_spectra(p, x, x, length=397)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        tab.cross_spectra(p, x, x, length=397)                       # cached: no read, no error
        monkeypatch.undo()
    torch.cuda.synchronize()


def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    x = torch.zeros((2, 1000), device="cuda")
    with pytest.raises(ValueError, match="same length"):
        bhw.csd(p, x, x[:, :900], length=64)
    with pytest.raises(ValueError, match="same dtype"):
        bhw.csd(p, x, x.to(torch.complex64), length=64)
    with pytest.raises(ValueError, match="float32 or complex64"):
        bhw.coherence(p, x, x.double(), length=64)
    with pytest.raises(ValueError, match="CUDA"):
        bhw.csd(p, x, x.cpu(), length=64)
    with pytest.raises(ValueError, match="CUDA"):
        bhw.csd(p, x.cpu(), x, length=64)
    with pytest.raises(ValueError, match="outputs"):
        bhw.cross_spectra(p, x, x, length=64, outputs=("pxy", "gain"))
    with pytest.raises(ValueError, match="outputs"):
        bhw.cross_spectra(p, x, x, length=64, outputs=())
    with pytest.raises(ValueError, match="batch"):
        bhw.csd(p, x, x[0], length=64)                               # a batched x needs a batched y
    with pytest.raises(ValueError, match="batch"):
        bhw.csd(p, x, torch.zeros((3, 1000), device="cuda"), length=64)
    with pytest.raises(ValueError, match="detrend"):
        bhw.csd(p, x, x, length=64, detrend="linear")
    with pytest.raises(ValueError, match="scaling"):
        bhw.csd(p, x, x, length=64, scaling="power")
    with pytest.raises(ValueError, match="noverlap"):
        bhw.csd(p, x, x, length=64, noverlap=64)
    with pytest.raises(ValueError, match="nfft"):
        bhw.csd(p, x, x, length=64, nfft=63)
    with pytest.raises(ValueError, match="zero segments"):
        bhw.csd(p, x[:, :50], x[:, :50], length=64)
    with pytest.raises(ValueError, match=r"\(T,\) or \(B, T\)"):
        bhw.csd(p, x.reshape(2, 10, 100), x.reshape(2, 10, 100), length=64)
    X = torch.zeros((2, 5, 33), dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError, match="complex64"):
        bhw.welch_csd(X.real.contiguous(), X, 1.0, nfft=64)
    with pytest.raises(ValueError, match="complex64"):
        bhw.welch_csd(X, X.real.contiguous(), 1.0, nfft=64)
    with pytest.raises(ValueError, match="bins"):
        bhw.welch_csd(X, X, 1.0, nfft=100)
    with pytest.raises(ValueError, match=r"\(frames, bins\)"):
        bhw.welch_csd(X[0, 0], X, 1.0, nfft=64)
    with pytest.raises(ValueError, match="same frames and bins"):
        bhw.welch_csd(X[:, :4], X, 1.0, nfft=64)
    with pytest.raises(ValueError, match="batched Y"):
        bhw.welch_csd(X, X[0], 1.0, nfft=64)
    with pytest.raises(ValueError, match="outputs"):
        bhw.welch_csd(X, X, 1.0, nfft=64, outputs=("pxy", "pxy"))
    with pytest.raises(ValueError, match="out must be a dict"):
        bhw.welch_csd(X, X, 1.0, nfft=64, out={"pxx": torch.zeros((2, 33), device="cuda")})     # not among the outputs asked for
    with pytest.raises(ValueError, match=r"out\['pxy'\] must be"):
        bhw.welch_csd(X, X, 1.0, nfft=64, out={"pxy": torch.zeros((2, 33), device="cuda")})     # float32 where complex64 is written
    with pytest.raises(ValueError, match=r"out\['pxx'\] must be"):
        bhw.welch_csd(X, X, 1.0, nfft=64, outputs=("pxx",), out={"pxx": torch.zeros((2, 32), device="cuda")})
    with pytest.raises(ValueError, match="same row stride"):
        bhw.welch_csd(X, X, 1.0, nfft=64, outputs=("pxx", "pyy"),
                      out={"pxx": torch.zeros((2, 33), device="cuda"), "pyy": torch.zeros((2, 40), device="cuda")[:, :33]})
    with pytest.raises(B.BhwError, match="not finite"):
        bhw.welch_csd(X, X, float("inf"), nfft=64)


# ---- end to end against the model ------------------------------------------------------------------------------------------------------

def _v(p, L):
    w = bhw.window(p, L).cpu().numpy()
    return np.ldexp(w.astype(np.float32), -(p.dat_width - 1)).astype(np.float32)


def _cross_ref64(x, y, v, fs, L, noverlap, nfft, detrend=True, scaling="density"):
    """scipy.signal.csd(x, y, fs, window=v, ...) and scipy.signal.coherence restated in NumPy float64: (freqs, Pxy, Cxy)."""
    x, y, v = (np.asarray(t, dtype=np.float64) for t in (x, y, v))
    hop = L - noverlap
    F = (x.shape[-1] - noverlap) // hop
    idx = np.arange(F)[:, None] * hop + np.arange(L)[None, :]
    sx, sy = x[..., idx], y[..., idx]
    if detrend:
        sx, sy = sx - sx.mean(axis=-1, keepdims=True), sy - sy.mean(axis=-1, keepdims=True)
    X, Y = np.fft.rfft(sx * v, n=nfft, axis=-1), np.fft.rfft(sy * v, n=nfft, axis=-1)
    scale = 1.0 / (fs * (v * v).sum()) if scaling == "density" else 1.0 / v.sum() ** 2
    d = np.full(nfft // 2 + 1, 2.0 * scale)
    d[0] = scale
    if nfft % 2 == 0:
        d[-1] = scale
    Pxy = (np.conj(X) * Y).mean(axis=-2) * d
    Pxx, Pyy = (np.abs(X) ** 2).mean(axis=-2) * d, (np.abs(Y) ** 2).mean(axis=-2) * d
    return np.fft.rfftfreq(nfft, 1.0 / fs), Pxy, np.abs(Pxy) ** 2 / (Pxx * Pyy)


def _torch_route(torch, x, y, v, fs, L, noverlap, nfft):
    """The torch-only float32 route: unfold, subtract mean, multiply, rfft, (X.conj() * Y).mean, abs() ** 2; (Pxy, Cxy)."""
    def spec(t):
        seg = t.unfold(-1, L, L - noverlap)
        return torch.fft.rfft((seg - seg.mean(-1, keepdim=True)) * v, n=nfft)
    X, Y = spec(x), spec(y)
    d = torch.full((nfft // 2 + 1,), 2.0, device=x.device)
    d[0] = 1.0
    if nfft % 2 == 0:
        d[-1] = 1.0
    d = d * (1.0 / (fs * (v * v).sum()))
    Pxy = (X.conj() * Y).mean(-2) * d
    Pxx, Pyy = (X.abs() ** 2).mean(-2) * d, (Y.abs() ** 2).mean(-2) * d
    return Pxy, Pxy.abs() ** 2 / (Pxx * Pyy)


def _butter4_lowpass(x, wn):
    """A 4th-order Butterworth low-pass (cutoff wn of Nyquist) by the bilinear transform, applied in float64 as two direct-form
    biquads -- what scipy.signal.butter(4, wn) + lfilter do, written out so that the test needs no scipy."""
    wa = 2.0 * np.tan(np.pi * wn / 2.0)                              # prewarped analog cutoff at fs = 1
    y = np.asarray(x, dtype=np.float64)
    for k in (0, 1):                                                 # the two conjugate pole pairs
        th = np.pi * (2 * k + 5) / 8.0
        re = 2.0 * wa * np.cos(th)                                   # s^2 - re s + wa^2
        a0 = 4.0 - 2.0 * re + wa * wa
        b = np.array([wa * wa, 2.0 * wa * wa, wa * wa]) / a0
        a1, a2 = (2.0 * wa * wa - 8.0) / a0, (4.0 + 2.0 * re + wa * wa) / a0
        out = np.empty_like(y)
        y1 = y2 = u1 = u2 = 0.0
        for n, u in enumerate(y.tolist()):
            o = b[0] * u + b[1] * u1 + b[2] * u2 - a1 * y1 - a2 * y2
            out[n] = o
            u2, u1, y2, y1 = u1, u, y1, o
        y = out
    return y


def _pair(T, seed, strong):
    """x: unit-variance white noise + a tone of amplitude `strong` + one of 1e-3 + a DC offset of 0.5 (the structure of section 15's
    signal); y: a 4th-order Butterworth low-pass of x (cutoff 0.2 cycles per sample: the strong tone passes, the weak one does not) +
    independent unit-variance noise + another offset.  The noise level is the one under which a CPU rehearsal of both routes (pocketfft's
    float32 FFT) lands where the issue that set these tests says its own rehearsal did: coherence errors of 6e-8 .. 4e-7 at strong = 4.
    With the noise 20 dB lower the tone's bin stands 65 dB above the noise floor, and the coherence error of BOTH routes is the float32
    FFT's own noise beside the tone (1e-4 absolute): an input that measures the FFT, not the code around it."""
    rng = np.random.default_rng(seed)
    n = np.arange(T, dtype=np.float64)
    x = strong * np.cos(2 * np.pi * 0.1234 * n) + 1e-3 * np.cos(2 * np.pi * 0.31 * n + 1.0) + rng.standard_normal(T) + 0.5
    y = _butter4_lowpass(x - 0.5, 0.4) + rng.standard_normal(T) - 0.25
    return x.astype(np.float32), y.astype(np.float32)


def test_butterworth_and_restatement_match_scipy(torch):
    signal = pytest.importorskip("scipy.signal")
    p = B.make_params(B.WIN_BH7, 16, 32)
    x, y = _pair(50000, 3, 4.0)
    b, a = signal.butter(4, 0.4)
    u = np.random.default_rng(1).standard_normal(5000)
    assert np.abs(signal.lfilter(b, a, u) - _butter4_lowpass(u, 0.4)).max() < 1e-10
    x, y = x.astype(np.float64), y.astype(np.float64)
    for L, nov, nfft in ((4096, 2048, 4096), (400, 240, 512), (401, 100, 513)):
        v = _v(p, L).astype(np.float64)
        for scaling in ("density", "spectrum"):
            f0, P0 = signal.csd(x, y, 2.0, window=v, noverlap=nov, nfft=nfft, detrend="constant", scaling=scaling)
            f1, P1, C1 = _cross_ref64(x, y, v, 2.0, L, nov, nfft, True, scaling)
            assert np.allclose(f0, f1, rtol=0, atol=1e-15)
            assert np.abs(P0 - P1).max() <= 1e-12 * np.abs(P0).max(), (L, scaling)
        _, C0 = signal.coherence(x, y, 2.0, window=v, noverlap=nov, nfft=nfft, detrend="constant")
        assert np.abs(C0 - C1).max() <= 1e-10, L


@pytest.mark.parametrize("L,noverlap,nfft", [(4096, 2048, 4096), (400, 240, 512)])
def test_csd_end_to_end_within_twice_the_torch_route(torch, L, noverlap, nfft):
    """BH-7 at 32 bits, T = 200 000, three seeds.  x: white noise + tones of amplitude 1e3 and 1e-3 + a DC offset; y: a 4th-order
    Butterworth low-pass of x + independent noise + another offset.  The reference is the float64 restatement of scipy.signal.csd with
    the window given as the array v; the yardstick is the error of the torch-only float32 route against it on the same GPU,
    max |dPxy| / max |Pxy|.  bhw.csd must stay within 2x the yardstick: both routes share the float32 FFT's error, which dominates.
    Measured on an MI355X: see DESIGN.md section 16."""
    p = B.make_params(B.WIN_BH7, 16, 32)
    vh = _v(p, L)
    for seed in (5, 6, 7):
        xh, yh = _pair(200000, seed, 1e3)
        x, y = torch.from_numpy(xh).cuda(), torch.from_numpy(yh).cuda()
        fr, ref, _ = _cross_ref64(xh, yh, vh, 1.0, L, noverlap, nfft)
        f, P = bhw.csd(p, x, y, 1.0, length=L, noverlap=noverlap, nfft=nfft)
        with bhw.ResidentTable(p) as tab:
            ft, Pt = tab.csd(p, x, y, 1.0, length=L, noverlap=noverlap, nfft=nfft)
        assert _same_out(P, Pt) and torch.equal(f, ft)
        assert f.dtype == torch.float64 and np.allclose(f.cpu().numpy(), fr, rtol=0, atol=1e-15)
        Pyard, _ = _torch_route(torch, x, y, torch.from_numpy(vh).cuda(), 1.0, L, noverlap, nfft)
        top = np.abs(ref).max()
        yard = float(np.abs(Pyard.cpu().numpy().astype(np.complex128) - ref).max() / top)
        err = float(np.abs(P.cpu().numpy().astype(np.complex128) - ref).max() / top)
        print(f"csd end to end L={L} nfft={nfft} hop={L - noverlap} seed={seed}: bhw.csd {err:.3e}, torch-only route {yard:.3e}, "
              f"ratio {err / yard:.3f}")
        assert err <= 2.0 * yard, (seed, err, yard)


@pytest.mark.parametrize("L,noverlap,nfft", [(4096, 2048, 4096), (400, 240, 512)])
def test_coherence_end_to_end_within_twice_the_torch_route(torch, L, noverlap, nfft):
    """The pair of the csd test with the strong tone at amplitude 4 instead of 1e3 (with the 120 dB pair the coherence error of both
    routes is the FFT's noise in the bins beside the tone, and their ratio says nothing), three seeds.  Reference: the float64
    restatement of scipy.signal.coherence; yardstick: the torch-only float32 route on the same GPU; error: max |dCxy| (absolute,
    C in [0, 1]); bound 2x the yardstick.  Measured on an MI355X: see DESIGN.md section 16."""
    p = B.make_params(B.WIN_BH7, 16, 32)
    vh = _v(p, L)
    for seed in (5, 6, 7):
        xh, yh = _pair(200000, seed, 4.0)
        x, y = torch.from_numpy(xh).cuda(), torch.from_numpy(yh).cuda()
        _, _, ref = _cross_ref64(xh, yh, vh, 1.0, L, noverlap, nfft)
        f, C = bhw.coherence(p, x, y, 1.0, length=L, noverlap=noverlap, nfft=nfft)
        _, Cyard = _torch_route(torch, x, y, torch.from_numpy(vh).cuda(), 1.0, L, noverlap, nfft)
        yard = float(np.abs(Cyard.cpu().numpy().astype(np.float64) - ref).max())
        err = float(np.abs(C.cpu().numpy().astype(np.float64) - ref).max())
        print(f"coherence end to end L={L} nfft={nfft} hop={L - noverlap} seed={seed}: bhw.coherence {err:.3e}, torch-only route {yard:.3e}, "
              f"ratio {err / yard:.3f}")
        assert err <= 2.0 * yard, (seed, err, yard)
