"""The mixed-radix fused window + complex FFT kernel for I/Q input on the GPU (bhw_stft_cmfft_f32_* through bhw.stft_iq_mixed,
bhw.spectrogram_iq_mixed and the ResidentTable methods).

The gates are the family's two, with no new numbers: for every case of tests/stft_cmfft_cases.py the reference is numpy.fft.fft in
float64 of the float32 rows (restated by the NumPy references of test_gpu_stft.py and test_gpu_welch.py with two channels), the
metric the largest relative l2 error of a spectrum row, the yardstick torch.fft.fft on the same GPU over the rows stft_frames /
welch_frames write for the complex64 x, and the bound twice the yardstick's error under a cap of 2^-24 * log2(n_fft).  The FFT is
not pinned bit for bit; everything around it is -- the shifted bins (odd n_fft too), the power rows, the strides, the slot, library
against table -- and those properties are held word for word."""
import ctypes
import math

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from test_gpu_stft import _same
from test_gpu_welch import _rel_err
from test_gpu_spectrogram import _power_ref
from test_gpu_stft_iq import (SENTINEL, _bits, _case_signal, _complex, _kw, _padded_io, _pairs, _parent_rows, _row_errors, _rows_ref,
                              _v)

import stft_cmfft_cases as XC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _call(p, c, x, table=None, out=None, power=False, fftshift=False):
    src = bhw if table is None else table
    fn = src.spectrogram_iq_mixed if power else src.stft_iq_mixed
    return fn(p, x, c["n_fft"], c["hop"], detrend=bool(c["detrend"]), fftshift=fftshift, out=out, **_kw(c))


@pytest.mark.parametrize("cid", XC.case_ids())
def test_accuracy_within_twice_rocfft_on_the_same_rows(torch, cid):
    c = XC.case(cid)
    p = XC.params(c["setup"])
    n = c["n_fft"]
    xh = _case_signal(c)
    v = _v(p, c["L"])
    pairs = _rows_ref(c, xh, v)
    rows = _complex(pairs)
    x = torch.from_numpy(xh).cuda()
    parent = _parent_rows(torch, p, c, x)
    assert parent.dtype == torch.complex64
    assert _same(torch.view_as_real(parent).cpu().numpy(), pairs), "the parent's rows are the restated rows"
    yard = _row_errors(torch.fft.fft(parent, dim=-1).cpu().numpy(), rows)
    Y = _call(p, c, x)
    assert Y.dtype == torch.complex64 and tuple(Y.shape) == rows.shape[:2] + (n,)
    power, shifted = bool(c.get("power")), bool(c.get("fftshift"))
    with bhw.ResidentTable(p) as tab:
        d = XC.parse(XC.line(c, table=tab._live()))
        assert d["table"] and "k_stft_cmfft_table" in d["kernels"] and (d["power"], d["shifted"]) == (power, shifted), d["line"]
        lib = XC.parse(XC.line(c))
        assert all(d[k] == lib[k] for k in ("schedule", "lpf", "fy", "cpl", "groups", "grid", "lds", "fold")), (d["line"], lib["line"])
        Yt = _call(p, c, x, table=tab)
        torch.cuda.synchronize()
    assert np.array_equal(_bits(torch, Yt), _bits(torch, Y)), "library against table"
    # the form the case names (power rows, shifted bins, padded strides) against the spectrum, word for word
    if power or shifted or c.get("padded"):
        want = torch.fft.fftshift(Y, dim=-1) if shifted else Y
        want = _power_ref(want.cpu().numpy()).view(np.uint32) if power else _bits(torch, want)
        if c.get("padded"):
            xv, ybuf, out, gaps = _padded_io(torch, c, xh, power)
            named = _call(p, c, xv, out=out, power=power, fftshift=shifted)
            assert named.data_ptr() == out.data_ptr()
            assert bool((ybuf[gaps] == SENTINEL).all()), "a gap was written"
        else:
            named = _call(p, c, x, power=power, fftshift=shifted)
        assert named.dtype == (torch.float32 if power else torch.complex64) and tuple(named.shape) == tuple(Y.shape)
        assert np.array_equal(_bits(torch, named), want), "the named form against the spectrum"
    Yh = Y.cpu().numpy()
    err = _row_errors(Yh, rows)
    cap = 2.0 ** -24 * math.log2(n)
    print(f"stft iq mixed {cid}: n_fft {n} L {c['L']} rows {rows.shape[0] * rows.shape[1]}: fused {err:.3e}, torch.fft.fft on the parent's "
          f"rows {yard:.3e}, ratio {err / yard:.3f}, cap {cap:.3e}")
    assert err <= 2.0 * yard, (cid, err, yard)
    assert err <= cap, (cid, err, cap)


@pytest.mark.parametrize("cid", ["n25-reflect-shift", "n2025-detrend"])
def test_a_row_depends_on_nothing_but_itself(torch, cid):
    """n_fft 25 (32 rows per workgroup, odd, the last column missing) and 2025 (one row per workgroup, odd, 8 columns, the last one
    missing).  The same signal alone and as signal 37 of a batch of 64; its later rows as the first rows of a copy shifted by three
    hops (another slot of the workgroup and another group) -- every frame where there is no padding, the frames no padding reaches
    where there is; packed against padded strides, the sentinels of every gap intact; library against table; the shifted bins against
    torch.fft.fftshift; the power rows against fl32(re^2 + im^2) in float64 of the same call.  Word for word."""
    c = dict(XC.case(cid), B=1, power=False, fftshift=False)
    p = XC.params(c["setup"])
    T = 400 if c["n_fft"] == 25 else c["T"]
    c["T"] = T
    rng = np.random.default_rng(7)
    xh = ((rng.standard_normal((64, T)) + 1j * rng.standard_normal((64, T))) * 100 + (3 - 2j)).astype(np.complex64)
    x = torch.from_numpy(xh).cuda()
    alone = _call(p, c, x[37:38].clone())
    batch = _call(p, dict(c, B=64), x)
    assert np.array_equal(_bits(torch, alone[0]), _bits(torch, batch[37]))
    hop, n = c["hop"], c["n_fft"]
    shifted = _call(p, dict(c, T=T - 3 * hop), x[37:38, 3 * hop:].clone())
    if c["detrend"] or not c["mode"]:                                  # no padding: frame f + 3 of x is frame f of x[3 * hop:]
        assert shifted.shape[1] == alone.shape[1] - 3 >= 1
        assert np.array_equal(_bits(torch, shifted[0]), _bits(torch, alone[0, 3:]))
    else:                                                              # centred: the same holds for the frames no padding reaches
        pad = n // 2
        inner = [f for f in range(shifted.shape[1]) if f * hop - pad >= 0 and f * hop - pad + n <= T - 3 * hop]
        assert len(inner) >= 4
        assert np.array_equal(_bits(torch, shifted[0, inner]), _bits(torch, alone[0, [f + 3 for f in inner]]))
    # the shifted bins and the power rows of the same call
    turned = _call(p, c, x[37:38], fftshift=True)
    assert np.array_equal(_bits(torch, turned), _bits(torch, torch.fft.fftshift(alone, dim=-1)))
    pw = _call(p, c, x[37:38], power=True)
    assert pw.dtype == torch.float32 and np.array_equal(_bits(torch, pw), _power_ref(alone.cpu().numpy()).view(np.uint32))
    pws = _call(p, c, x[37:38], power=True, fftshift=True)
    assert np.array_equal(_bits(torch, pws), _bits(torch, torch.fft.fftshift(pw, dim=-1)))
    # padded x and output strides, both forms
    for power in (False, True):
        cp = dict(c, B=5, padded=True)
        xv, ybuf, out, gaps = _padded_io(torch, cp, xh[35:40], power)
        _call(p, cp, xv, out=out, power=power)
        assert np.array_equal(_bits(torch, out[2]), _bits(torch, (pw if power else alone)[0]))
        assert bool((ybuf[gaps] == SENTINEL).all()), "a gap was written"
    with bhw.ResidentTable(p) as tab:
        assert np.array_equal(_bits(torch, _call(p, c, x[37:38].clone(), table=tab)), _bits(torch, alone))
        assert np.array_equal(_bits(torch, _call(p, c, x[37:38].clone(), table=tab, power=True, fftshift=True)), _bits(torch, pws))
        torch.cuda.synchronize()


@pytest.mark.parametrize("n_fft,L,hop", [(18, 13, 5), (2025, 2025, 700)])
def test_x_off_the_eight_byte_grid_is_read_by_four_byte_loads(torch, n_fft, L, hop):
    """x is read under the frames call's rule: 4-byte alignment, any signal stride in floats.  The same samples one float off the
    8-byte grid, with an odd stride, through the C entry point: the bits of the aligned call."""
    p = B.make_params(B.WIN_BH7, 12, 32)
    nb, T = 3, 6000
    rng = np.random.default_rng(11)
    xh = ((rng.standard_normal((nb, T)) + 1j * rng.standard_normal((nb, T))) * 50 + (1 + 4j)).astype(np.complex64)
    want = bhw.stft_iq_mixed(p, torch.from_numpy(xh).cuda(), n_fft, hop, win_length=L, center=True, pad_mode="reflect")
    frames = want.shape[1]
    xs = 2 * T + 1
    buf = torch.full((1 + nb * xs,), SENTINEL, device="cuda")
    assert buf.data_ptr() % 8 == 0
    buf[1:].view(nb, xs)[:, :2 * T] = torch.from_numpy(_pairs(xh).reshape(nb, 2 * T)).cuda()
    got = torch.zeros_like(want)
    s = B.make_stft(nb, T, frames, hop, n_fft, col0=(n_fft - L) // 2, pad=n_fft // 2, pad_mode=B.PAD_REFLECT, channels=2, shift=p.dat_width - 1,
                    x_stride=xs)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    B.check(B.lib().bhw_stft_cmfft_f32_device(ctypes.byref(p), L, torch.cuda.current_device(), stream, ctypes.byref(s), 0,
                                              ctypes.c_void_p(buf.data_ptr() + 4), ctypes.c_void_p(got.data_ptr())))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(torch, got), _bits(torch, want))


@pytest.mark.parametrize("n_fft,L,hop", [(25, 20, 9), (2025, 2025, 700)])
def test_zero_signal_gives_zeros_and_a_nan_reaches_only_its_rows(torch, n_fft, L, hop):
    p = B.make_params(B.WIN_BH7, 12, 32)
    T = 8000
    for power in (False, True):
        fn = bhw.spectrogram_iq_mixed if power else bhw.stft_iq_mixed
        z = fn(p, torch.zeros((2, T), dtype=torch.complex64, device="cuda"), n_fft, hop, win_length=L)
        assert not bool((torch.view_as_real(z) if z.is_complex() else z).ne(0).any())
    rng = np.random.default_rng(3)
    xh = ((rng.standard_normal((3, T)) + 1j * rng.standard_normal((3, T))) * 10 + (1 - 1j)).astype(np.complex64)
    for detrend in (False, True):
        kw = dict(win_length=L, center=False, detrend=detrend)
        clean = bhw.stft_iq_mixed(p, torch.from_numpy(xh).cuda(), n_fft, hop, **kw)
        for bad in ("a NaN in a real part", "an infinity in an imaginary part"):
            xn = xh.copy()
            t0 = 4000
            xn[1, t0] = np.complex64(complex(np.nan, xh[1, t0].imag) if "NaN" in bad else complex(xh[1, t0].real, np.inf))
            got = bhw.stft_iq_mixed(p, torch.from_numpy(xn).cuda(), n_fft, hop, **kw)
            frames = clean.shape[1]
            col0 = 0 if detrend else (n_fft - L) // 2
            hit = np.zeros((3, frames), dtype=bool)
            for f in range(frames):
                hit[1, f] = f * hop + col0 <= t0 < f * hop + col0 + L
            assert hit.sum() in (2, 3, 4)
            finite = torch.isfinite(torch.view_as_real(got)).all(-1).all(-1).cpu().numpy()
            assert np.array_equal(~finite, hit), (detrend, bad)
            assert np.array_equal(_bits(torch, got)[~hit], _bits(torch, clean)[~hit])


def test_against_torch_stft(torch):
    """The bound of test_gpu_stft_iq.test_against_torch_stft at 400 / 400 / 160 reflect, 75 / 75 / 20 constant (odd) and
    1536 / 1200 / 384 with no padding, complex x, all n_fft bins."""
    p = B.make_params(B.WIN_BH7, 12, 32)
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.view_as_complex(torch.randn((3, 5000, 2), device="cuda", generator=g))
    for n_fft, L, hop, center, mode in ((400, 400, 160, True, "reflect"), (75, 75, 20, True, "constant"), (1536, 1200, 384, False, "reflect")):
        v = bhw.window(p, L, dtype=torch.float32)
        want = torch.stft(x, n_fft, hop, L, window=v, center=center, pad_mode=mode, onesided=False, return_complex=True)
        got = bhw.stft_iq_mixed(p, x, n_fft, hop, win_length=L, center=center, pad_mode=mode).transpose(-1, -2)
        assert got.shape == want.shape
        assert float((got - want).abs().max() / want.abs().max()) < 1e-5
        one = bhw.stft_iq_mixed(p, x[1], n_fft, hop, win_length=L, center=center, pad_mode=mode)
        assert one.dim() == 2 and torch.equal(torch.view_as_real(one), torch.view_as_real(got.transpose(-1, -2)[1]))


def test_two_sided_welch_through_stft_iq_mixed(torch):
    """welch_psd(stft_iq_mixed(detrend=True, center=False), scale, nfft=1000, onesided=False) on the signal, the parameters and the
    float64 reference of test_gpu_stft_iq.test_two_sided_welch_through_stft_iq restated at nfft = 1000, within twice the error of
    bhw.welch on its default route, library and table."""
    p = B.make_params(B.WIN_BH4, 14, 24)
    rng = np.random.default_rng(21)
    T, L, nov, nfft = 20000, 300, 100, 1000
    xh = (rng.standard_normal(T) + 1j * rng.standard_normal(T) + (0.3 - 0.2j)).astype(np.complex64)
    v = _v(p, L).astype(np.float64)
    hop = L - nov
    F = (T - nov) // hop
    seg = xh.astype(np.complex128)[np.arange(F)[:, None] * hop + np.arange(L)[None, :]]
    seg = seg - seg.mean(axis=-1, keepdims=True)
    Yr = np.fft.fft(seg * v, n=nfft, axis=-1)
    ref = (np.abs(Yr) ** 2).mean(axis=0) / (4.0 * (v * v).sum())
    x = torch.from_numpy(xh).cuda()
    base = _rel_err(bhw.welch(p, x, 4.0, length=L, noverlap=nov, nfft=nfft)[1].cpu().numpy(), ref)
    sums = bhw.window_sums(p, L, f32=True)
    with bhw.ResidentTable(p) as tab:
        for src in (bhw, tab):
            Y = src.stft_iq_mixed(p, x, nfft, hop, win_length=L, center=False, detrend=True)
            assert tuple(Y.shape) == (F, nfft)
            P = bhw.welch_psd(Y, B.welch_scale(sums, F, 4.0, "density"), nfft=nfft, onesided=False)
            assert P.shape == (nfft,)
            err = _rel_err(P.cpu().numpy(), ref)
            print(f"two-sided welch through stft_iq_mixed ({'table' if src is tab else 'library'}): fused {err:.3e}, bhw.welch default route "
                  f"{base:.3e}, ratio {err / base:.3f}")
            assert err <= 2.0 * base, (err, base)
        torch.cuda.synchronize()


def test_graph_capture_with_no_warm_call(torch):
    """All four forms -- spectrum and power, library and table -- captured on their first call, replayed once on new samples, equal to
    the eager results."""
    p = B.make_params(B.WIN_BH5, 13, 32)                               # a setup no other test of this module has used
    L, nfft, hop, T, nb = 400, 480, 160, 24000, 4
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.view_as_complex(torch.randn((nb, T, 2), device="cuda", generator=g)) + (5.0 - 1.0j)
    kw = dict(win_length=L, center=False, detrend=True)
    with bhw.ResidentTable(p) as tab:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                outs = [bhw.stft_iq_mixed(p, x, nfft, hop, **kw), bhw.spectrogram_iq_mixed(p, x, nfft, hop, fftshift=True, **kw),
                        tab.stft_iq_mixed(p, x, nfft, hop, **kw), tab.spectrogram_iq_mixed(p, x, nfft, hop, fftshift=True, **kw)]
        torch.cuda.current_stream().wait_stream(s)
        x.copy_(torch.view_as_complex(torch.randn((nb, T, 2), device="cuda", generator=g)) * 3.0 - 2.0)
        for o in outs:
            o.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        eager = [bhw.stft_iq_mixed(p, x, nfft, hop, **kw), bhw.spectrogram_iq_mixed(p, x, nfft, hop, fftshift=True, **kw),
                 tab.stft_iq_mixed(p, x, nfft, hop, **kw), tab.spectrogram_iq_mixed(p, x, nfft, hop, fftshift=True, **kw)]
        torch.cuda.synchronize()
        for o, e in zip(outs, eager):
            assert o.dtype == e.dtype and np.array_equal(_bits(torch, o), _bits(torch, e))
        assert np.array_equal(_bits(torch, outs[0]), _bits(torch, outs[2])) and bool((outs[1] > 0).all())


def test_python_errors(torch):
    p = B.make_params(B.WIN_BH7, 16, 32)
    x = torch.zeros((2, 4000), device="cuda")
    xc = torch.zeros((2, 4000), dtype=torch.complex64, device="cuda")
    with bhw.ResidentTable(p) as tab:
        for src in (bhw, tab):
            for fn, good, other in ((src.stft_iq_mixed, torch.complex64, torch.float32), (src.spectrogram_iq_mixed, torch.float32, torch.complex64)):
                with pytest.raises(ValueError, match="complex64"):
                    fn(p, x, 100, 16)
                with pytest.raises(ValueError, match="complex64"):
                    fn(p, xc.to(torch.complex128), 100, 16)
                with pytest.raises(ValueError, match="stft_iq"):
                    fn(p, xc, 64, 16)
                for n in (2048, 4096):
                    with pytest.raises(ValueError, match="power of two"):
                        fn(p, xc, n, 16)
                for n in (17, 28, 2160):
                    with pytest.raises(ValueError, match=r"2\^a·3\^b·5\^c in 16..2047"):
                        fn(p, xc, n, 16)
                with pytest.raises(ValueError, match="center=False"):
                    fn(p, xc, 100, 16, detrend=True)
                with pytest.raises(ValueError, match="out must be"):
                    fn(p, xc, 100, 16, out=torch.zeros((2, 251, 100), dtype=other, device="cuda"))
                with pytest.raises(ValueError, match="out must be"):
                    fn(p, xc, 100, 16, out=torch.zeros((2, 251, 51), dtype=good, device="cuda"))
                with pytest.raises(ValueError, match="CUDA tensor"):
                    fn(p, xc.cpu(), 100, 16)
                assert tuple(fn(p, xc, 100, 16, out=torch.zeros((2, 251, 100), dtype=good, device="cuda")).shape) == (2, 251, 100)
        # the four existing fronts keep refusing what they refused, in their words
        for fn in (bhw.stft_iq, bhw.spectrogram_iq):
            with pytest.raises(ValueError, match="power of two in 16..2048"):
                fn(p, xc, 100, 16)
        for fn in (bhw.stft_mixed, bhw.spectrogram_mixed):
            with pytest.raises(ValueError, match="real float32"):
                fn(p, xc, 100, 16)
            with pytest.raises(ValueError, match="even"):
                fn(p, x, 75, 16)
        torch.cuda.synchronize()
