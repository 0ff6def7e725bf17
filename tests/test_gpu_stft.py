"""Batched, centred STFT framing and overlap-add on the GPU (bhw_stft_frames_f32_* / bhw_istft_ola_f32_*): the frames bit for bit
against NumPy float32 pad -> unfold -> * v over window setups, both pad modes, center on and off, L = n_fft and L < n_fft, hops below,
at and above L, one and two channels, batches and short signals, with IEEE special values; the untouched gaps of y_stride and
y_batch_stride; library and from-table results identical; the identity with apply_frames at B = 1, pad = 0, col0 = 0, n_fft = L; the
overlap-add bit for bit against a NumPy binary64 ascending-order reference, with and without normalisation and with a length past the
extent; torch.stft / torch.istft with bhw.window(float32); graph capture; the Python errors."""
import ctypes

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

pytestmark = pytest.mark.gpu

SPECIAL = np.array([0.0, -0.0, 1e-40, -3e-42, 1.5e-45, np.inf, -np.inf, np.nan, 3e38, -2e38, 1.0, -1.0], dtype=np.float32)
SETUPS = [(B.WIN_BH7, 12, 32, {}), (B.WIN_HANN, 10, 16, {}), (B.WIN_BH4, 14, 24, {"model": B.MODEL_VHDL, "combine": B.COMBINE_VHDL}),
          (B.WIN_HAMMING, 9, 24, {"model": B.MODEL_CPP}), (B.WIN_BH5, 16, 32, {})]
# (n_fft, L, hop, center, pad_mode, C, batch, T)
FRAMINGS = [(64, 64, 16, True, "reflect", 1, 3, 200), (64, 49, 13, True, "constant", 2, 3, 150), (64, 49, 64, False, "reflect", 1, 1, 300),
            (32, 32, 1, True, "reflect", 2, 64, 40), (48, 40, 60, True, "constant", 1, 3, 100), (64, 64, 16, True, "constant", 1, 3, 20),
            (64, 61, 40, True, "reflect", 2, 2, 33), (100, 77, 77, True, "reflect", 1, 64, 90)]


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


def _same(a, b):
    """Bit-equal float32 arrays, NaN positions compared instead of NaN payloads."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def _signal(rng, shape, special=True):
    x = (rng.standard_normal(shape) * 1000).astype(np.float32)
    if special:
        flat = x.reshape(-1)
        idx = rng.choice(flat.size, size=min(flat.size, 3 * len(SPECIAL)), replace=False)
        flat[idx] = np.resize(SPECIAL, len(idx))
    return x


def _frames_ref(x, v, n_fft, hop, col0, pad, mode):
    """x (B, T, C) float32 -> (B, frames, n_fft, C): pad, unfold, window columns times v, +0.0 elsewhere."""
    xp = np.pad(x, ((0, 0), (pad, pad), (0, 0)), mode=mode)
    frames = 1 + (xp.shape[1] - n_fft) // hop
    idx = np.arange(frames)[:, None] * hop + np.arange(n_fft)[None, :]
    y = np.zeros((x.shape[0], frames, n_fft, x.shape[2]), dtype=np.float32)
    L = len(v)
    y[:, :, col0:col0 + L, :] = xp[:, idx[:, col0:col0 + L], :] * v[None, None, :, None]
    return y


def _ola_ref(y, v, hop, col0, pad, T, normalize):
    """y (B, frames, n_fft, C) -> (B, T, C): binary64 sums over ascending frames, rounded once."""
    nb, frames, _, C = y.shape
    L = len(v)
    S = np.zeros((nb, T, C))
    E = np.zeros(T)
    vd = v.astype(np.float64)
    for f in range(frames):                                   # ascending f: each output's sum in ascending frame order
        t = f * hop + col0 + np.arange(L) - pad               # the outputs of window columns k
        ok = (t >= 0) & (t < T)
        S[:, t[ok], :] += y[:, f, col0 + np.arange(L)[ok], :].astype(np.float64) * vd[ok][None, :, None]
        E[t[ok]] += vd[ok] * vd[ok]
    if not normalize:
        return S.astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(E[None, :, None] > 0, S / np.where(E > 0, E, 1.0)[None, :, None], 0.0).astype(np.float32)


def _to_torch(torch, x, C):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return torch.view_as_complex(t) if C == 2 else t[..., 0]


def _to_np(torch, t, C):
    return (torch.view_as_real(t) if C == 2 else t[..., None]).cpu().numpy()


@pytest.mark.parametrize("case", range(len(FRAMINGS)))
def test_frames_bit_for_bit_against_pad_unfold_multiply(torch, case):
    n_fft, L, hop, center, mode, C, nb, T = FRAMINGS[case]
    p = _params(case)
    rng = np.random.default_rng(100 + case)
    x = _signal(rng, (nb, T, C))
    pad = n_fft // 2 if center else 0
    ref = _frames_ref(x, _v(p, L), n_fft, hop, (n_fft - L) // 2, pad, mode)
    xt = _to_torch(torch, x, C)
    y_lib = bhw.stft_frames(p, xt, n_fft, hop, win_length=L, center=center, pad_mode=mode)
    with bhw.ResidentTable(p) as tab:
        y_tab = tab.stft_frames(p, xt, n_fft, hop, win_length=L, center=center, pad_mode=mode)
    torch.cuda.synchronize()
    a, b = _to_np(torch, y_lib, C), _to_np(torch, y_tab, C)
    assert _same(a, ref), case
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    col0 = (n_fft - L) // 2
    outside = np.concatenate([a[:, :, :col0], a[:, :, col0 + L:]], axis=2)
    assert not outside.size or (not np.isnan(outside).any() and np.all(outside.view(np.uint32) == 0))   # exactly +0.0
    if nb == 1:                                                    # 1-D input: (frames, n_fft)
        y1 = bhw.stft_frames(p, xt[0], n_fft, hop, win_length=L, center=center, pad_mode=mode)
        assert _same(_to_np(torch, y1, C), ref[0])


def test_frames_strided_batch_and_untouched_gaps(torch):
    p = _params(0)
    n_fft, L, hop, T, nb, C = 64, 50, 24, 130, 3, 2
    rng = np.random.default_rng(7)
    big = _signal(rng, (nb, T + 9, C))
    ref = _frames_ref(big[:, :T], _v(p, L), n_fft, hop, 7, 32, "reflect")
    frames = ref.shape[1]
    xt = _to_torch(torch, big, C)[:, :T]                           # x_stride = (T + 9) * C
    assert _same(_to_np(torch, bhw.stft_frames(p, xt, n_fft, hop, win_length=L), C), ref)
    # rows of y_stride > n_fft * C, signals y_batch_stride apart with a gap: the sentinels stay
    ys, ybs = n_fft * C + 6, (frames * (n_fft * C + 6)) + 10
    sent = np.float32(-123.25)
    buf = torch.full((nb * ybs,), float(sent), device="cuda")
    s = B.make_stft(nb, T, frames, hop, n_fft, col0=7, pad=32, pad_mode=B.PAD_REFLECT, channels=C, shift=p.dat_width - 1,
                    x_stride=(T + 9) * C, y_stride=ys, y_batch_stride=ybs)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    xs = torch.view_as_real(_to_torch(torch, big, C)).contiguous()
    B.check(B.lib().bhw_stft_frames_f32_device(ctypes.byref(p), L, torch.cuda.current_device(), st, ctypes.byref(s),
                                               ctypes.c_void_p(xs.data_ptr()), ctypes.c_void_p(buf.data_ptr())))
    got = buf.cpu().numpy()
    for b in range(nb):
        sig = got[b * ybs:(b + 1) * ybs]
        rows = sig[:frames * ys].reshape(frames, ys)
        assert _same(rows[:, :n_fft * C].reshape(frames, n_fft, C), ref[b])
        assert np.all(rows[:, n_fft * C:] == sent) and np.all(sig[frames * ys:] == sent)


def test_frames_equal_apply_frames_at_no_padding(torch):
    p = _params(0)
    N, hop, frames = 1 << 12, 1 << 10, 9
    x = torch.from_numpy(_signal(np.random.default_rng(3), ((frames - 1) * hop + N,))).cuda()
    a = bhw.stft_frames(p, x, N, hop, center=False)
    b = bhw.apply_frames(p, x, hop)
    torch.cuda.synchronize()
    assert a.shape == b.shape and _same(a.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("case", range(len(FRAMINGS)))
@pytest.mark.parametrize("normalize", [False, True])
def test_overlap_add_bit_for_bit_against_ascending_binary64(torch, case, normalize):
    n_fft, L, hop, center, _, C, nb, T = FRAMINGS[case]
    if not center and L < n_fft:
        center = True
    p = _params(case + 1)
    pad = n_fft // 2 if center else 0
    rng = np.random.default_rng(200 + case)
    frames = 1 + max(T + 2 * pad - n_fft, 0) // hop
    y = _signal(rng, (nb, frames, n_fft, C), special=False)
    v = _v(p, L)
    yt = _to_torch(torch, y, C)
    default_len = n_fft + hop * (frames - 1) - 2 * pad
    end = (frames - 1) * hop + (n_fft - L) // 2 + L - pad            # past the last window column
    for length in (None, end + 37):
        T_out = default_len if length is None else length
        ref = _ola_ref(y, v, hop, (n_fft - L) // 2, pad, T_out, normalize)
        got = bhw.istft_overlap_add(p, yt, n_fft, hop, win_length=L, center=center, length=length, normalize=normalize)
        with bhw.ResidentTable(p) as tab:
            got_t = tab.istft_overlap_add(p, yt, n_fft, hop, win_length=L, center=center, length=length, normalize=normalize)
        torch.cuda.synchronize()
        a = _to_np(torch, got, C)
        assert _same(a, ref), (case, length)
        assert torch.equal(got, got_t)
        if length is not None:                                     # empty sums: +0.0
            assert np.all(a[:, end:].view(np.uint32) == 0)


def test_broadcast_strided_and_conjugated_inputs_read_as_their_values(torch):
    p = _params(1)
    n_fft, L, hop, T, nb = 64, 49, 16, 300, 4
    g = torch.Generator(device="cuda").manual_seed(11)
    for dtype in (torch.float32, torch.complex64):
        x1 = torch.randn(T, dtype=dtype, device="cuda", generator=g)
        xe = x1.expand(nb, T)                                       # stride (0, 1): one signal's storage for every row
        assert torch.equal(bhw.stft_frames(p, xe, n_fft, hop, win_length=L), bhw.stft_frames(p, xe.contiguous(), n_fft, hop, win_length=L))
        xt = torch.randn(T, nb, dtype=dtype, device="cuda", generator=g).t()     # stride (1, nb)
        assert torch.equal(bhw.stft_frames(p, xt, n_fft, hop, win_length=L), bhw.stft_frames(p, xt.contiguous(), n_fft, hop, win_length=L))
        y = bhw.stft_frames(p, xt.contiguous(), n_fft, hop, win_length=L)
        ye = y[0].expand(nb, *y.shape[1:])                           # batch stride 0
        assert torch.equal(bhw.istft_overlap_add(p, ye, n_fft, hop, win_length=L), bhw.istft_overlap_add(p, ye.contiguous(), n_fft, hop, win_length=L))
        yr = y[:, :1].expand(nb, y.shape[1], n_fft)                  # row stride 0
        assert torch.equal(bhw.istft_overlap_add(p, yr, n_fft, hop, win_length=L), bhw.istft_overlap_add(p, yr.contiguous(), n_fft, hop, win_length=L))
        if dtype == torch.complex64:                                 # a lazy conjugate is resolved, not read as x
            xc = xt.contiguous().conj()
            assert xc.is_conj()
            assert torch.equal(bhw.stft_frames(p, xc, n_fft, hop, win_length=L), bhw.stft_frames(p, xc.resolve_conj(), n_fft, hop, win_length=L))
            assert torch.equal(bhw.istft_overlap_add(p, y.conj(), n_fft, hop, win_length=L),
                               bhw.istft_overlap_add(p, y.conj().resolve_conj(), n_fft, hop, win_length=L))
    # out takes the shape the call returns, unbatched included
    x1 = torch.randn(T, device="cuda", generator=g)
    want = bhw.stft_frames(p, x1, n_fft, hop)
    out = torch.empty_like(want)
    assert bhw.stft_frames(p, x1, n_fft, hop, out=out) is out and torch.equal(out, want)
    wantx = bhw.istft_overlap_add(p, want, n_fft, hop)
    outx = torch.empty_like(wantx)
    assert wantx.dim() == 1 and bhw.istft_overlap_add(p, want, n_fft, hop, out=outx) is outx and torch.equal(outx, wantx)


def test_odd_strides_take_the_four_byte_pair_path(torch):
    """Two channels with an odd x_stride and y_batch_stride: the 8-byte pair access is not aligned, the kernels move 4-byte halves."""
    p = _params(0)
    n_fft, L, hop, T, nb, C = 64, 50, 24, 130, 3, 2
    col0, pad = (n_fft - L) // 2, n_fft // 2
    rng = np.random.default_rng(21)
    x = _signal(rng, (nb, T, C))
    ref = _frames_ref(x, _v(p, L), n_fft, hop, col0, pad, "reflect")
    frames = ref.shape[1]
    xs, ybs = T * C + 1, frames * n_fft * C + 1
    xflat = np.zeros((nb - 1) * xs + T * C, dtype=np.float32)
    for b in range(nb):
        xflat[b * xs:b * xs + T * C] = x[b].reshape(-1)
    xd = torch.from_numpy(xflat).cuda()
    yd = torch.full(((nb - 1) * ybs + frames * n_fft * C,), 5.0, device="cuda")
    s = B.make_stft(nb, T, frames, hop, n_fft, col0=col0, pad=pad, pad_mode=B.PAD_REFLECT, channels=C, shift=p.dat_width - 1,
                    x_stride=xs, y_batch_stride=ybs)
    st, dev = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), torch.cuda.current_device()
    assert "channels" in B.describe_stft(p, L, s)
    with bhw.ResidentTable(p) as tab:
        for call in (lambda: B.lib().bhw_stft_frames_f32_device(ctypes.byref(p), L, dev, st, ctypes.byref(s), ctypes.c_void_p(xd.data_ptr()),
                                                                 ctypes.c_void_p(yd.data_ptr())),
                     lambda: B.lib().bhw_stft_frames_f32_from_table(tab.handle, ctypes.byref(p), L, st, ctypes.byref(s),
                                                                     ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(yd.data_ptr()))):
            B.check(call())
            got = yd.cpu().numpy()
            for b in range(nb):
                assert _same(got[b * ybs:b * ybs + frames * n_fft * C].reshape(frames, n_fft, C), ref[b])
        # the overlap-add of the same rows into signals an odd stride apart
        yy = _signal(rng, (nb, frames, n_fft, C), special=False)
        yflat = np.zeros((nb - 1) * ybs + frames * n_fft * C, dtype=np.float32)
        for b in range(nb):
            yflat[b * ybs:b * ybs + frames * n_fft * C] = yy[b].reshape(-1)
        yd = torch.from_numpy(yflat).cuda()
        xo = torch.full(((nb - 1) * xs + T * C,), 5.0, device="cuda")
        si = B.make_stft(nb, T, frames, hop, n_fft, col0=col0, pad=pad, channels=C, shift=p.dat_width - 1, x_stride=xs,
                         y_batch_stride=ybs)
        want = _ola_ref(yy, _v(p, L), hop, col0, pad, T, True)
        for call in (lambda: B.lib().bhw_istft_ola_f32_device(ctypes.byref(p), L, dev, st, ctypes.byref(si), 1, ctypes.c_void_p(yd.data_ptr()),
                                                               ctypes.c_void_p(xo.data_ptr())),
                     lambda: B.lib().bhw_istft_ola_f32_from_table(tab.handle, ctypes.byref(p), L, st, ctypes.byref(si), 1,
                                                                   ctypes.c_void_p(yd.data_ptr()), ctypes.c_void_p(xo.data_ptr()))):
            B.check(call())
            got = xo.cpu().numpy()
            for b in range(nb):
                assert _same(got[b * xs:b * xs + T * C].reshape(T, C), want[b])
            assert np.all(got[[b * xs + T * C for b in range(nb - 1)]] == 5.0)          # the gaps between signals stay


def test_overlap_add_batch_beyond_one_grid_z_launch(torch):
    """65 539 signals: the overlap-add launches grid z in chunks of 65 535."""
    p = _params(1)
    n_fft, L, hop, T, nb = 8, 8, 4, 16, 65535 + 4
    frames = 1 + (T + n_fft - n_fft) // hop
    y = _signal(np.random.default_rng(31), (nb, frames, n_fft, 1), special=False)
    got = bhw.istft_overlap_add(p, torch.from_numpy(y[..., 0]).cuda(), n_fft, hop, length=T)
    assert "65539 signals (grid z 65535)" in B.describe_stft(p, L, B.make_stft(nb, T, frames, hop, n_fft, pad=n_fft // 2), inverse=True,
                                                               normalize=True)
    assert _same(got.cpu().numpy()[..., None], _ola_ref(y, _v(p, L), hop, 0, n_fft // 2, T, True))


def test_from_table_calls_refuse_another_key(torch):
    p = _params(0)
    other = B.make_params(B.WIN_BH7, p.phi_width + 1, p.dat_width)
    x = torch.randn((2, 1000), device="cuda")
    with bhw.ResidentTable(p) as tab:
        y = tab.stft_frames(p, x, 64, 16)
        with pytest.raises(B.BhwError, match="phi_width"):
            tab.stft_frames(other, x, 64, 16)
        with pytest.raises(B.BhwError, match="phi_width"):
            tab.istft_overlap_add(other, y, 64, 16)


def test_against_torch_stft_and_istft(torch):
    p = B.make_params(B.WIN_BH4, 24, 32)
    n_fft, L, hop, T = 512, 400, 160, 16000
    wv = bhw.window(p, L, dtype=torch.float32)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((3, T), device="cuda", generator=g)
    xc = torch.randn((2, T), dtype=torch.complex64, device="cuda", generator=g)
    for mode in ("reflect", "constant"):
        spec = torch.fft.rfft(bhw.stft_frames(p, x, n_fft, hop, win_length=L, pad_mode=mode)).transpose(-1, -2)
        ref = torch.stft(x, n_fft, hop, L, window=wv, center=True, pad_mode=mode, return_complex=True)
        assert torch.allclose(spec, ref, rtol=1e-5, atol=1e-5 * ref.abs().max().item())
        specc = torch.fft.fft(bhw.stft_frames(p, xc, n_fft, hop, win_length=L, pad_mode=mode)).transpose(-1, -2)
        refc = torch.stft(xc, n_fft, hop, L, window=wv, center=True, pad_mode=mode, return_complex=True)
        assert torch.allclose(specc, refc, rtol=1e-5, atol=1e-5 * refc.abs().max().item())
    spec = torch.stft(x, n_fft, hop, L, window=wv, center=True, return_complex=True)
    y = torch.fft.irfft(spec.transpose(-1, -2), n=n_fft)
    xr = bhw.istft_overlap_add(p, y, n_fft, hop, win_length=L, length=T)
    ref = torch.istft(spec, n_fft, hop, L, window=wv, center=True, length=T)
    assert xr.shape == ref.shape == x.shape
    assert torch.allclose(xr, ref, rtol=1e-5, atol=1e-5 * ref.abs().max().item())
    assert torch.allclose(xr, x, rtol=1e-4, atol=1e-4 * x.abs().max().item())


def test_graph_capture_of_both_calls(torch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    n_fft, L, hop, T, nb = 512, 400, 160, 4000, 4
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn((nb, T), device="cuda", generator=g)
    with bhw.ResidentTable(p) as tab:
        want_f = bhw.stft_frames(p, x, n_fft, hop, win_length=L)
        want_x = bhw.istft_overlap_add(p, want_f, n_fft, hop, win_length=L, length=T)
        yl, yt = torch.empty_like(want_f), torch.empty_like(want_f)
        xl, xt = torch.empty_like(want_x), torch.empty_like(want_x)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                bhw.stft_frames(p, x, n_fft, hop, win_length=L, out=yl)
                tab.stft_frames(p, x, n_fft, hop, win_length=L, out=yt)
                bhw.istft_overlap_add(p, yl, n_fft, hop, win_length=L, length=T, out=xl)
                tab.istft_overlap_add(p, yt, n_fft, hop, win_length=L, length=T, out=xt)
        torch.cuda.current_stream().wait_stream(s)
        for t in (yl, yt, xl, xt):
            t.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(yl, want_f) and torch.equal(yt, want_f)
        assert torch.equal(xl, want_x) and torch.equal(xt, want_x)


def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    x = torch.zeros((2, 100), device="cuda")
    with pytest.raises(ValueError, match="reflect"):
        bhw.stft_frames(p, x[:, :64], 128, 32)                    # pad 64 not below T = 64
    bhw.stft_frames(p, x[:, :64], 128, 32, pad_mode="constant")   # constant padding has no such rule
    with pytest.raises(ValueError, match="win_length"):
        bhw.stft_frames(p, x, 64, 16, win_length=65)
    with pytest.raises(ValueError, match="zero frames"):
        bhw.stft_frames(p, x[:, :10], 64, 16, center=False)
    with pytest.raises(ValueError, match="pad_mode"):
        bhw.stft_frames(p, x, 64, 16, pad_mode="circular")
    y = torch.zeros((2, 5, 64), device="cuda")
    with pytest.raises(ValueError, match="center=False"):
        bhw.istft_overlap_add(p, y, 64, 16, win_length=48, center=False)
    with pytest.raises(ValueError, match="win_length"):
        bhw.istft_overlap_add(p, y, 64, 16, win_length=80)
    with pytest.raises(ValueError, match="zero frames"):
        bhw.istft_overlap_add(p, y[:, :0], 64, 16)
    with pytest.raises(ValueError):
        bhw.stft_frames(p, x.to(torch.int32), 64, 16)
