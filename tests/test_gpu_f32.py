"""Float32 frame apply and overlap-add on the GPU (bhw_apply_frames_f32_* / bhw_overlap_add_f32_*): the frames bit for bit against
NumPy float32 (x_frames * v) over the models, combine rules, term counts, widths, lengths, channels, hops, strides and IEEE special
values; the overlap-add bit for bit against a NumPy float64 reference that sums the frames in ascending order (with a case that tells
the orders apart), with and without the envelope division; the STFT round trip through torch.fft; torch.stft with bhw.window(float32);
graph capture of the from-table and library calls; the Python errors."""
import ctypes

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

pytestmark = pytest.mark.gpu

WIN_OF_TERMS = {2: B.WIN_HAMMING, 3: B.WIN_BH3, 4: B.WIN_BH4, 5: B.WIN_BH5, 7: B.WIN_BH7}
SPECIAL = np.array([0.0, -0.0, 1e-40, -3e-42, 1.5e-45, np.inf, -np.inf, np.nan, 3e38, -2e38, 1.0, -1.0], dtype=np.float32)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _valid(p):
    return B.lib().bhw_params_validate(ctypes.byref(p)) == 0


def _v(p, L, shift=None):
    """v[k] = fl32(w[k]) * 2^-shift in NumPy, from the int32 window of the int32 calls."""
    shift = p.dat_width - 1 if shift is None else shift
    w = bhw.window(p, L).cpu().numpy()
    return np.ldexp(w.astype(np.float32), -shift).astype(np.float32)


def _same(a, b):
    """Bit-equal float32 arrays, NaN positions compared instead of NaN payloads."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def _signal(rng, n, special=True):
    x = (rng.standard_normal(n) * 1000).astype(np.float32)
    if special:
        idx = rng.choice(n, size=min(n, 4 * len(SPECIAL)), replace=False)
        x[idx] = np.resize(SPECIAL, len(idx))
    return x


def _frames_ref(x, v, hop, frames, C):
    L = len(v)
    xs = x.reshape(-1, C)
    idx = np.arange(frames)[:, None] * hop + np.arange(L)[None, :]
    return xs[idx] * v[None, :, None]                                 # float32 x float32: one rounding


def _ola_ref(yf, v, hop, t0, count, normalize, descending=False):
    """yf: (frames, L, C) float32.  binary64 sums over the frames in ascending (or descending) order, vectorised over t."""
    frames, L, C = yf.shape
    t = np.arange(t0, t0 + count)
    S = np.zeros((count, C))
    E = np.zeros(count)
    v64 = v.astype(np.float64)
    order = range(frames - 1, -1, -1) if descending else range(frames)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in order:
            k = t - f * hop
            m = (k >= 0) & (k < L)
            if not m.any():
                continue
            S[m] += yf[f, k[m], :].astype(np.float64) * v64[k[m]][:, None]
            E[m] += v64[k[m]] * v64[k[m]]
        if not normalize:
            return S.astype(np.float32)
        out = np.zeros((count, C))
        np.divide(S, E[:, None], out=out, where=(E > 0)[:, None])
    return out.astype(np.float32)


def _params():
    """The model x combine x term count x width lattice (valid configurations only)."""
    out = []
    for model in (B.MODEL_HLS, B.MODEL_CPP, B.MODEL_VHDL):
        for combine in (B.COMBINE_HLS, B.COMBINE_VHDL):
            for K in (2, 3, 4, 5, 7):
                for W in (16, 24, 32):
                    p = B.make_params(WIN_OF_TERMS[K], 12, W, model=model, combine=combine, validate=False)
                    if _valid(p):
                        out.append(p)
    return out


def test_frames_bit_exact_over_the_lattice(torch):
    rng = np.random.default_rng(1)
    P = 12
    lengths = (1 << P, 400, 1023, (1 << P) - 1)
    n = 0
    for i, p in enumerate(_params()):
        L = lengths[i % len(lengths)]
        C = 1 + (i // len(lengths)) % 2
        hop = (L // 3, L, L + 7)[i % 3]
        frames = 5
        shift = 0 if i % 7 == 3 else None                       # shift 0: |v| up to 2^31, the 3e38 samples overflow to inf
        v = _v(p, L, shift)
        x_np = _signal(rng, ((frames - 1) * hop + L) * C)
        want = _frames_ref(x_np, v, hop, frames, C)
        x = torch.from_numpy(x_np).cuda()
        got = bhw.apply_frames(p, x, hop, channels=C, shift=shift, length=L)
        assert got.dtype == torch.float32 and _same(got.cpu().numpy().reshape(want.shape), want), (i, L, C, hop)
        with bhw.ResidentTable(p) as t:
            got = t.apply_frames(p, x, hop, channels=C, shift=shift, length=L)
            assert _same(got.cpu().numpy().reshape(want.shape), want), (i, L, C, hop, "table")
        n += 1
    assert n >= 60


def test_frames_padding_misalignment_and_window(torch):
    rng = np.random.default_rng(2)
    p = B.make_params(B.WIN_BH4, 10, 24)
    N, hop, frames = 1024, 256, 9
    v = _v(p, N)
    # apply_frames(ones) is the float32 window itself, in both routes and at L = 400
    ones = torch.ones(N, dtype=torch.float32, device="cuda")
    wv = bhw.window(p, N, dtype=torch.float32)
    assert wv.dtype == torch.float32 and _same(wv.cpu().numpy(), v)
    assert torch.equal(bhw.apply_frames(p, ones, N)[0], wv)
    with bhw.ResidentTable(p) as t:
        assert torch.equal(t.apply_frames(p, ones, N)[0], wv)
    assert torch.equal(bhw.apply_frames(p, ones[:400], 400, length=400)[0], bhw.window(p, 400, dtype=torch.float32))
    for shift in (0, 5, 31, 62):
        assert _same(bhw.window(p, 401, sym=True, dtype=torch.float32, shift=shift).cpu().numpy(),
                     np.ldexp(bhw.window(p, 401, sym=True).cpu().numpy().astype(np.float32), -shift))
    for C in (1, 2):
        x_np = _signal(rng, ((frames - 1) * hop + N) * C + 1)
        # a padded y_stride whose padding stays untouched
        stride = N * C + 6
        out = torch.full((frames * stride,), 7.5, dtype=torch.float32, device="cuda")
        x = torch.from_numpy(x_np[:-1]).cuda()
        got = bhw.apply_frames(p, x, hop, channels=C, y_stride=stride, out=out).cpu().numpy()
        assert _same(got[:, :N * C].reshape(frames, N, C), _frames_ref(x_np[:-1], v, hop, frames, C))
        assert (got[:, N * C:] == 7.5).all()
        # a base 4 bytes off the 8-byte alignment: the two-access I/Q path
        buf = torch.from_numpy(x_np).cuda()
        xm = buf[1:]
        assert xm.data_ptr() % 8 == 4
        got = bhw.apply_frames(p, xm, hop, channels=C)
        assert _same(got.cpu().numpy().reshape(frames, N, C), _frames_ref(x_np[1:], v, hop, frames, C))


@pytest.mark.parametrize("L,P", [(1 << 10, 10), (400, 12)])
def test_overlap_add_bit_exact(torch, L, P):
    rng = np.random.default_rng(3)
    p = B.make_params(B.WIN_BH7, P, 32)
    v = _v(p, L)
    with bhw.ResidentTable(p) as t:
        for C in (1, 2):
            # pad 5: an odd stride for I/Q (two 4-byte accesses); pad 6: an even one (one 8-byte access per pair)
            for (hop, frames), pad in zip(((L // 4, 11), (L // 3 + 1, 7), (L, 4), (L + 9, 4)), (5, 6, 6, 5)):
                ext = (frames - 1) * hop + L
                rows = rng.standard_normal((frames, L * C + pad)).astype(np.float32)
                rows[:, L * C:] = np.nan                                # the padding is never read
                yf = rows[:, :L * C].reshape(frames, L, C)
                y = torch.from_numpy(rows).cuda()
                for t0, count in ((0, ext), (ext // 3, ext // 3 + 1), (ext - 5, 5)):
                    for normalize in (False, True):
                        want = _ola_ref(yf, v, hop, t0, count, normalize)
                        kw = dict(channels=C, y_stride=L * C + pad, t0=t0, count=count, normalize=normalize,
                                  length=None if L == 1 << P else L)
                        got = bhw.overlap_add(p, y, hop, **kw).cpu().numpy()
                        assert _same(got.reshape(want.shape), want), (C, hop, t0, normalize)
                        got = t.overlap_add(p, y, hop, **kw).cpu().numpy()
                        assert _same(got.reshape(want.shape), want), (C, hop, t0, normalize, "table")
                if hop > L:                                             # the gaps between frames: +0.0
                    got = bhw.overlap_add(p, y, hop, channels=C, y_stride=L * C + pad, normalize=True,
                                          length=None if L == 1 << P else L).cpu().numpy().reshape(ext, C)
                    gap = got[L:hop]
                    assert (gap == 0).all() and not np.signbit(gap).any()


def test_overlap_add_iq_pairs(torch):
    """Two channels with 8-byte aligned bases and an even row stride (y_stride None: 2L): the one-access-per-pair path, both routes,
    with and without the division, power-of-two and L = 400.  The channels hold different data, so a swapped pair shows."""
    rng = np.random.default_rng(6)
    for P, L, hop, frames in ((10, 1 << 10, 256, 9), (12, 400, 100, 13)):
        p = B.make_params(B.WIN_BH4, P, 24)
        v = _v(p, L)
        length = None if L == 1 << P else L
        yf = rng.standard_normal((frames, L, 2)).astype(np.float32)
        yf[..., 1] *= 1000.0
        y = torch.from_numpy(yf).cuda()
        assert y.data_ptr() % 8 == 0
        ext = (frames - 1) * hop + L
        with bhw.ResidentTable(p) as t:
            for normalize in (False, True):
                want = _ola_ref(yf, v, hop, 0, ext, normalize)
                for call in (bhw.overlap_add, t.overlap_add):
                    got = call(p, y, hop, channels=2, normalize=normalize, length=length)
                    assert got.shape == (ext, 2) and got.data_ptr() % 8 == 0
                    assert _same(got.cpu().numpy(), want), (P, normalize, call)


def test_overlap_add_sums_frames_in_ascending_order(torch):
    """Products of about 1, +2^100 v v' and exactly -(2^100 v v') at one t, then 0: summed in ascending frame order the small one is
    absorbed and the result is +0; summed in descending order it survives.  The references must differ, and the GPU must agree with
    the ascending one."""
    p = B.make_params(B.WIN_BH4, 10, 24)
    N = 1 << 10
    hop, frames = N // 4, 4
    v = _v(p, N)
    c = np.float32(2.0 ** 100)
    k = np.arange(N)
    y = np.zeros((frames, N), dtype=np.float32)
    y[0] = 1.0
    y[1] = c * v[np.clip(k - hop, 0, N - 1)]                       # frame 1 at t: c * v[t - 2 hop], the coefficient frame 2 uses
    y[2] = -c * v[np.clip(k + hop, 0, N - 1)]                      # frame 2 at t: -c * v[t - hop]
    yf = y.reshape(frames, N, 1)
    ext = (frames - 1) * hop + N
    asc = _ola_ref(yf, v, hop, 0, ext, False)
    desc = _ola_ref(yf, v, hop, 0, ext, False, descending=True)
    assert not _same(asc, desc), "the case must tell the orders apart"
    assert (asc[3 * hop:N] != desc[3 * hop:N]).sum() > N // 8
    got = bhw.overlap_add(p, torch.from_numpy(y).cuda(), hop).cpu().numpy()
    assert _same(got.reshape(asc.shape), asc)
    with bhw.ResidentTable(p) as t:
        assert _same(t.overlap_add(p, torch.from_numpy(y).cuda(), hop).cpu().numpy().reshape(asc.shape), asc)
    asc_n = _ola_ref(yf, v, hop, 0, ext, True)
    got = bhw.overlap_add(p, torch.from_numpy(y).cuda(), hop, normalize=True).cpu().numpy()
    assert _same(got.reshape(asc_n.shape), asc_n)


@pytest.mark.parametrize("win,P,L,hop", [(B.WIN_BH4, 10, 1 << 10, 256), (B.WIN_HANN, 12, 400, 100)])
def test_stft_round_trip_and_torch_stft(torch, win, P, L, hop):
    rng = np.random.default_rng(4)
    p = B.make_params(win, P, 24 if win == B.WIN_BH4 else 16)
    length = None if L == 1 << P else L
    x_np = rng.standard_normal(40 * hop + L).astype(np.float32)
    x = torch.from_numpy(x_np).cuda()
    fr = bhw.apply_frames(p, x, hop, length=length)
    spec = torch.fft.rfft(fr, dim=-1)
    back = torch.fft.irfft(spec, n=L, dim=-1).contiguous()
    xr = bhw.overlap_add(p, back, hop, normalize=True, length=length)
    inner = slice(L, len(x_np) - L)
    err = torch.linalg.norm(xr[inner] - x[inner]) / torch.linalg.norm(x[inner])
    assert err.item() <= 1e-6, err.item()
    # torch.stft with the window the kernels apply
    wv = bhw.window(p, L, dtype=torch.float32)
    ref = torch.stft(x, n_fft=L, hop_length=hop, window=wv, center=False, return_complex=True).T
    assert ref.shape == spec.shape
    assert torch.allclose(spec, ref, rtol=1e-5, atol=1e-5 * ref.abs().max().item())


def test_graph_capture(torch):
    p = B.make_params(B.WIN_BH7, 16, 32)
    L, hop, frames = 400, 160, 50
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((frames - 1) * hop + L).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.standard_normal((frames, L)).astype(np.float32)).cuda()
    with bhw.ResidentTable(p) as t:
        wf, wo = t.apply_frames(p, x, hop, length=L), t.overlap_add(p, y, hop, length=L, normalize=True)
        lf, lo = bhw.apply_frames(p, x, hop, length=L), bhw.overlap_add(p, y, hop, length=L)
        of, oo, olf, olo = (torch.zeros_like(a) for a in (wf, wo, lf, lo))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s):
            t.apply_frames(p, x, hop, out=of, length=L)
            t.overlap_add(p, y, hop, out=oo, length=L, normalize=True)
            bhw.apply_frames(p, x, hop, out=olf, length=L)             # library calls: no prepare, no scratch
            bhw.overlap_add(p, y, hop, out=olo, length=L)
        for _ in range(2):
            for a in (of, oo, olf, olo):
                a.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(of.view_as(wf), wf) and torch.equal(oo, wo) and torch.equal(olf.view_as(lf), lf) and torch.equal(olo, lo)


def test_python_errors(torch):
    p = B.make_params(B.WIN_BH4, 10, 24)
    x64 = torch.zeros(4096, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        bhw.apply_frames(p, x64, 256)
    with pytest.raises(ValueError):
        bhw.overlap_add(p, x64.view(4, 1024), 256)
    yi = torch.zeros((4, 1024), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        bhw.overlap_add(p, yi, 256, normalize=True)
    with bhw.ResidentTable(p) as t:
        with pytest.raises(ValueError):
            t.overlap_add(p, yi, 256, normalize=True)
    xf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        bhw.apply_frames(p, xf, 256, out=torch.zeros(13 * 1024, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        bhw.overlap_add(p, xf.view(4, 1024), 256, out=torch.zeros(4096, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        bhw.window(p, 1024, dtype=torch.float64)
    # int32 calls are unchanged: int32 in, int32 out
    assert bhw.apply_frames(p, torch.zeros(4096, dtype=torch.int32, device="cuda"), 256).dtype == torch.int32
    assert bhw.overlap_add(p, yi, 256).dtype == torch.int32
