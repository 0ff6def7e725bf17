"""The fused inverse mixed-radix FFT + overlap-add kernel on the GPU (bhw_istft_mfft_f32_* through bhw.istft_mixed and
ResidentTable.istft_mixed), in the manner of tests/test_gpu_istft_fft.py.

Accuracy is the gate, twice over: for every case of tests/istft_mfft_cases.py the reference is numpy in float64 (irfft of Y in
complex128, then the overlap-add contract with the float32 v), the metric the largest over the signals of |got - ref|_2 / |ref|_2, the
yardstick bhw.istft_overlap_add(torch.fft.irfft(Y, n=n_fft)) on the same GPU; the fused call is held to twice the yardstick's error AND
to 2^-24 * log2(n_fft).  The inverse FFT is not pinned bit for bit; everything around it is, and those properties are held word for
word, on n_fft 50 (M = 25 is odd: no self-mirrored bin, a lane without its last ring column) and 1200."""
import ctypes
import math

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import istft_mfft_cases as XC

pytestmark = pytest.mark.gpu

SENTINEL = 12345.5


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _v(p, L):
    w = bhw.window(p, L).cpu().numpy()
    return np.ldexp(w.astype(np.float32), -(p.dat_width - 1)).astype(np.float32)


def _spectra(nb, F, n_fft, seed=0, scale=100.0):
    """(B, F, K) complex64 noise with purely real bins 0 and n_fft / 2."""
    rng = np.random.default_rng(2400 + seed)
    K = n_fft // 2 + 1
    Y = ((rng.standard_normal((nb, F, K)) + 1j * rng.standard_normal((nb, F, K))) * scale).astype(np.complex64)
    Y[..., 0] = Y[..., 0].real
    Y[..., -1] = Y[..., -1].real
    return Y


def _ref64(Yh, v, n_fft, hop, col0, pad, T, normalize):
    """float64: irfft of every row, then S = sum r * v and E = sum v^2 over the frames reaching each output; (B, T)."""
    nb, F, _ = Yh.shape
    L = len(v)
    t0 = pad - col0
    vd = v.astype(np.float64)
    W = max(t0 + T, (F - 1) * hop + L)
    S, E = np.zeros((nb, W)), np.zeros(W)
    for f0 in range(0, F, 256):
        rows = np.fft.irfft(Yh[:, f0:f0 + 256].astype(np.complex128), n=n_fft, axis=-1)
        for i in range(rows.shape[1]):
            w = (f0 + i) * hop
            S[:, w:w + L] += rows[:, i, col0:col0 + L] * vd
            E[w:w + L] += vd * vd
    S, E = S[:, t0:t0 + T], E[t0:t0 + T]
    if not normalize:
        return S
    return np.where(E > 0, S / np.where(E > 0, E, 1.0), 0.0)


def _err(got, ref):
    """max over the signals of |got - ref|_2 / |ref|_2; a signal whose reference is zero must come out zero."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref)
    nr = np.sqrt((ref ** 2).sum(axis=-1))
    ne = np.sqrt(((got - ref) ** 2).sum(axis=-1))
    zero = nr == 0
    assert not (ne[zero] != 0).any(), "a signal whose reference is zero must come out zero"
    return float((ne[~zero] / nr[~zero]).max()) if (~zero).any() else 0.0


def _kw(c):
    return dict(win_length=c["L"], center=c["center"], length=XC.geometry(c)[4], normalize=c["normalize"])


def _raw_call(torch, p, c, Y, table=None):
    """The C call on the case's own descriptor (padded strides included): Y (B, F, K) complex64 on the GPU -> the x buffer (B, x_stride)
    and the Y buffer laid out by the strides, both filled with a sentinel first."""
    s, L, _, _, T = XC.desc(c)
    nb, F, K = Y.shape
    ys = (s.y_stride or 2 * K) // 2
    ybs = (s.y_batch_stride or F * ys * 2) // 2
    ybuf = torch.full((nb, ybs), complex(SENTINEL, -SENTINEL), dtype=torch.complex64, device="cuda")
    ybuf[:, :F * ys].view(nb, F, ys)[:, :, :K] = Y
    before = ybuf.clone()
    xs = s.x_stride or T
    xbuf = torch.full((nb, xs), SENTINEL, device="cuda")
    flags = B.OLA_NORMALIZE if c["normalize"] else 0
    dev = Y.device.index
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    tail = (ctypes.byref(s), flags, ctypes.c_void_p(ybuf.data_ptr()), ctypes.c_void_p(xbuf.data_ptr()))
    if table is None:
        B.check(B.lib().bhw_istft_mfft_f32_device(ctypes.byref(p), L, dev, stream, *tail))
    else:
        B.check(B.lib().bhw_istft_mfft_f32_from_table(table._live(), ctypes.byref(p), L, stream, *tail))
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(ybuf), torch.view_as_real(before)), "Y, its gaps included, is only read"
    return xbuf, T


def _call(torch, p, c, Y, table=None):
    """(B, T) float32 on the GPU: bhw.istft_mixed / ResidentTable.istft_mixed, or for a padded case the C call, the sentinels of the
    gaps checked."""
    if c.get("padded"):
        xbuf, T = _raw_call(torch, p, c, Y, table)
        assert bool((xbuf[:, T:] == SENTINEL).all()), "a gap of x was written"
        return xbuf[:, :T].contiguous()
    fn = bhw.istft_mixed if table is None else table.istft_mixed
    return fn(p, Y, c["n_fft"], c["hop"], **_kw(c))


def _bits(t):
    return t.contiguous().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("cid", XC.case_ids())
def test_accuracy_within_twice_the_two_step_route_and_the_float32_cap(torch, cid):
    c = XC.case(cid)
    p = XC.params(c["setup"])
    L, col0, pad, _, T = XC.geometry(c)
    Yh = _spectra(c["B"], c["F"], c["n_fft"])
    v = _v(p, L)
    ref = _ref64(Yh, v, c["n_fft"], c["hop"], col0, pad, T, c["normalize"])
    Y = torch.from_numpy(Yh).cuda()
    two = bhw.istft_overlap_add(p, torch.fft.irfft(Y, n=c["n_fft"], dim=-1), c["n_fft"], c["hop"], **_kw(c))
    yard = _err(two.cpu().numpy(), ref)
    got = _call(torch, p, c, Y)
    assert got.dtype == torch.float32 and tuple(got.shape) == (c["B"], T)
    with bhw.ResidentTable(p) as tab:
        d = XC.parse(XC.line(c, table=tab._live()))
        assert d["table"] and "k_istft_mfft_table" in d["kernels"], d["line"]
        gt = _call(torch, p, c, Y, table=tab)
        torch.cuda.synchronize()
    assert np.array_equal(_bits(got), _bits(gt)), "library against table"
    err = _err(got.cpu().numpy(), ref)
    cap = 2.0 ** -24 * math.log2(c["n_fft"])
    print(f"istft mfft {cid}: n_fft {c['n_fft']} L {L} hop {c['hop']} rows {c['B'] * c['F']}: fused {err:.3e}, irfft + istft_overlap_add "
          f"{yard:.3e}, ratio {err / yard if yard else float('nan'):.3f}, cap {cap:.3e}")
    assert err <= 2.0 * yard, (cid, err, yard)
    assert err <= cap, (cid, err, cap)
    # outputs no frame reaches are +0.0
    t0 = pad - col0
    w = np.arange(T) + t0
    reached = np.zeros(T, dtype=bool)
    for f in range(c["F"]):
        reached |= (w >= f * c["hop"]) & (w < f * c["hop"] + L)
    assert not _bits(got)[:, ~reached].any()
    if "hop above L (zeros inside the signal)" in c["classes"] or "length past the frames' extent" in c["classes"]:
        assert (~reached).any()


PROPERTY_SHAPES = [
    dict(id="n50", setup=3, n_fft=50, L=37, hop=11, center=True, normalize=True, B=1, F=40),
    dict(id="n1200", setup=4, n_fft=1200, L=1200, hop=300, center=True, normalize=True, B=1, F=24),
]


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=[s["id"] for s in PROPERTY_SHAPES])
def test_an_output_depends_on_nothing_but_its_rows(torch, shape):
    """The same signal alone and as signal 37 of a batch of 64; as the last signal of a longer call, which has more spans, and as the
    first frames of a shorter one, whose first span is shorter; packed against padded strides; the imaginary parts of bins 0 and
    n_fft / 2 changed, NaN and infinity included.  Word for word.  Outputs formed across span boundaries of different cuts are held by
    test_the_cut_into_spans_does_not_reach_the_bits."""
    c = dict(shape)
    p = XC.params(c["setup"])
    n_fft, hop, F = c["n_fft"], c["hop"], c["F"]
    Yh = _spectra(64, F, n_fft, seed=5)
    Y = torch.from_numpy(Yh).cuda()
    T = XC.geometry(c)[4]
    alone = _call(torch, p, c, Y[37:38].clone())
    batch = _call(torch, p, dict(c, B=64), Y)
    assert np.array_equal(_bits(alone[0]), _bits(batch[37]))
    # a longer output and more signals: more spans, another slot and group
    cl = dict(c, B=7, extra=3 * n_fft)
    d1 = XC.parse(XC.line(c))
    long = _call(torch, p, cl, Y[31:38].clone())
    assert np.array_equal(_bits(long[6, :T]), _bits(alone[0]))
    assert XC.parse(XC.line(cl))["spans"] > d1["spans"]
    # padded strides against packed ones, the gaps of x and Y intact (_call checks them)
    padded = _call(torch, p, dict(c, B=5, padded=True), Y[35:40].clone())
    assert np.array_equal(_bits(padded[2]), _bits(alone[0]))
    # all but the first nine frames dropped: the planner cuts that call into shorter spans (S is at most the frame count), and only the
    # outputs the dropped frames reach change
    t0 = XC.desc(c)[3] - XC.desc(c)[2]
    cf = dict(c, F=9, extra=(F - 9) * hop)
    assert XC.geometry(cf)[4] == T and XC.parse(XC.line(cf))["S"] != d1["S"]
    fewer = _call(torch, p, cf, Y[37:38, :9].contiguous())
    keep = np.arange(T) + t0 < 9 * hop
    assert keep.sum() > 4 * hop
    assert np.array_equal(_bits(fewer[0])[keep], _bits(alone[0])[keep])
    assert not np.array_equal(_bits(fewer[0])[~keep], _bits(alone[0])[~keep])
    # the imaginary parts of the purely real bins never enter the arithmetic
    for bad in (3.0, np.nan, np.inf):
        Yi = Yh[37:38].copy()
        Yi.imag[..., 0] = bad                                            # not `re + 1j * bad`: 1j * nan has a NaN real part too
        Yi.imag[..., -1] = -bad
        assert np.array_equal(Yi.real, Yh[37:38].real)
        assert np.array_equal(_bits(_call(torch, p, c, torch.from_numpy(Yi).cuda())), _bits(alone)), bad
    with bhw.ResidentTable(p) as tab:
        assert np.array_equal(_bits(_call(torch, p, c, Y[37:38].clone(), table=tab)), _bits(alone))
        torch.cuda.synchronize()


# One long signal alone is cut by the halo term (S = 4 * halo); as signal 37 of 64 the grid term wins (S = 64 * F / (1024 * fy)).
SPAN_SHAPES = [
    dict(id="n50", setup=3, n_fft=50, L=37, hop=11, center=True, normalize=True, B=1, F=8000),
    dict(id="n1200", setup=4, n_fft=1200, L=1200, hop=300, center=True, normalize=True, B=1, F=256),
]


def _cuts(d, T):
    """The span boundaries of a signal that lie strictly inside its outputs, on the axis w = t + t0."""
    step = d["S"] * d["hop_eff"]
    return {s * step for s in range(1, d["spans"]) if d["t0"] < s * step < d["t0"] + T}


@pytest.mark.parametrize("shape", SPAN_SHAPES, ids=[s["id"] for s in SPAN_SHAPES])
def test_the_cut_into_spans_does_not_reach_the_bits(torch, shape):
    """The same signal in two calls whose describe lines show spans of different lengths -- S = 4 * halo alone, S from the grid target
    as signal 37 of 64: every output of the signal, word for word.  Both calls cut the signal several times and at different places,
    so the compared outputs include ones that one call forms right behind a boundary, from halo frames it transforms a second time,
    and the other in the middle of a span."""
    c = dict(shape)
    cb = dict(c, B=64)
    p = XC.params(c["setup"])
    n_fft, hop, F = c["n_fft"], c["hop"], c["F"]
    T = XC.geometry(c)[4]
    d1, d2 = XC.parse(XC.line(c)), XC.parse(XC.line(cb))
    for d in (d1, d2):
        d["hop_eff"] = min(hop, d["t0"] + T)
        assert d["halo"] > 0 and d["spans"] > 2 and d["repeated"] > 0, d["line"]
    assert d1["S"] == XC.HALO_FACTOR * d1["halo"] and d2["S"] > d1["S"], (d1["line"], d2["line"])
    k1, k2 = _cuts(d1, T), _cuts(d2, T)
    assert len(k1 - k2) >= 2 and len(k2 - k1) >= 2, (sorted(k1)[:4], sorted(k2)[:4])    # the compared range crosses boundaries of both
    g = torch.Generator(device="cuda").manual_seed(77)
    K = n_fft // 2 + 1
    Y = torch.view_as_complex(torch.randn((64, F, K, 2), device="cuda", generator=g) * 100.0)
    alone = _call(torch, p, c, Y[37:38].clone())
    batch = _call(torch, p, cb, Y)
    assert tuple(alone.shape) == (1, T) and tuple(batch.shape) == (64, T)
    a, b = _bits(alone[0]), _bits(batch[37])
    assert np.array_equal(a, b), np.flatnonzero(a != b)[:8] + d1["t0"]
    assert bool(torch.isfinite(alone).all()) and len(np.unique(a)) > T // 2


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=[s["id"] for s in PROPERTY_SHAPES])
def test_zeros_give_plus_zero_and_a_nan_reaches_exactly_the_outputs_under_its_window(torch, shape):
    c = dict(shape, B=3)
    p = XC.params(c["setup"])
    n_fft, hop, F, L = c["n_fft"], c["hop"], c["F"], c["L"]
    _, _, col0, pad, T = XC.desc(c)
    t0 = pad - col0
    for normalize in (True, False):
        cn = dict(c, normalize=normalize)
        z = _call(torch, p, cn, torch.zeros((3, F, n_fft // 2 + 1), dtype=torch.complex64, device="cuda"))
        assert not _bits(z).any(), "zeros in, +0.0 out"
        Yh = _spectra(3, F, n_fft, seed=9)
        clean = _call(torch, p, cn, torch.from_numpy(Yh).cuda())
        assert bool(torch.isfinite(clean).all())
        for bad in (np.nan, np.inf):
            Yn = Yh.copy()
            f = F // 2
            Yn[1, f, 5] = bad
            got = _call(torch, p, cn, torch.from_numpy(Yn).cuda())
            w = np.arange(T) + t0
            hit = np.zeros((3, T), dtype=bool)
            hit[1] = (w >= f * hop) & (w < f * hop + L)
            assert hit.sum() == L
            assert np.array_equal(~torch.isfinite(got).cpu().numpy(), hit), (normalize, bad)
            assert np.array_equal(_bits(got)[~hit], _bits(clean)[~hit])


@pytest.mark.parametrize("n_fft,L,hop", [(400, 400, 160), (480, 400, 100)])
def test_round_trip_reproduces_the_signal_as_well_as_torch(torch, n_fft, L, hop):
    """bhw.istft_mixed(bhw.stft_mixed(x)) with normalize=True and length=T (BH-4, reflect) against torch.istft(torch.stft(x)) with the
    same float window v: its relative l2 error is at most twice torch's, the factor the accuracy gate gives the fused transform over
    rocFFT's."""
    p = B.make_params(B.WIN_BH4, 12, 32)
    T = 16000
    g = torch.Generator(device="cuda").manual_seed(21)
    x = torch.randn((3, T), device="cuda", generator=g) * 100 + 5.0
    v = bhw.window(p, L, dtype=torch.float32)
    back = bhw.istft_mixed(p, bhw.stft_mixed(p, x, n_fft, hop, win_length=L), n_fft, hop, win_length=L, length=T)
    St = torch.stft(x, n_fft, hop, L, window=v, center=True, pad_mode="reflect", return_complex=True)
    tback = torch.istft(St, n_fft, hop, L, window=v, center=True, length=T)
    xh = x.cpu().numpy().astype(np.float64)
    err, yard = _err(back.cpu().numpy(), xh), _err(tback.cpu().numpy(), xh)
    print(f"istft_mixed(stft_mixed(x)) {L} / {n_fft} / {hop}: fused {err:.3e}, torch.istft(torch.stft(x)) {yard:.3e}, ratio {err / yard:.3f}")
    assert back.shape == x.shape and err <= 2.0 * yard, (err, yard)
    with bhw.ResidentTable(p) as tab:
        tb = tab.istft_mixed(p, tab.stft_mixed(p, x, n_fft, hop, win_length=L), n_fft, hop, win_length=L, length=T)
        torch.cuda.synchronize()
    assert torch.equal(tb, back)


def test_against_torch_istft(torch):
    """bhw.istft_mixed(S.transpose(-1, -2), 400, 160) against torch.istft(S, 400, 160, window=v): both against the float64 reference,
    the fused within twice torch."""
    p = B.make_params(B.WIN_BH7, 12, 32)
    n_fft, L, hop, F, nb = 400, 400, 160, 60, 3
    for extra in (0, -7):
        Yh = _spectra(nb, F, n_fft, seed=n_fft)
        S = torch.from_numpy(np.ascontiguousarray(Yh.transpose(0, 2, 1))).cuda()            # torch's layout (B, K, F)
        v = bhw.window(p, L, dtype=torch.float32)
        T = n_fft + hop * (F - 1) - n_fft + extra
        want = torch.istft(S, n_fft, hop, L, window=v, center=True, length=T)
        got = bhw.istft_mixed(p, S.transpose(-1, -2), n_fft, hop, length=T)
        assert got.shape == want.shape == (nb, T)
        ref = _ref64(Yh, _v(p, L), n_fft, hop, 0, n_fft // 2, T, True)
        err, yard = _err(got.cpu().numpy(), ref), _err(want.cpu().numpy(), ref)
        print(f"istft_mixed against torch.istft n_fft {n_fft} hop {hop} length {T}: fused {err:.3e}, torch {yard:.3e}, ratio {err / yard:.3f}")
        assert err <= 2.0 * yard, (err, yard)
        one = bhw.istft_mixed(p, S[1].transpose(-1, -2), n_fft, hop, length=T)
        assert one.dim() == 1 and torch.equal(one, got[1])
        # rows apart are read in place: the same bits as their packed copy
        wide = torch.zeros((nb, F, n_fft // 2 + 4), dtype=torch.complex64, device="cuda")
        wide[..., :n_fft // 2 + 1] = S.transpose(-1, -2)
        assert torch.equal(bhw.istft_mixed(p, wide[..., :n_fft // 2 + 1], n_fft, hop, length=T), got)


def test_graph_capture(torch):
    p = B.make_params(B.WIN_BH7, 12, 32)
    n_fft, hop, T, nb = 400, 160, 48000, 4
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((nb, T), device="cuda", generator=g) + 5.0
    with bhw.ResidentTable(p) as tab:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                Y = tab.stft_mixed(p, x, n_fft, hop)
                back = tab.istft_mixed(p, Y, n_fft, hop, length=T)                          # no warm call
                lib = bhw.istft_mixed(p, Y, n_fft, hop, length=T, normalize=False)          # no bhw_prepare_device
        torch.cuda.current_stream().wait_stream(s)
        x.copy_(torch.randn((nb, T), device="cuda", generator=g) * 3.0 - 2.0)
        back.fill_(-1.0)
        lib.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        Ye = tab.stft_mixed(p, x, n_fft, hop)
        be = tab.istft_mixed(p, Ye, n_fft, hop, length=T)
        le = bhw.istft_mixed(p, Ye, n_fft, hop, length=T, normalize=False)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(Y), torch.view_as_real(Ye))
        assert torch.equal(back, be) and torch.equal(lib, le)
        assert float((back - x).abs().max()) < 1e-3 * float(x.abs().max())


def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    Y = torch.zeros((2, 10, 201), dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError, match=r"power of two: bhw\.istft "):
        bhw.istft_mixed(p, torch.zeros((2, 10, 257), dtype=torch.complex64, device="cuda"), 512, 160)
    with pytest.raises(ValueError, match="2\\^a 3\\^b 5\\^c"):
        bhw.istft_mixed(p, torch.zeros((2, 10, 202), dtype=torch.complex64, device="cuda"), 402, 160)       # a factor 67
    with pytest.raises(ValueError, match="201 bins"):
        bhw.istft_mixed(p, Y, 480, 160)
    with pytest.raises(ValueError, match="complex64"):
        bhw.istft_mixed(p, Y.real.contiguous(), 400, 160)
    with pytest.raises(ValueError, match="complex64"):
        bhw.istft_mixed(p, Y.to(torch.complex128), 400, 160)
    with pytest.raises(ValueError, match="CUDA tensor"):
        bhw.istft_mixed(p, Y.cpu(), 400, 160)
    with pytest.raises(ValueError, match="out must be"):
        bhw.istft_mixed(p, Y, 400, 160, out=torch.zeros((2, 2880), device="cuda")[:, ::2])                # not contiguous
    with pytest.raises(ValueError, match="out must be"):
        bhw.istft_mixed(p, Y, 400, 160, out=torch.zeros((2, 100), device="cuda"))
    with pytest.raises(ValueError, match="power of two"):                                                 # and bhw.istft still refuses 400
        bhw.istft(p, Y, 400, 160)
    out = torch.empty((2, 1440), device="cuda")
    assert bhw.istft_mixed(p, Y, 400, 160, out=out).data_ptr() == out.data_ptr() and not bool(out.ne(0).any())
    # a parameter set the table was not built for: the key match of the from-table form
    with bhw.ResidentTable(p) as tab:
        with pytest.raises(B.BhwError):
            tab.istft_mixed(B.make_params(B.WIN_HANN, 11, 16), Y, 400, 160)
    torch.cuda.synchronize()
