"""The fused inverse mixed-radix complex FFT + overlap-add kernel on the GPU (bhw_istft_cmfft_f32_* through bhw.istft_iq_mixed and
ResidentTable.istft_iq_mixed), in the shape of tests/test_gpu_istft_iq.py.

Accuracy is the gate, and it is relative to the project's own two-step route: for every case of tests/istft_cmfft_cases.py the
reference is numpy in float64 (numpy.fft.ifft of the float32 bins in complex128, times the float32 v, overlap-added and divided by the
envelope), the metric the largest over the signals of |got - ref|_2 / |ref|_2, the yardstick
bhw.istft_overlap_add(torch.fft.ifft(Y)) on the same GPU, and the bounds twice the yardstick's error and 2^-24 * log2(n_fft).  A case
of a dozen rows lets single rows weigh in the ratio (1.42 was measured for the real mixed-radix inverse), so every case of the table
has at least 50 rows (tests/test_istft_cmfft_plan_coverage.py holds the table to that) and both gates apply to all of them.  The
inverse FFT is not pinned bit for bit; everything around it is, and those properties are held word for word at an even size (1536)
and an odd one (75)."""
import ctypes
import math

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import istft_cmfft_cases as IC

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
    """(B, F, n_fft) complex64 noise."""
    rng = np.random.default_rng(3100 + seed)
    return ((rng.standard_normal((nb, F, n_fft)) + 1j * rng.standard_normal((nb, F, n_fft))) * scale).astype(np.complex64)


def _ref64(Yh, v, n_fft, hop, col0, pad, T, normalize):
    """float64: ifft of every row, then S = sum r * v per part and E = sum v^2 over the frames reaching each output; (B, T) complex."""
    nb, F, _ = Yh.shape
    L = len(v)
    t0 = pad - col0
    vd = v.astype(np.float64)
    W = max(t0 + T, (F - 1) * hop + L)
    S, E = np.zeros((nb, W), dtype=np.complex128), np.zeros(W)
    for f0 in range(0, F, 256):
        rows = np.fft.ifft(Yh[:, f0:f0 + 256].astype(np.complex128), axis=-1)
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
    got, ref = np.asarray(got, dtype=np.complex128), np.asarray(ref)
    nr = np.sqrt((np.abs(ref) ** 2).sum(axis=-1))
    ne = np.sqrt((np.abs(got - ref) ** 2).sum(axis=-1))
    zero = nr == 0
    assert not (ne[zero] != 0).any(), "a signal whose reference is zero must come out zero"
    return float((ne[~zero] / nr[~zero]).max()) if (~zero).any() else 0.0


def _kw(c):
    return dict(win_length=c["L"], center=c["center"], length=IC.geometry(c)[4], normalize=c["normalize"])


def _raw_call(torch, p, c, Y, table=None):
    """The C call on the case's own descriptor (padded or odd strides included): Y (B, F, n_fft) complex64 on the GPU, bins in order ->
    (the float32 x buffer (B, x_stride) filled with a sentinel first, T).  The Y buffer is laid out by the strides, shifted along the
    bins for a shifted case; for an odd case x starts one float off the 8-byte grid."""
    s, L, _, _, T = IC.desc(c)
    nb, F, n = Y.shape
    ys = (s.y_stride or 2 * n) // 2
    ybs = (s.y_batch_stride or F * ys * 2) // 2
    ybuf = torch.full((nb, ybs), complex(SENTINEL, -SENTINEL), dtype=torch.complex64, device="cuda")
    ybuf[:, :F * ys].view(nb, F, ys)[:, :, :n] = torch.fft.fftshift(Y, dim=-1) if c.get("fftshift") else Y
    xs = s.x_stride or 2 * T
    off = 1 if c.get("odd") else 0
    store = torch.full((nb * xs + 2,), SENTINEL, device="cuda")
    assert store.data_ptr() % 8 == 0
    xbuf = store[off:off + nb * xs].view(nb, xs)
    assert xbuf.data_ptr() % 8 == 4 * off
    flags = (B.OLA_NORMALIZE if c["normalize"] else 0) | (B.CFFT_SHIFT if c.get("fftshift") else 0)
    dev = Y.device.index
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    tail = (ctypes.byref(s), flags, ctypes.c_void_p(ybuf.data_ptr()), ctypes.c_void_p(xbuf.data_ptr()))
    if table is None:
        B.check(B.lib().bhw_istft_cmfft_f32_device(ctypes.byref(p), L, dev, stream, *tail))
    else:
        B.check(B.lib().bhw_istft_cmfft_f32_from_table(table._live(), ctypes.byref(p), L, stream, *tail))
    torch.cuda.synchronize()
    assert float(store[0]) == SENTINEL or not off, "the float in front of x was written"
    assert bool((store[off + nb * xs:] == SENTINEL).all()), "a float behind x was written"
    return xbuf, T


def _call(torch, p, c, Y, table=None):
    """(B, T) complex64 on the GPU from bins in order: bhw.istft_iq_mixed / ResidentTable.istft_iq_mixed, or for a padded or an odd
    case the C call, the sentinels of the gaps checked."""
    if c.get("padded") or c.get("odd"):
        xbuf, T = _raw_call(torch, p, c, Y, table)
        assert bool((xbuf[:, 2 * T:] == SENTINEL).all()), "a gap of x was written"
        return torch.view_as_complex(xbuf[:, :2 * T].clone().view(-1, T, 2))     # a copy: x may sit one float off the grid
    fn = bhw.istft_iq_mixed if table is None else table.istft_iq_mixed
    if c.get("fftshift"):
        return fn(p, torch.fft.fftshift(Y, dim=-1), c["n_fft"], c["hop"], fftshift=True, **_kw(c))
    return fn(p, Y, c["n_fft"], c["hop"], **_kw(c))


def _bits(t):
    """(..., 2) words: both parts of every sample."""
    import torch
    return torch.view_as_real(t.contiguous()).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("cid", IC.case_ids())
def test_accuracy_within_twice_the_two_step_route(torch, cid):
    """Gate one: err <= 2 x the error of istft_overlap_add(torch.fft.ifft(Y)) on the same GPU.  Gate two: err <= 2^-24 * log2(n_fft)."""
    c = IC.case(cid)
    p = IC.params(c["setup"])
    L, col0, pad, _, T = IC.geometry(c)
    Yh = _spectra(c["B"], c["F"], c["n_fft"])
    v = _v(p, L)
    ref = _ref64(Yh, v, c["n_fft"], c["hop"], col0, pad, T, c["normalize"])
    Y = torch.from_numpy(Yh).cuda()
    two = bhw.istft_overlap_add(p, torch.fft.ifft(Y, dim=-1), c["n_fft"], c["hop"], **_kw(c))
    yard = _err(two.cpu().numpy(), ref)
    got = _call(torch, p, c, Y)
    assert got.dtype == torch.complex64 and tuple(got.shape) == (c["B"], T)
    with bhw.ResidentTable(p) as tab:
        d = IC.parse(IC.line(c, table=tab._live()))
        assert d["table"] and "k_istft_cmfft_table" in d["kernels"], d["line"]
        gt = _call(torch, p, c, Y, table=tab)
        torch.cuda.synchronize()
    assert np.array_equal(_bits(got), _bits(gt)), "library against table"
    err = _err(got.cpu().numpy(), ref)
    cap = 2.0 ** -24 * math.log2(c["n_fft"])
    print(f"istft cmfft {cid}: n_fft {c['n_fft']} L {L} hop {c['hop']} rows {c['B'] * c['F']}: fused {err:.3e}, ifft + istft_overlap_add "
          f"{yard:.3e}, ratio {err / yard if yard else float('nan'):.3f}, cap {cap:.3e} (share {err / cap:.3f})")
    assert err <= 2.0 * yard, (cid, err, yard)
    assert err <= cap, (cid, err, cap)
    # outputs no frame reaches are +0.0 in both parts
    t0 = pad - col0
    w = np.arange(T) + t0
    reached = np.zeros(T, dtype=bool)
    for f in range(c["F"]):
        reached |= (w >= f * c["hop"]) & (w < f * c["hop"] + L)
    assert not _bits(got)[:, ~reached].any()
    if "hop above L (zeros inside the signal)" in c["classes"] or "length past the frames' extent" in c["classes"]:
        assert (~reached).any()


PROPERTY_SHAPES = [
    dict(id="odd-75", setup=3, n_fft=75, L=60, hop=17, center=True, normalize=True, B=1, F=40),
    dict(id="even-1536", setup=4, n_fft=1536, L=1536, hop=384, center=True, normalize=True, B=1, F=24),
]


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=[s["id"] for s in PROPERTY_SHAPES])
def test_an_output_depends_on_nothing_but_its_rows(torch, shape):
    """The same signal alone and as signal 37 of a batch of 64; as the last signal of a longer call, which has more spans, and as the
    first frames of a shorter one, whose first span is shorter; packed against padded strides; x one float off the 8-byte grid with an
    odd stride against the aligned call; the shifted call on shifted bins against the call on bins in order; library against table.
    Word for word.  These calls share their span length or compare inside a first span; outputs formed across span boundaries are
    held by test_the_cut_into_spans_does_not_reach_the_bits."""
    c = dict(shape)
    p = IC.params(c["setup"])
    n_fft, hop, F = c["n_fft"], c["hop"], c["F"]
    Yh = _spectra(64, F, n_fft, seed=5)
    Y = torch.from_numpy(Yh).cuda()
    T = IC.geometry(c)[4]
    alone = _call(torch, p, c, Y[37:38].clone())
    batch = _call(torch, p, dict(c, B=64), Y)
    assert np.array_equal(_bits(alone[0]), _bits(batch[37]))
    # a longer output and more signals: more spans of the same length, another slot and group
    cl = dict(c, B=7, extra=3 * n_fft)
    d1 = IC.parse(IC.line(c))
    long = _call(torch, p, cl, Y[31:38].clone())
    assert np.array_equal(_bits(long[6, :T]), _bits(alone[0]))
    assert IC.parse(IC.line(cl))["spans"] > d1["spans"]
    # padded strides against packed ones, the gaps of x intact (_call checks them)
    padded = _call(torch, p, dict(c, B=5, padded=True), Y[35:40].clone())
    assert np.array_equal(_bits(padded[2]), _bits(alone[0]))
    # x one float off the 8-byte grid and an odd stride: two 4-byte stores per sample, the same bits
    odd = _call(torch, p, dict(c, B=5, odd=True), Y[35:40].clone())
    assert np.array_equal(_bits(odd[2]), _bits(alone[0]))
    one_off = _call(torch, p, dict(c, odd=True), Y[37:38].clone())
    assert np.array_equal(_bits(one_off), _bits(alone))
    # the shift is a load index: shifted bins under the flag, the bits of the call on the bins in order (Python and C call)
    assert np.array_equal(_bits(_call(torch, p, dict(c, fftshift=True), Y[37:38].clone())), _bits(alone))
    assert np.array_equal(_bits(_call(torch, p, dict(c, B=5, fftshift=True, padded=True), Y[35:40].clone())[2]), _bits(alone[0]))
    # all but the first nine frames dropped: the planner cuts that call into shorter spans (S is at most the frame count), and only the
    # outputs the dropped frames reach change
    t0 = IC.desc(c)[3] - IC.desc(c)[2]
    cf = dict(c, F=9, extra=(F - 9) * hop)
    assert IC.geometry(cf)[4] == T and IC.parse(IC.line(cf))["S"] != d1["S"]
    fewer = _call(torch, p, cf, Y[37:38, :9].contiguous())
    keep = np.arange(T) + t0 < 9 * hop
    assert keep.sum() > 4 * hop
    assert np.array_equal(_bits(fewer[0])[keep], _bits(alone[0])[keep])
    assert not np.array_equal(_bits(fewer[0])[~keep], _bits(alone[0])[~keep])
    with bhw.ResidentTable(p) as tab:
        assert np.array_equal(_bits(_call(torch, p, c, Y[37:38].clone(), table=tab)), _bits(alone))
        torch.cuda.synchronize()


# One long signal alone is cut by the halo term (S = 4 * halo); as signal 37 of 64 the grid term wins (S = 64 * F / (1024 * fy)).
SPAN_SHAPES = [
    dict(id="odd-75", setup=3, n_fft=75, L=60, hop=17, center=True, normalize=True, B=1, F=4000),
    dict(id="even-1536", setup=4, n_fft=1536, L=1536, hop=384, center=True, normalize=True, B=1, F=256),
]


def _cuts(d, T):
    """The span boundaries of a signal that lie strictly inside its outputs, on the axis w = t + t0."""
    step = d["S"] * d["hop_eff"]
    return {s * step for s in range(1, d["spans"]) if d["t0"] < s * step < d["t0"] + T}


@pytest.mark.parametrize("shape", SPAN_SHAPES, ids=[s["id"] for s in SPAN_SHAPES])
def test_the_cut_into_spans_does_not_reach_the_bits(torch, shape):
    """The same signal in two calls whose describe lines show spans of different lengths -- alone the halo sets S (4 * halo), in the
    batch the grid target does: every output of the signal, word for word.  Both calls cut the signal several times and at different
    places, so the compared outputs include ones that one call forms right behind a boundary, from halo frames it transforms a
    second time, and the other in the middle of a span."""
    c = dict(shape)
    cb = dict(c, B=64)
    p = IC.params(c["setup"])
    n_fft, hop, F = c["n_fft"], c["hop"], c["F"]
    T = IC.geometry(c)[4]
    d1, d2 = IC.parse(IC.line(c)), IC.parse(IC.line(cb))
    for d in (d1, d2):
        d["hop_eff"] = min(hop, d["t0"] + T)
        assert d["halo"] > 0 and d["spans"] > 2 and d["repeated"] > 0, d["line"]
    assert d1["S"] == IC.HALO_FACTOR * d1["halo"] and d2["S"] == 64 * F // (IC.TARGET_GROUPS * d2["fy"]) > d1["S"], (d1["line"], d2["line"])
    k1, k2 = _cuts(d1, T), _cuts(d2, T)
    assert len(k1 - k2) >= 2 and len(k2 - k1) >= 2, (sorted(k1)[:4], sorted(k2)[:4])    # the compared range crosses boundaries of both
    g = torch.Generator(device="cuda").manual_seed(77)
    Y = torch.view_as_complex(torch.randn((64, F, n_fft, 2), device="cuda", generator=g) * 100.0)
    alone = _call(torch, p, c, Y[37:38].clone())
    batch = _call(torch, p, cb, Y)
    assert tuple(alone.shape) == (1, T) and tuple(batch.shape) == (64, T)
    a, b = _bits(alone[0]), _bits(batch[37])
    assert np.array_equal(a, b), np.flatnonzero((a != b).any(axis=-1))[:8] + d1["t0"]
    assert bool(torch.isfinite(torch.view_as_real(alone)).all()) and len(np.unique(a)) > T // 2


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=[s["id"] for s in PROPERTY_SHAPES])
def test_zeros_give_plus_zero_and_a_nan_reaches_exactly_the_outputs_under_its_window(torch, shape):
    """A bin that is NaN in both parts makes both parts of exactly the outputs under that row's window non-finite; every other output
    keeps its bits."""
    c = dict(shape, B=3)
    p = IC.params(c["setup"])
    n_fft, hop, F, L = c["n_fft"], c["hop"], c["F"], c["L"]
    _, _, col0, pad, T = IC.desc(c)
    t0 = pad - col0
    for normalize in (True, False):
        for shifted in (False, True):
            cn = dict(c, normalize=normalize, fftshift=shifted)
            z = _call(torch, p, cn, torch.zeros((3, F, n_fft), dtype=torch.complex64, device="cuda"))
            assert not _bits(z).any(), "zeros in, +0.0 out"
            Yh = _spectra(3, F, n_fft, seed=9)
            clean = _call(torch, p, cn, torch.from_numpy(Yh).cuda())
            assert bool(torch.isfinite(torch.view_as_real(clean)).all())
            Yn = Yh.copy()
            f = F // 2
            Yn[1, f, 5] = complex(np.nan, np.nan)
            got = _call(torch, p, cn, torch.from_numpy(Yn).cuda())
            w = np.arange(T) + t0
            hit = np.zeros((3, T), dtype=bool)
            hit[1] = (w >= f * hop) & (w < f * hop + L)
            assert hit.sum() == L
            bad = ~torch.isfinite(torch.view_as_real(got)).cpu().numpy()
            assert np.array_equal(bad[..., 0], hit) and np.array_equal(bad[..., 1], hit), (normalize, shifted)
            assert np.array_equal(_bits(got)[~hit], _bits(clean)[~hit])


@pytest.mark.parametrize("n_fft,L,hop", [(400, 400, 160), (375, 300, 125)], ids=["400-160", "odd-375"])
def test_round_trip_reproduces_the_signal_as_well_as_torch(torch, n_fft, L, hop):
    """bhw.istft_iq_mixed(bhw.stft_iq_mixed(x)) with normalize=True and length=T (BH-4, reflect) against
    torch.istft(torch.stft(x, onesided=False), return_complex=True) with the same v: its relative l2 error is at most twice torch's.
    In order and shifted both ways, at 400 / 160 and at an odd n_fft."""
    p = B.make_params(B.WIN_BH4, 12, 32)
    T = 16000
    g = torch.Generator(device="cuda").manual_seed(21)
    x = torch.view_as_complex(torch.randn((3, T, 2), device="cuda", generator=g) * 100 + 5.0)
    v = bhw.window(p, L, dtype=torch.float32)
    back = bhw.istft_iq_mixed(p, bhw.stft_iq_mixed(p, x, n_fft, hop, win_length=L), n_fft, hop, win_length=L, length=T)
    St = torch.stft(x, n_fft, hop, L, window=v, center=True, pad_mode="reflect", onesided=False, return_complex=True)
    tback = torch.istft(St, n_fft, hop, L, window=v, center=True, length=T, onesided=False, return_complex=True)
    xh = x.cpu().numpy().astype(np.complex128)
    err, yard = _err(back.cpu().numpy(), xh), _err(tback.cpu().numpy(), xh)
    print(f"istft_iq_mixed(stft_iq_mixed(x)) {L} / {n_fft} / {hop}: fused {err:.3e}, torch.istft(torch.stft(x)) {yard:.3e}, ratio {err / yard:.3f}")
    assert back.shape == x.shape and back.dtype == torch.complex64 and err <= 2.0 * yard, (err, yard)
    shifted = bhw.istft_iq_mixed(p, bhw.stft_iq_mixed(p, x, n_fft, hop, win_length=L, fftshift=True), n_fft, hop, win_length=L, length=T,
                                 fftshift=True)
    assert torch.equal(torch.view_as_real(shifted), torch.view_as_real(back))
    with bhw.ResidentTable(p) as tab:
        tb = tab.istft_iq_mixed(p, tab.stft_iq_mixed(p, x, n_fft, hop, win_length=L), n_fft, hop, win_length=L, length=T)
        torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(tb), torch.view_as_real(back))


def test_against_torch_istft(torch):
    """bhw.istft_iq_mixed(S.transpose(-1, -2)) against torch.istft(S, onesided=False, return_complex=True): both against the float64
    reference, the fused within twice torch.  center=False needs L = n_fft and a window that does not vanish at its ends (torch.istft
    refuses an envelope below 1e-11, and a BH-7 end squared is below it): Hamming, whose ends are 0.08."""
    bh7, hamming = B.make_params(B.WIN_BH7, 12, 32), B.make_params(B.WIN_HAMMING, 12, 32)
    for p, n_fft, L, hop, center, extra in ((bh7, 600, 400, 160, True, 0), (bh7, 400, 400, 100, True, -7), (bh7, 75, 49, 16, True, 5),
                                            (hamming, 300, 300, 75, False, 0)):
        F, nb = 60, 3
        Yh = _spectra(nb, F, n_fft, seed=n_fft)
        S = torch.from_numpy(np.ascontiguousarray(Yh.transpose(0, 2, 1))).cuda()            # torch's layout (B, n_fft, F)
        v = bhw.window(p, L, dtype=torch.float32)
        pad = n_fft // 2 if center else 0
        T = n_fft + hop * (F - 1) - 2 * pad + extra
        want = torch.istft(S, n_fft, hop, L, window=v, center=center, length=T, onesided=False, return_complex=True)
        kw = dict(win_length=L, center=center, length=T)
        got = bhw.istft_iq_mixed(p, S.transpose(-1, -2), n_fft, hop, **kw)
        assert got.shape == want.shape == (nb, T) and got.dtype == torch.complex64
        ref = _ref64(Yh, _v(p, L), n_fft, hop, (n_fft - L) // 2, pad, T, True)
        err, yard = _err(got.cpu().numpy(), ref), _err(want.cpu().numpy(), ref)
        print(f"istft_iq_mixed against torch.istft n_fft {n_fft} L {L} hop {hop} center {center}: fused {err:.3e}, torch {yard:.3e}, "
              f"ratio {err / yard:.3f}")
        assert err <= 2.0 * yard, (n_fft, err, yard)
        one = bhw.istft_iq_mixed(p, S[1].transpose(-1, -2), n_fft, hop, **kw)
        assert one.dim() == 1 and np.array_equal(_bits(one), _bits(got[1]))
        # rows apart are read in place, a broadcast and a lazy conjugate are copied: the same bits as their packed copies
        wide = torch.zeros((nb, F, n_fft + 4), dtype=torch.complex64, device="cuda")
        wide[..., :n_fft] = S.transpose(-1, -2)
        assert np.array_equal(_bits(bhw.istft_iq_mixed(p, wide[..., :n_fft], n_fft, hop, **kw)), _bits(got))
        row = S.transpose(-1, -2)[0:1]
        assert np.array_equal(_bits(bhw.istft_iq_mixed(p, row.expand(2, -1, -1), n_fft, hop, **kw)[1]), _bits(got[0]))
        cj = S.transpose(-1, -2).conj()
        assert cj.is_conj()
        assert np.array_equal(_bits(bhw.istft_iq_mixed(p, cj, n_fft, hop, **kw)),
                              _bits(bhw.istft_iq_mixed(p, cj.resolve_conj().contiguous(), n_fft, hop, **kw)))


def test_graph_capture(torch):
    """Both forms with no warm call (the table form on its first call, the library form with no bhw_prepare_device), and a captured
    stft_iq_mixed -> istft_iq_mixed chain."""
    p = B.make_params(B.WIN_BH7, 12, 32)
    L, n_fft, hop, T, nb = 400, 600, 160, 48000, 4
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.view_as_complex(torch.randn((nb, T, 2), device="cuda", generator=g) + 5.0)
    with bhw.ResidentTable(p) as tab:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                Y = tab.stft_iq_mixed(p, x, n_fft, hop, win_length=L)
                back = tab.istft_iq_mixed(p, Y, n_fft, hop, win_length=L, length=T)                  # no warm call
                lib = bhw.istft_iq_mixed(p, Y, n_fft, hop, win_length=L, length=T, normalize=False)  # no bhw_prepare_device
        torch.cuda.current_stream().wait_stream(s)
        x.copy_(torch.view_as_complex(torch.randn((nb, T, 2), device="cuda", generator=g) * 3.0 - 2.0))
        back.fill_(-1.0)
        lib.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        Ye = tab.stft_iq_mixed(p, x, n_fft, hop, win_length=L)
        be = tab.istft_iq_mixed(p, Ye, n_fft, hop, win_length=L, length=T)
        le = bhw.istft_iq_mixed(p, Ye, n_fft, hop, win_length=L, length=T, normalize=False)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(Y), torch.view_as_real(Ye))
        assert torch.equal(torch.view_as_real(back), torch.view_as_real(be)) and torch.equal(torch.view_as_real(lib), torch.view_as_real(le))
        assert float((back - x).abs().max()) < 1e-3 * float(x.abs().max())


def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    Y = torch.zeros((2, 10, 48), dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError, match="complex64"):
        bhw.istft_iq_mixed(p, Y.real.contiguous(), 48, 16)
    with pytest.raises(ValueError, match="complex64"):
        bhw.istft_iq_mixed(p, Y.to(torch.complex128), 48, 16)
    with pytest.raises(ValueError, match="complex64 CUDA tensor"):
        bhw.istft_iq_mixed(p, Y.cpu(), 48, 16)
    with pytest.raises(ValueError, match="25 bins"):
        bhw.istft_iq_mixed(p, Y[..., :25], 48, 16)                        # a one-sided spectrum
    with pytest.raises(ValueError, match="48 bins"):
        bhw.istft_iq_mixed(p, Y, 96, 16)
    with pytest.raises(ValueError, match="power of two: bhw.istft_iq"):
        bhw.istft_iq_mixed(p, torch.zeros((2, 10, 64), dtype=torch.complex64, device="cuda"), 64, 16)
    with pytest.raises(ValueError, match=r"2\^a 3\^b 5\^c in 16..2047"):
        bhw.istft_iq_mixed(p, torch.zeros((2, 3, 2160), dtype=torch.complex64, device="cuda"), 2160, 540, win_length=1024)
    with pytest.raises(ValueError, match=r"2\^a 3\^b 5\^c in 16..2047"):
        bhw.istft_iq_mixed(p, torch.zeros((2, 10, 70), dtype=torch.complex64, device="cuda"), 70, 16)
    with pytest.raises(ValueError, match="center=False"):
        bhw.istft_iq_mixed(p, Y, 48, 16, win_length=40, center=False)
    with pytest.raises(ValueError, match="hop"):
        bhw.istft_iq_mixed(p, Y, 48, 0)
    with pytest.raises(ValueError, match=r"\(frames, n_fft\)"):
        bhw.istft_iq_mixed(p, Y[0, 0], 48, 16)
    with pytest.raises(ValueError, match="out must be"):
        bhw.istft_iq_mixed(p, Y, 48, 16, out=torch.zeros((2, 100), dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        bhw.istft_iq_mixed(p, Y, 48, 16, out=torch.zeros((2, 144), device="cuda"))
    with pytest.raises(ValueError, match="length"):
        bhw.istft_iq_mixed(p, Y, 48, 16, length=-1)
    out = torch.empty((2, 144), dtype=torch.complex64, device="cuda")
    assert bhw.istft_iq_mixed(p, Y, 48, 16, out=out).data_ptr() == out.data_ptr() and not _bits(out).any()
    # the older fronts keep refusing what they refuse
    with pytest.raises(ValueError, match="power of two"):
        bhw.istft_iq(p, Y, 48, 16)
    with pytest.raises(ValueError, match="48 bins"):
        bhw.istft_mixed(p, Y, 48, 16)
    # a parameter set the table was not built for: the key match of the from-table form
    with bhw.ResidentTable(p) as tab:
        with pytest.raises(B.BhwError):
            tab.istft_iq_mixed(B.make_params(B.WIN_HANN, 11, 16), Y, 48, 16)
    torch.cuda.synchronize()
