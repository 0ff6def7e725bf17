"""The mixed-radix fused STFT + mask + inverse STFT kernel on the GPU (bhw_mask_mfft_f32_* through bhw.stft_mask_istft_mixed).

The gate is exact: for every case of tests/mask_mfft_cases.py, library and table form, the output equals WORD FOR WORD (torch.equal on
the int32 views, so the sign of a zero counts) bhw.istft_mixed(p, Ym) with
Ym = view_as_complex(view_as_real(bhw.stft_mixed(p, x)) * g[..., None]) in float32 -- the three-call route the kernel replaces.  The
properties around it (sentinels, batch independence, broadcast gains, NaN locality, zero and unit gains, graph capture) are held word
for word too; one test holds the whole chain to float64 within twice torch's own error.

Measured end to end on an MI355X (maximum absolute error against float64, fused / torch.istft(torch.stft * g) in float32): see
DESIGN.md section 42."""
import ctypes

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import mask_mfft_cases as MM
import table_source_cases as TS

pytestmark = pytest.mark.gpu

SENTINEL = 12345.5
GUARD = 64


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _same(torch, a, b):
    """Word for word: the int32 views are equal (a +0.0 is not a -0.0, a NaN equals the NaN of the same bits)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _where(torch, a, b):
    d = (a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).nonzero()
    return int(d.shape[0]), d[:4].tolist()


def _inputs(torch, nb, Tin, F, K, seed=0):
    """x (B, T_in) fixed-seed noise with an offset, g (B, F, K) uniform in [0, 2) with about a tenth exact 0 and a tenth exact 1."""
    g = torch.Generator(device="cuda").manual_seed(4200 + seed)
    x = torch.randn((nb, Tin), device="cuda", generator=g) * 100.0 + 5.0
    gains = torch.rand((nb, F, K), device="cuda", generator=g) * 2.0
    pick = torch.rand((nb, F, K), device="cuda", generator=g)
    gains = torch.where(pick < 0.1, torch.zeros_like(gains), torch.where(pick > 0.9, torch.ones_like(gains), gains))
    return x, gains


def _layout(gains, layout):
    """The mask tensor of a layout, and the same gains expanded to (B, F, K)."""
    if layout == "K":
        m = gains[0, 0].contiguous()
    elif layout == "FK":
        m = gains[0].contiguous()
    elif layout == "B1K":
        m = gains[:, 0:1].contiguous()
    else:
        m = gains
    return m, m.expand(gains.shape)


def _kw(c):
    return dict(win_length=c["L"], center=c["center"], length=MM.geometry(c)[4], normalize=c["normalize"])


def _three_calls(torch, p, c, x, gfull, table=None):
    """The route the kernel replaces: stft_mixed, a float32 multiply of each part by its gain, istft_mixed -- all from the same source."""
    stft, istft = (bhw.stft_mixed, bhw.istft_mixed) if table is None else (table.stft_mixed, table.istft_mixed)
    Y = stft(p, x, c["n_fft"], c["hop"], win_length=c["L"], center=c["center"], pad_mode=c["pad_mode"])
    Ym = torch.view_as_complex((torch.view_as_real(Y) * gfull[..., None]).contiguous())
    return istft(p, Ym, c["n_fft"], c["hop"], **_kw(c))


def _raw_call(torch, p, c, x, gfull, table=None):
    """The C call on the case's own descriptors (padded strides): sentinels around out and in the gaps of its stride, NaN in the gaps of
    the input stride and of the gain strides, so a stray read shows in the result.  Returns (B, T) and checks the sentinels."""
    sa, ss, L, Tin, T, gs, gbs = MM.desc(c)
    nb, F, K = gfull.shape
    xs, os_ = sa.x_stride or Tin, ss.x_stride or T
    xbuf = torch.full((nb, xs), float("nan"), device="cuda")
    xbuf[:, :Tin] = x
    gbuf = torch.full((nb * max(gbs, 1) + F * max(gs, 1) + K,), float("nan"), device="cuda")
    rows = torch.as_strided(gbuf, (nb if gbs else 1, F if gs else 1, K), (gbs, gs, 1))
    rows.copy_(gfull[:rows.shape[0], :rows.shape[1]])
    flat = torch.full((2 * GUARD + nb * os_,), SENTINEL, device="cuda")
    obuf = flat[GUARD:GUARD + nb * os_].view(nb, os_)
    flags = B.OLA_NORMALIZE if c["normalize"] else 0
    dev = x.device.index
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    tail = (ctypes.byref(sa), ctypes.byref(ss), flags, ctypes.c_void_p(xbuf.data_ptr()), ctypes.c_void_p(gbuf.data_ptr()), gs, gbs,
            ctypes.c_void_p(obuf.data_ptr()))
    if table is None:
        B.check(B.lib().bhw_mask_mfft_f32_device(ctypes.byref(p), L, dev, stream, *tail))
    else:
        B.check(B.lib().bhw_mask_mfft_f32_from_table(table._live(), ctypes.byref(p), L, stream, *tail))
    torch.cuda.synchronize()
    assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + nb * os_:] == SENTINEL).all()), "a word around out was written"
    assert bool((obuf[:, T:] == SENTINEL).all()), "a gap of out was written"
    assert bool(torch.isnan(xbuf[:, Tin:]).all()) and int(torch.isnan(gbuf).sum()) == gbuf.numel() - rows.numel()
    return obuf[:, :T].contiguous()


def _call(torch, p, c, x, mask, gfull, table=None):
    if c.get("padded") or c["gains"] == "padded":
        return _raw_call(torch, p, c, x, gfull, table)
    return bhw.stft_mask_istft_mixed(p, x, mask, c["n_fft"], c["hop"], pad_mode=c["pad_mode"], table=table, **_kw(c))


@pytest.mark.parametrize("cid", MM.case_ids())
def test_word_for_word_the_three_call_route(torch, cid):
    c = MM.case(cid)
    p = MM.params(c["setup"])
    _, _, _, Tin, T = MM.geometry(c)
    K = c["n_fft"] // 2 + 1
    x, gains = _inputs(torch, c["B"], Tin, c["F"], K)
    mask, gfull = _layout(gains, c["gains"])
    want = _three_calls(torch, p, c, x, gfull)
    got = _call(torch, p, c, x, mask, gfull)
    assert got.dtype == torch.float32 and tuple(got.shape) == (c["B"], T)
    assert _same(torch, got, want), (cid, "library", _where(torch, got, want), MM.line(c))
    with bhw.ResidentTable(p) as tab:
        d = MM.parse(MM.line(c, table=tab._live()))
        assert d["table"] and list(d["kernels"]) == ["k_mask_mfft_table"], d["line"]
        wt = _three_calls(torch, p, c, x, gfull, table=tab)
        gt = _call(torch, p, c, x, mask, gfull, table=tab)
        torch.cuda.synchronize()
    assert _same(torch, gt, wt), (cid, "table", _where(torch, gt, wt))
    assert _same(torch, gt, got), "library against table"
    assert bool(torch.isfinite(got).all()) and (T == 0 or int(torch.unique(got.view(torch.int32)).numel()) > min(T, 64) // 2)


def test_sentinels_beyond_length_stay(torch):
    """out= longer than asked for is refused; an out of the exact shape inside a larger buffer leaves every word behind `length`."""
    c = MM.case("n30-l24-short")
    p = MM.params(c["setup"])
    _, _, _, Tin, T = MM.geometry(c)
    x, gains = _inputs(torch, c["B"], Tin, c["F"], 16, seed=2)
    flat = torch.full((c["B"] * T + 2 * GUARD,), SENTINEL, device="cuda")
    out = flat[GUARD:GUARD + c["B"] * T].view(c["B"], T)
    got = bhw.stft_mask_istft_mixed(p, x, gains, 30, c["hop"], pad_mode="reflect", out=out, **_kw(c))
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + c["B"] * T:] == SENTINEL).all())
    assert _same(torch, got, _three_calls(torch, p, dict(c, pad_mode="reflect"), x, gains))


TRIPLES = {}
for _t in TS.TABLES:
    for _w in TS.ROTATION[_t]:
        TRIPLES.setdefault(TS.triple(_t, _w), (_t, _w))


@pytest.mark.parametrize("triple", sorted(TRIPLES), ids=[f"fmt{f}-nt{n}-mode{m}" for f, n, m in sorted(TRIPLES)])
def test_every_table_instance(torch, triple):
    """k_mask_mfft_table<FMT, NT, MODE> for every triple the tables and weight sets of table_source_cases.py name, at the smallest mixed
    shape with an even M, a radix-5, a radix-3 and a radix-2 pass (n_fft 60): the describe line names the instance, and the result is
    the three-call route's from the same table, word for word."""
    tname, wname = TRIPLES[triple]
    p = TS.params(tname, wname)
    c = dict(n_fft=60, L=57, hop=17, F=24, B=2, center=True, normalize=True, pad_mode="reflect", setup=None)
    L, col0, pad, Tin, T = MM.geometry(c)
    K = 31
    x, gains = _inputs(torch, 2, Tin, 24, K, seed=7)
    with bhw.ResidentTable(p, table_format=TS.LIMITS[TS.TABLES[tname][3]]) as tab:
        sa = B.make_stft(2, Tin, 24, 17, 60, col0=col0, pad=pad, pad_mode=1, shift=p.dat_width - 1)
        ss = B.make_stft(2, T, 24, 17, 60, col0=col0, pad=pad, shift=p.dat_width - 1)
        d = MM.parse(B.describe_mask_mfft(p, L, sa, ss, normalize=True, g_stride=K, g_batch_stride=24 * K, table=tab._live()))
        assert d["kernels"] == {"k_mask_mfft_table": tuple(str(v) for v in triple)}, d["line"]
        want = _three_calls(torch, p, c, x, gains, table=tab)
        got = bhw.stft_mask_istft_mixed(p, x, gains, 60, 17, table=tab, **_kw(c))
        torch.cuda.synchronize()
    assert _same(torch, got, want) and bool(torch.isfinite(got).all()), _where(torch, got, want)


PROPERTY_SHAPES = [
    dict(id="small-odd-M", setup=3, n_fft=90, L=71, hop=13, center=True, normalize=True, B=1, F=40, pad_mode="reflect", gains="BFK"),
    dict(id="large", setup=4, n_fft=2000, L=2000, hop=500, center=True, normalize=True, B=1, F=24, pad_mode="constant", gains="BFK"),
]


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=[s["id"] for s in PROPERTY_SHAPES])
def test_an_output_depends_on_nothing_but_its_frames(torch, shape):
    """A signal alone and as signal 37 of 64; packed against padded strides (NaN in every gap); the (K,), (F, K) and (B, 1, K) layouts
    against the same gains materialised to (B, F, K); an expand() view against its copy.  Word for word."""
    c = dict(shape)
    p = MM.params(c["setup"])
    _, _, _, Tin, T = MM.geometry(c)
    F, K = c["F"], c["n_fft"] // 2 + 1
    x, gains = _inputs(torch, 64, Tin, F, K, seed=5)
    alone = _call(torch, p, c, x[37:38].clone(), gains[37:38].clone(), gains[37:38])
    batch = _call(torch, p, dict(c, B=64), x, gains, gains)
    assert _same(torch, alone[0], batch[37])
    padded = _call(torch, p, dict(c, B=5, padded=True, gains="padded"), x[35:40], None, gains[35:40])
    assert _same(torch, padded[2], alone[0])
    for layout in ("K", "FK", "B1K"):
        mask, gfull = _layout(gains[30:34], layout)
        assert mask.dim() == {"K": 1, "FK": 2, "B1K": 3}[layout]
        cb = dict(c, B=4)
        lean = _call(torch, p, cb, x[30:34], mask, gfull)
        full = _call(torch, p, cb, x[30:34], gfull.contiguous(), gfull)
        assert _same(torch, lean, full), layout
        view = _call(torch, p, cb, x[30:34], gfull, gfull)              # the expand() view itself: zero strides, nothing materialised
        assert gfull.stride(0) == 0 or gfull.stride(1) == 0
        assert _same(torch, view, full), layout
    one = bhw.stft_mask_istft_mixed(p, x[37], gains[37], c["n_fft"], c["hop"], pad_mode=c["pad_mode"], **_kw(c))
    assert one.dim() == 1 and _same(torch, one, alone[0])


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=[s["id"] for s in PROPERTY_SHAPES])
def test_a_nan_reaches_exactly_the_outputs_under_its_frame_and_zero_and_unit_gains(torch, shape):
    c = dict(shape, B=3)
    p = MM.params(c["setup"])
    L, col0, pad, Tin, T = MM.geometry(c)
    n_fft, hop, F, K = c["n_fft"], c["hop"], c["F"], c["n_fft"] // 2 + 1
    t0 = pad - col0
    x, gains = _inputs(torch, 3, Tin, F, K, seed=9)
    for normalize in (True, False):
        cn = dict(c, normalize=normalize)
        clean = _call(torch, p, cn, x, gains, gains)
        assert bool(torch.isfinite(clean).all())
        f = F // 2
        w = np.arange(T) + t0
        hit = np.zeros((3, T), dtype=bool)
        hit[1] = (w >= f * hop) & (w < f * hop + L)
        assert 0 < hit.sum() <= L
        keep = torch.from_numpy(~hit).cuda()
        for bad in (float("nan"), float("inf")):
            gn = gains.clone()
            gn[1, f, 5] = bad
            got = _call(torch, p, cn, x, gn, gn)
            assert np.array_equal(~torch.isfinite(got).cpu().numpy(), hit), (normalize, bad)
            assert _same(torch, got[keep], clean[keep])
        # a NaN sample: exactly the outputs under the frames whose window covers it
        xn = x.clone()
        ts = Tin // 2
        xn[1, ts] = float("nan")
        fr = [q for q in range(F) if 0 <= ts + pad - q * hop - col0 < L]
        hx = np.zeros((3, T), dtype=bool)
        for q in fr:
            hx[1] |= (w >= q * hop) & (w < q * hop + L)
        got = _call(torch, p, cn, xn, gains, gains)
        assert fr and np.array_equal(~torch.isfinite(got).cpu().numpy(), hx), normalize
        keep = torch.from_numpy(~hx).cuda()
        assert _same(torch, got[keep], clean[keep])
        # zero gains: what istft_mixed gives on those rows, sign of zero included; unit gains: istft_mixed(stft_mixed(x)) bit for bit
        zeros, ones = torch.zeros_like(gains), torch.ones_like(gains)
        assert _same(torch, _call(torch, p, cn, x, zeros, zeros), _three_calls(torch, p, cn, x, zeros))
        Y = bhw.stft_mixed(p, x, n_fft, hop, win_length=L, center=c["center"], pad_mode=c["pad_mode"])
        back = bhw.istft_mixed(p, Y, n_fft, hop, **_kw(cn))
        assert _same(torch, _call(torch, p, cn, x, ones, ones), back)


def test_graph_capture(torch):
    """The library form with no warm call, on a shape with several spans per signal; the table form on its first call; one stream, no
    parallel branches."""
    p = B.make_params(B.WIN_BH5, 12, 32)
    L, n_fft, hop, T, nb = 400, 400, 160, 48000, 4
    kw = dict(win_length=L, length=T)
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((nb, T), device="cuda", generator=g) + 5.0
    F, K = 1 + T // hop, n_fft // 2 + 1
    sa = B.make_stft(nb, T, F, hop, n_fft, col0=0, pad=200, pad_mode=1, shift=31)
    ss = B.make_stft(nb, T, F, hop, n_fft, col0=0, pad=200, shift=31)
    assert MM.parse(B.describe_mask_mfft(p, L, sa, ss, normalize=True, g_stride=K, g_batch_stride=F * K))["spans"] > 2
    mask = torch.rand((nb, F, K), device="cuda", generator=g) * 2.0
    with bhw.ResidentTable(p) as tab:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                lib = bhw.stft_mask_istft_mixed(p, x, mask, n_fft, hop, **kw)                     # no warm call, no bhw_prepare_device
                tb = bhw.stft_mask_istft_mixed(p, x, mask[0, 0], n_fft, hop, table=tab, **kw)      # the table form's first call
        torch.cuda.current_stream().wait_stream(s)
        x.copy_(torch.randn((nb, T), device="cuda", generator=g) * 3.0 - 2.0)
        mask.copy_(torch.rand((nb, F, K), device="cuda", generator=g))
        lib.fill_(-1.0)
        tb.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        le = bhw.stft_mask_istft_mixed(p, x, mask, n_fft, hop, **kw)
        te = bhw.stft_mask_istft_mixed(p, x, mask[0, 0], n_fft, hop, table=tab, **kw)
        torch.cuda.synchronize()
    assert _same(torch, lib, le) and _same(torch, tb, te)
    assert not torch.equal(lib, tb) and bool(torch.isfinite(lib).all())


def _ref64(x, g, v, n_fft, hop, L, pad_mode, T):
    """numpy float64 from x and g: rfft of the windowed frames (the library's float32 window values), times g, irfft, weighted
    overlap-add and envelope division; center=True."""
    nb, Tin = x.shape
    pad, col0 = n_fft // 2, (n_fft - L) // 2
    xp = np.pad(x.astype(np.float64), ((0, 0), (pad, pad)), mode="reflect" if pad_mode == "reflect" else "constant")
    F = 1 + (Tin + 2 * pad - n_fft) // hop
    vd = np.zeros(n_fft)
    vd[col0:col0 + L] = v.astype(np.float64)
    S, E = np.zeros((nb, (F - 1) * hop + n_fft)), np.zeros((F - 1) * hop + n_fft)
    for f in range(F):
        row = np.fft.irfft(np.fft.rfft(xp[:, f * hop:f * hop + n_fft] * vd, axis=-1) * g[:, f], n=n_fft, axis=-1)
        S[:, f * hop:f * hop + n_fft] += row * vd
        E[f * hop:f * hop + n_fft] += vd * vd
    S, E = S[:, pad:pad + T], E[pad:pad + T]
    return np.where(E > 0, S / np.where(E > 0, E, 1.0), 0.0)


E2E_SHAPES = [dict(id="400-400-160", n_fft=400, L=400, hop=160, T=8000, B=2), dict(id="960-960-480", n_fft=960, L=960, hop=480, T=19200, B=2)]


@pytest.mark.parametrize("shape", E2E_SHAPES, ids=[s["id"] for s in E2E_SHAPES])
def test_end_to_end_against_float64_within_twice_torch(torch, shape):
    """Noise in, the maximum absolute error against the float64 reference at most twice that of
    torch.istft(torch.stft(x, window=v) * g, window=v) in float32 against the same reference."""
    p = B.make_params(B.WIN_BH4, 12, 32)
    n_fft, L, hop, T, nb = (shape[k] for k in ("n_fft", "L", "hop", "T", "B"))
    g_ = torch.Generator(device="cuda").manual_seed(21)
    x = torch.randn((nb, T), device="cuda", generator=g_)
    F, K = 1 + T // hop, n_fft // 2 + 1
    gains = torch.rand((nb, F, K), device="cuda", generator=g_) * 2.0
    v = bhw.window(p, L, dtype=torch.float32)
    got = bhw.stft_mask_istft_mixed(p, x, gains, n_fft, hop, win_length=L, length=T)
    St = torch.stft(x, n_fft, hop, L, window=v, center=True, pad_mode="reflect", return_complex=True)
    yard = torch.istft(St * gains.transpose(-1, -2), n_fft, hop, L, window=v, center=True, length=T)
    ref = _ref64(x.cpu().numpy(), gains.cpu().numpy().astype(np.float64), v.cpu().numpy(), n_fft, hop, L, "reflect", T)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    yerr = float(np.abs(yard.cpu().numpy().astype(np.float64) - ref).max())
    print(f"mask mfft end to end {shape['id']}: fused max abs error {err:.3e}, torch.istft(torch.stft * g) {yerr:.3e}, ratio {err / yerr:.3f}")
    assert got.shape == x.shape and err <= 2.0 * yerr, (err, yerr)


def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    x = torch.zeros((2, 1000), device="cuda")
    m = torch.ones((31,), device="cuda")
    with pytest.raises(ValueError, match="bhw.stft_mixed, a complex multiply and bhw.istft_mixed"):
        bhw.stft_mask_istft_mixed(p, x, m.to(torch.complex64), 60, 16)
    with pytest.raises(ValueError, match="bhw.stft_mask_istft takes it"):
        bhw.stft_mask_istft_mixed(p, x, torch.ones((33,), device="cuda"), 64, 16)
    with pytest.raises(ValueError, match="stft_iq_mixed"):
        bhw.stft_mask_istft_mixed(p, x.to(torch.complex64), m, 60, 16)
    with pytest.raises(ValueError, match="got 2560"):
        bhw.stft_mask_istft_mixed(p, torch.zeros((2, 9000), device="cuda"), torch.ones((1281,), device="cuda"), 2560, 640, win_length=1024)
    with pytest.raises(ValueError, match="2\\^a·3\\^b·5\\^c"):
        bhw.stft_mask_istft_mixed(p, x, torch.ones((12,), device="cuda"), 22, 16)
    with pytest.raises(ValueError, match="broadcast"):
        bhw.stft_mask_istft_mixed(p, x, torch.ones((3, 1, 31), device="cuda"), 60, 16)
    with pytest.raises(ValueError, match=r"\(K,\)"):
        bhw.stft_mask_istft_mixed(p, x, torch.ones((32,), device="cuda"), 60, 16)
    with pytest.raises(ValueError, match="last axis"):
        bhw.stft_mask_istft_mixed(p, x, torch.ones((31, 63), device="cuda").t(), 60, 16)
    with pytest.raises(ValueError, match="float32 CUDA tensor"):
        bhw.stft_mask_istft_mixed(p, x, m.cpu(), 60, 16)
    with pytest.raises(ValueError, match="out must be"):
        bhw.stft_mask_istft_mixed(p, x, m, 60, 16, out=torch.zeros((2, 999), device="cuda"))
    with pytest.raises(ValueError, match="table must be"):
        bhw.stft_mask_istft_mixed(p, x, m, 60, 16, table=object())
    with pytest.raises(B.BhwError, match="overlap"):
        bhw.stft_mask_istft_mixed(p, x, m, 60, 16, out=x)
    out = torch.empty((2, 1000), device="cuda")
    assert bhw.stft_mask_istft_mixed(p, x, m, 60, 16, out=out).data_ptr() == out.data_ptr() and not bool(out.ne(0).any())
    torch.cuda.synchronize()
