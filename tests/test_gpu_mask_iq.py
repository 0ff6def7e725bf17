"""The fused STFT + real or complex gain + inverse STFT kernels for I/Q input on the GPU (bhw_[c]mask_cfft_f32_* /
bhw_[c]mask_cmfft_f32_* through bhw.stft_mask_istft_iq, bhw.stft_cmask_istft_iq and their _mixed siblings).

The gate is exact: for every case of tests/mask_iq_cases.py, library and table form, the output equals WORD FOR WORD (torch.equal on
the int32 views, so the sign of a zero counts) istft_iq*(p, reference(stft_iq*(p, x), g)) with reference() the separately rounded
float32 products of the contract on the real and imaginary planes -- from the same call arguments.  The properties around it
(sentinels, batch position, broadcast gains and views, shifted gain columns, unit gains, gi = +0 against the real-gain call, a real
signal under a Hermitian mask, NaN locality, graph capture) are held word for word too; one test holds the whole chain to float64
within twice torch's own complex64 error.

Measured end to end on an MI355X: see DESIGN.md section 44."""
import ctypes
import math

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import mask_iq_cases as MC
import table_source_cases as TS

pytestmark = pytest.mark.gpu

SENTINEL = 12345.5
GUARD = 64


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _words(torch, a):
    a = a.contiguous()
    return (torch.view_as_real(a) if a.is_complex() else a).view(torch.int32)


def _same(torch, a, b):
    """Word for word: the int32 views are equal (a +0.0 is not a -0.0, a NaN equals the NaN of the same bits)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_words(torch, a), _words(torch, b))


def _where(torch, a, b):
    d = (_words(torch, a) != _words(torch, b)).nonzero()
    return int(d.shape[0]), d[:4].tolist()


def _values_equal(torch, a, b):
    """== on both parts (a zero of either sign equals a zero), for the comparisons in which a product by +0 may turn a zero's sign."""
    return a.shape == b.shape and bool((torch.view_as_real(a) == torch.view_as_real(b)).all())


def _inputs(torch, nb, Tin, F, K, seed=0, gtype="pair"):
    """x (B, T_in) complex64 fixed-seed noise with an offset; g (B, F, K) from mask_iq_cases.gains."""
    gen = torch.Generator(device="cuda").manual_seed(4400 + seed)
    xr = torch.randn((nb, Tin, 2), device="cuda", generator=gen) * 100.0 + 5.0
    return torch.view_as_complex(xr), torch.from_numpy(MC.gains(nb, F, K, seed, gtype)).cuda()


def _layout(g, layout):
    """The mask tensor of a layout, and the same gains expanded to (B, F, K)."""
    if layout == "K":
        m = g[0, 0].contiguous()
    elif layout == "FK":
        m = g[0].contiguous()
    elif layout == "B1K":
        m = g[:, 0:1].contiguous()
    else:
        m = g
    return m, m.expand(g.shape)


def _kw(c):
    return dict(win_length=c["L"], center=c["center"], length=MC.geometry(c)[4], normalize=c["normalize"])


def _rows(p, c, x, table=None):
    """The forward parent's rows in natural bin order."""
    stft = getattr(bhw if table is None else table, MC.family(c).stft)
    return stft(p, x, c["n_fft"], c["hop"], win_length=c["L"], center=c["center"], pad_mode=c["pad_mode"])


def _exact(torch, p, c, x, gfull, table=None):
    """The exact reference: the forward call's rows, the formula in separate float32 operations, the inverse call -- one source.  Under
    the shift the mask's columns are put in natural order first."""
    istft = getattr(bhw if table is None else table, MC.family(c).istft)
    g = MC.unshift(gfull, c["n_fft"]) if c.get("fftshift") else gfull
    return istft(p, MC.reference(_rows(p, c, x, table), g), c["n_fft"], c["hop"], **_kw(c))


def _raw_call(torch, p, c, x, gfull, table=None):
    """The C call on the case's own descriptors (padded or odd strides): sentinels around out and in the gaps of its stride, NaN in the
    gaps of the input stride and in every gap of the gain strides, so a stray read shows in the result.  odd: both signal buffers begin
    one float off the 8-byte grid.  Returns complex64 (B, T)."""
    sa, ss, L, Tin, T, gs, gbs = MC.desc(c)
    nb, F, K = gfull.shape
    xs, os_ = sa.x_stride or 2 * Tin, ss.x_stride or 2 * T
    off = 1 if c.get("odd") else 0
    xflat = torch.full((off + nb * xs,), float("nan"), device="cuda")
    xbuf = xflat[off:].view(nb, xs)
    xbuf[:, :2 * Tin] = torch.view_as_real(x.contiguous()).reshape(nb, 2 * Tin)
    pair = gfull.is_complex()
    fill = complex(float("nan"), float("nan")) if pair else float("nan")
    gbuf = torch.full((nb * max(gbs, 1) + F * max(gs, 1) + K,), fill, dtype=gfull.dtype, device="cuda")
    rows = torch.as_strided(gbuf, (nb if gbs else 1, F if gs else 1, K), (gbs, gs, 1))
    rows.copy_(gfull[:rows.shape[0], :rows.shape[1]])
    flat = torch.full((2 * GUARD + off + nb * os_,), SENTINEL, device="cuda")
    lo = GUARD + off
    obuf = flat[lo:lo + nb * os_].view(nb, os_)
    flags = (B.OLA_NORMALIZE if c["normalize"] else 0) | (B.CFFT_SHIFT if c.get("fftshift") else 0)
    dev = x.device.index
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert gbuf.data_ptr() % 8 == 0 and (xbuf.data_ptr() % 8 == 4) == bool(off) and (obuf.data_ptr() % 8 == 4) == bool(off)
    tail = (ctypes.byref(sa), ctypes.byref(ss), flags, ctypes.c_void_p(xbuf.data_ptr()), ctypes.c_void_p(gbuf.data_ptr()), gs, gbs,
            ctypes.c_void_p(obuf.data_ptr()))
    stem = "bhw_" + MC.c_name(c["family"], "pair" if pair else "real") + "_f32"
    if table is None:
        B.check(getattr(B.lib(), stem + "_device")(ctypes.byref(p), L, dev, stream, *tail))
    else:
        B.check(getattr(B.lib(), stem + "_from_table")(table._live(), ctypes.byref(p), L, stream, *tail))
    torch.cuda.synchronize()
    assert bool((flat[:lo] == SENTINEL).all()) and bool((flat[lo + nb * os_:] == SENTINEL).all()), "a word around out was written"
    assert bool((obuf[:, 2 * T:] == SENTINEL).all()), "a gap of out was written"
    parts = torch.view_as_real(gbuf) if pair else gbuf
    assert bool(torch.isnan(xbuf[:, 2 * Tin:]).all()) and int(torch.isnan(parts).sum()) == (2 if pair else 1) * (gbuf.numel() - rows.numel())
    return torch.view_as_complex(obuf[:, :2 * T].contiguous().view(nb, T, 2))


def _call(torch, p, c, x, mask, gfull, table=None):
    if c.get("padded") or c.get("odd") or c["gains"] == "padded":
        return _raw_call(torch, p, c, x, gfull, table)
    name = MC.call_name(c["family"], "pair" if gfull.is_complex() else "real")
    return getattr(bhw, name)(p, x, mask, c["n_fft"], c["hop"], pad_mode=c["pad_mode"], fftshift=bool(c.get("fftshift")), table=table, **_kw(c))


@pytest.mark.parametrize("cid", MC.case_ids())
def test_word_for_word_the_exact_reference(torch, cid):
    c = MC.case(cid)
    p = MC.params(c)
    _, _, _, Tin, T = MC.geometry(c)
    x, g = _inputs(torch, c["B"], Tin, c["F"], c["n_fft"], gtype=c["gtype"])
    mask, gfull = _layout(g, c["gains"])
    want = _exact(torch, p, c, x, gfull)
    got = _call(torch, p, c, x, mask, gfull)
    assert got.dtype == torch.complex64 and tuple(got.shape) == (c["B"], T)
    assert _same(torch, got, want), (cid, "library", _where(torch, got, want), MC.line(c))
    with bhw.ResidentTable(p) as tab:
        d = MC.parse(c, MC.line(c, table=tab._live()))
        assert d["table"] and list(d["kernels"]) == [f"k_{MC.c_name(c['family'], c['gtype'])}_table"], d["line"]
        wt = _exact(torch, p, c, x, gfull, table=tab)
        gt = _call(torch, p, c, x, mask, gfull, table=tab)
        torch.cuda.synchronize()
    assert _same(torch, gt, wt), (cid, "table", _where(torch, gt, wt))
    assert _same(torch, gt, got), "library against table"
    parts = torch.view_as_real(got)
    assert bool(torch.isfinite(parts).all()) and (T == 0 or int(torch.unique(parts.view(torch.int32)).numel()) > min(T, 64) // 2)


TRIPLES = {}
for _t in TS.TABLES:
    for _w in TS.ROTATION[_t]:
        TRIPLES.setdefault(TS.triple(_t, _w), (_t, _w))
INSTANCE_SHAPES = {"cfft": dict(family="cfft", n_fft=64, L=57, hop=17, F=24, B=2, center=True, normalize=True, pad_mode="reflect", setup=None),
                   "cmfft": dict(family="cmfft", n_fft=75, L=57, hop=17, F=24, B=2, center=True, normalize=True, pad_mode="reflect", setup=None)}
INSTANCES = [(fam, t) for fam in INSTANCE_SHAPES for t in sorted(TRIPLES)]


@pytest.mark.parametrize("fam,triple", INSTANCES, ids=[f"{fam}-fmt{f}-nt{n}-mode{m}" for fam, (f, n, m) in INSTANCES])
def test_every_table_instance(torch, fam, triple):
    """k_[c]mask_cfft_table / k_[c]mask_cmfft_table <FMT, NT, MODE> for every triple the tables and weight sets of
    table_source_cases.py name, at n_fft 64 and 75 (4x4x4, and 5x5x3: more than one pass of a radix kind), both gain types: the describe
    line names the instance, and the result is the exact reference's from the same table."""
    tname, wname = TRIPLES[triple]
    p = TS.params(tname, wname)
    c = INSTANCE_SHAPES[fam]
    n = c["n_fft"]
    L, col0, pad, Tin, T = MC.geometry(c)
    with bhw.ResidentTable(p, table_format=TS.LIMITS[TS.TABLES[tname][3]]) as tab:
        sa = B.make_stft(2, Tin, 24, 17, n, col0=col0, pad=pad, pad_mode=1, channels=2, shift=p.dat_width - 1)
        ss = B.make_stft(2, T, 24, 17, n, col0=col0, pad=pad, channels=2, shift=p.dat_width - 1)
        for gtype in MC.GTYPES:
            x, g = _inputs(torch, 2, Tin, 24, n, seed=7, gtype=gtype)
            text = MC.describe(fam, gtype)(p, L, sa, ss, normalize=True, g_stride=n, g_batch_stride=24 * n, table=tab._live())
            d = MC.parse(c, text)
            assert d["kernels"] == {f"k_{MC.c_name(fam, gtype)}_table": tuple(str(v) for v in triple)}, text
            want = _exact(torch, p, c, x, g, table=tab)
            got = getattr(bhw, MC.call_name(fam, gtype))(p, x, g, n, 17, table=tab, **_kw(c))
            torch.cuda.synchronize()
            assert _same(torch, got, want) and bool(torch.isfinite(torch.view_as_real(got)).all()), (gtype, _where(torch, got, want))


PROPERTY_SHAPES = [
    dict(id="cfft-small", family="cfft", setup=3, n_fft=64, L=49, hop=13, center=True, normalize=True, B=1, F=40, pad_mode="reflect", gains="BFK"),
    dict(id="cfft-large", family="cfft", setup=4, n_fft=2048, L=2048, hop=512, center=True, normalize=True, B=1, F=24, pad_mode="constant",
         gains="BFK"),
    dict(id="cmfft-small-odd", family="cmfft", setup=3, n_fft=75, L=61, hop=13, center=True, normalize=True, B=1, F=40, pad_mode="reflect",
         gains="BFK"),
    dict(id="cmfft-large", family="cmfft", setup=4, n_fft=2000, L=2000, hop=500, center=True, normalize=True, B=1, F=24, pad_mode="constant",
         gains="BFK"),
]
PROPERTY_IDS = [s["id"] for s in PROPERTY_SHAPES]


@pytest.mark.parametrize("gtype", MC.GTYPES)
@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=PROPERTY_IDS)
def test_an_output_depends_on_nothing_but_its_frames(torch, shape, gtype):
    """A signal alone and as signal 37 of 64; packed against padded strides (NaN in every gap); the (K,), (F, K) and (B, 1, K) layouts
    against the same gains materialised to (B, F, K); an expand() view against its copy; a conjugate view against its copy."""
    c = dict(shape)
    p = MC.params(c)
    call = getattr(bhw, MC.call_name(c["family"], gtype))
    _, _, _, Tin, T = MC.geometry(c)
    F, K = c["F"], c["n_fft"]
    x, g = _inputs(torch, 64, Tin, F, K, seed=5, gtype=gtype)
    alone = _call(torch, p, c, x[37:38].clone(), g[37:38].clone(), g[37:38])
    batch = _call(torch, p, dict(c, B=64), x, g, g)
    assert _same(torch, alone[0], batch[37])
    assert _same(torch, alone, _exact(torch, p, c, x[37:38], g[37:38]))
    padded = _call(torch, p, dict(c, B=5, padded=True, gains="padded"), x[35:40], None, g[35:40])
    assert _same(torch, padded[2], alone[0])
    odd = _call(torch, p, dict(c, B=5, odd=True), x[35:40], None, g[35:40])               # 4-byte loads and stores
    assert _same(torch, odd[2], alone[0])
    for layout in ("K", "FK", "B1K"):
        mask, gfull = _layout(g[30:34], layout)
        assert mask.dim() == {"K": 1, "FK": 2, "B1K": 3}[layout]
        cb = dict(c, B=4)
        lean = _call(torch, p, cb, x[30:34], mask, gfull)
        full = _call(torch, p, cb, x[30:34], gfull.contiguous(), gfull)
        assert _same(torch, lean, full), layout
        view = _call(torch, p, cb, x[30:34], gfull, gfull)              # the expand() view itself: zero strides, nothing materialised
        assert gfull.stride(0) == 0 or gfull.stride(1) == 0
        assert _same(torch, view, full), layout
    kw = dict(pad_mode=c["pad_mode"], **_kw(c))
    one = call(p, x[37], g[37], c["n_fft"], c["hop"], **kw)
    assert one.dim() == 1 and _same(torch, one, alone[0])
    if gtype == "pair":
        lazy = g[37].conj()
        assert lazy.is_conj()
        assert _same(torch, call(p, x[37], lazy, c["n_fft"], c["hop"], **kw), call(p, x[37], lazy.resolve_conj(), c["n_fft"], c["hop"], **kw))
        assert not _same(torch, call(p, x[37], lazy, c["n_fft"], c["hop"], **kw), one)
    xl = x[37].conj()                                                       # a lazily conjugated signal is resolved too
    assert xl.is_conj() and _same(torch, call(p, xl, g[37], c["n_fft"], c["hop"], **kw), call(p, xl.resolve_conj(), g[37], c["n_fft"], c["hop"], **kw))


@pytest.mark.parametrize("gtype", MC.GTYPES)
@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=PROPERTY_IDS)
def test_shifted_gain_columns_are_a_load_index(torch, shape, gtype):
    """fftshift=True with the mask on a centred axis (torch.fft.fftshift of the gains) == fftshift=False with the gains in order, at an
    even and an odd n_fft, word for word; and the shifted call with the unshifted mask differs."""
    c = dict(shape, B=2)
    p = MC.params(c)
    call = getattr(bhw, MC.call_name(c["family"], gtype))
    _, _, _, Tin, T = MC.geometry(c)
    n = c["n_fft"]
    x, g = _inputs(torch, 2, Tin, c["F"], n, seed=21, gtype=gtype)
    kw = dict(pad_mode=c["pad_mode"], **_kw(c))
    plain = call(p, x, g, n, c["hop"], **kw)
    centred = torch.fft.fftshift(g, dim=-1).contiguous()
    assert torch.equal(MC.unshift(centred, n), g) and torch.equal(centred[..., n // 2], g[..., 0])
    assert _same(torch, call(p, x, centred, n, c["hop"], fftshift=True, **kw), plain)
    assert not _same(torch, call(p, x, g, n, c["hop"], fftshift=True, **kw), plain)
    with bhw.ResidentTable(p) as tab:
        assert _same(torch, call(p, x, centred, n, c["hop"], fftshift=True, table=tab, **kw), plain)
        torch.cuda.synchronize()


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=PROPERTY_IDS)
def test_unit_gains_give_the_round_trip_and_zero_imaginary_parts_the_real_call(torch, shape):
    """Gains 1: istft_iq*(stft_iq*(x)) word for word (fl32(y * 1) is y).  Gains 1 + 0i, and gi = +0 everywhere against the real-gain call
    with gr: == on finite data (a float comparison: fl32(im * +0) is a zero of either sign, which may turn the sign of a zero sum)."""
    c = dict(shape, B=3)
    f = MC.family(c)
    p = MC.params(c)
    _, _, _, Tin, T = MC.geometry(c)
    F, n = c["F"], c["n_fft"]
    x, g = _inputs(torch, 3, Tin, F, n, seed=17)
    gr = g.real.contiguous()
    g0 = torch.complex(gr, torch.zeros_like(gr))
    for normalize in (True, False):
        cn = dict(c, normalize=normalize)
        back = getattr(bhw, f.istft)(p, _rows(p, cn, x), n, c["hop"], **_kw(cn))
        ones = torch.ones_like(gr)
        assert _same(torch, _call(torch, p, cn, x, ones, ones), back), normalize
        cones = torch.ones_like(g)
        unit = _call(torch, p, cn, x, cones, cones)
        assert _values_equal(torch, unit, back) and _same(torch, unit, _exact(torch, p, cn, x, cones)), normalize
        got = _call(torch, p, cn, x, g0, g0)
        real = _call(torch, p, cn, x, gr, gr)
        assert bool(torch.isfinite(torch.view_as_real(got)).all()) and _values_equal(torch, got, real), normalize
        assert _same(torch, got, _exact(torch, p, cn, x, g0)) and _same(torch, real, _exact(torch, p, cn, x, gr))


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=PROPERTY_IDS)
def test_a_real_signal_under_a_hermitian_mask_stays_real(torch, shape):
    """A purely real x with G[k] = conj(G[(n - k) % n]): the imaginary part of the output is rounding error alone, at most
    MC.REAL_SIGNAL_FACTOR * 2^-24 * log2(n_fft) times the signal's largest output magnitude (the bound and its reasons:
    mask_iq_cases.real_signal_bound; tests/test_mask_iq_cases.py holds the CPU stand-in to it first)."""
    c = dict(shape, B=2)
    p = MC.params(c)
    _, _, _, Tin, T = MC.geometry(c)
    n = c["n_fft"]
    xn, gn = MC.real_signal_inputs(2, Tin, c["F"], n)
    x, g = torch.from_numpy(xn).cuda(), torch.from_numpy(gn).cuda()
    got = _call(torch, p, c, x, g, g)
    assert _same(torch, got, _exact(torch, p, c, x, g))
    mag = got.abs().amax(dim=-1)
    worst = got.imag.abs().amax(dim=-1)
    bound = MC.real_signal_bound(n, mag.cpu().numpy())
    print(f"real signal {shape['id']}: max |imag| / (2^-24 log2 n max |out|) = {(worst / mag).max().item() / (2.0 ** -24 * math.log2(n)):.3f}")
    assert bool((mag > 1.0).all()) and bool((worst.cpu().numpy() <= bound).all()), (worst.tolist(), bound.tolist())


@pytest.mark.parametrize("gtype", MC.GTYPES)
@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=PROPERTY_IDS)
def test_nan_and_infinity_reach_exactly_the_outputs_under_their_frames(torch, shape, gtype):
    c = dict(shape, B=3)
    p = MC.params(c)
    L, col0, pad, Tin, T = MC.geometry(c)
    hop, F, n = c["hop"], c["F"], c["n_fft"]
    t0 = pad - col0
    x, g = _inputs(torch, 3, Tin, F, n, seed=9, gtype=gtype)

    def bad_of(out):                                     # an output is hit when either part is not finite; both parts must be
        nf = ~torch.isfinite(torch.view_as_real(out))
        assert torch.equal(nf[..., 0], nf[..., 1]), "one part of an output is finite, the other is not"
        return nf[..., 0].cpu().numpy()

    for normalize in (True, False):
        cn = dict(c, normalize=normalize)
        clean = _call(torch, p, cn, x, g, g)
        assert not bad_of(clean).any()
        f = F // 2
        w = np.arange(T) + t0
        hit = np.zeros((3, T), dtype=bool)
        hit[1] = (w >= f * hop) & (w < f * hop + L)
        assert 0 < hit.sum() <= L
        keep = torch.from_numpy(~hit).cuda()
        for bad in (float("nan"), float("inf")):
            for part in (("real", "imag") if gtype == "pair" else ("real",)):
                gn = g.clone()
                (getattr(gn, part) if gtype == "pair" else gn)[1, f, 5] = bad
                got = _call(torch, p, cn, x, gn, gn)
                assert np.array_equal(bad_of(got), hit), (normalize, bad, part)
                assert _same(torch, got[keep], clean[keep])
        # a NaN or an infinity in one part of one sample: exactly the outputs under the frames whose window covers it
        ts = Tin // 2
        fr = [q for q in range(F) if 0 <= ts + pad - q * hop - col0 < L]
        hx = np.zeros((3, T), dtype=bool)
        for q in fr:
            hx[1] |= (w >= q * hop) & (w < q * hop + L)
        keep = torch.from_numpy(~hx).cuda()
        for bad, part in ((float("nan"), 0), (float("inf"), 1)):
            xn = x.clone()
            torch.view_as_real(xn)[1, ts, part] = bad
            got = _call(torch, p, cn, xn, g, g)
            assert fr and np.array_equal(bad_of(got), hx), (normalize, bad, part)
            assert _same(torch, got[keep], clean[keep])


@pytest.mark.parametrize("fam", list(MC.FAMILIES))
def test_graph_capture(torch, fam):
    """The library form with no warm call, on a shape with several spans per signal; the table form on its first call; one stream, no
    parallel branches; pair gains in the library form and real gains in the table form."""
    p = B.make_params(B.WIN_BH5, 12, 32)
    n_fft = 512 if fam == "cfft" else 400
    L, hop, T, nb = 400, 160, 48000, 4
    kw = dict(win_length=L, length=T)
    x, _ = _inputs(torch, nb, T, 1, 1, seed=11)
    F = 1 + T // hop
    sa = B.make_stft(nb, T, F, hop, n_fft, col0=(n_fft - L) // 2, pad=n_fft // 2, pad_mode=1, channels=2, shift=31)
    ss = B.make_stft(nb, T, F, hop, n_fft, col0=(n_fft - L) // 2, pad=n_fft // 2, channels=2, shift=31)
    c = dict(family=fam)
    assert MC.parse(c, MC.describe(fam, "pair")(p, L, sa, ss, normalize=True, g_stride=n_fft, g_batch_stride=F * n_fft))["spans"] > 2
    cmask = torch.from_numpy(MC.gains(nb, F, n_fft, seed=11)).cuda()
    rmask = torch.from_numpy(MC.gains(1, 1, n_fft, seed=11, gtype="real")[0, 0]).cuda()
    ccall, rcall = getattr(bhw, MC.call_name(fam, "pair")), getattr(bhw, MC.call_name(fam, "real"))
    with bhw.ResidentTable(p) as tab:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                lib = ccall(p, x, cmask, n_fft, hop, **kw)                             # no warm call, no bhw_prepare_device
                tb = rcall(p, x, rmask, n_fft, hop, table=tab, **kw)                   # the table form's first call
        torch.cuda.current_stream().wait_stream(s)
        x.copy_(_inputs(torch, nb, T, 1, 1, seed=12)[0])
        cmask.copy_(torch.from_numpy(MC.gains(nb, F, n_fft, seed=12)).cuda())
        rmask.copy_(torch.from_numpy(MC.gains(1, 1, n_fft, seed=12, gtype="real")[0, 0]).cuda())
        lib.fill_(-1.0)
        tb.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        le = ccall(p, x, cmask, n_fft, hop, **kw)
        te = rcall(p, x, rmask, n_fft, hop, table=tab, **kw)
        torch.cuda.synchronize()
    assert _same(torch, lib, le) and _same(torch, tb, te)
    assert not torch.equal(lib, tb) and bool(torch.isfinite(torch.view_as_real(lib)).all())


@pytest.mark.parametrize("gtype", MC.GTYPES)
@pytest.mark.parametrize("shape", MC.E2E_SHAPES, ids=[s["id"] for s in MC.E2E_SHAPES])
def test_end_to_end_against_float64_within_twice_torch(torch, shape, gtype):
    """Complex noise in, the maximum absolute error against the float64 reference torch.istft(torch.stft(x128, onesided=False) * G128)
    at most twice that of the same expression evaluated by torch in complex64."""
    p = B.make_params(B.WIN_BH4, 12, 32)
    n_fft, L, hop, T = (shape[k] for k in ("n_fft", "L", "hop", "T"))
    xn, gn = MC.e2e_inputs(shape, gtype)
    x, g = torch.from_numpy(xn).cuda(), torch.from_numpy(gn).cuda()
    v = bhw.window(p, L, dtype=torch.float32)
    got = getattr(bhw, MC.call_name(shape["family"], gtype))(p, x, g, n_fft, hop, win_length=L, length=T)

    def chain(xx, vv, gg):
        S = torch.stft(xx, n_fft, hop, L, window=vv, center=True, pad_mode="reflect", onesided=False, return_complex=True)
        return torch.istft(S * gg.transpose(-1, -2), n_fft, hop, L, window=vv, center=True, length=T, onesided=False, return_complex=True)

    yard = chain(x, v, g)
    ref = chain(x.to(torch.complex128), v.double(), g.to(torch.complex128) if gtype == "pair" else g.double())
    err = float((got.to(torch.complex128) - ref).abs().max())
    yerr = float((yard.to(torch.complex128) - ref).abs().max())
    print(f"mask iq end to end {shape['id']} {gtype}: fused max abs error {err:.3e}, torch.istft(torch.stft * G) {yerr:.3e}, ratio {err / yerr:.3f}")
    assert got.shape == x.shape and yard.dtype == torch.complex64 and err <= 2.0 * yerr, (err, yerr)


def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    x = torch.zeros((2, 1000), dtype=torch.complex64, device="cuda")
    m = torch.ones((64,), dtype=torch.complex64, device="cuda")
    r = torch.ones((64,), device="cuda")
    with pytest.raises(ValueError, match="bhw.stft_mask_istft_iq takes real gains"):
        bhw.stft_cmask_istft_iq(p, x, r, 64, 16)
    with pytest.raises(ValueError, match="bhw.stft_cmask_istft_iq takes complex gains"):
        bhw.stft_mask_istft_iq(p, x, m, 64, 16)
    with pytest.raises(ValueError, match="bhw.stft_cmask_istft_iq_mixed takes it"):
        bhw.stft_cmask_istft_iq(p, x, torch.ones((60,), dtype=torch.complex64, device="cuda"), 60, 16)
    with pytest.raises(ValueError, match="bhw.stft_mask_istft_iq takes it"):
        bhw.stft_mask_istft_iq_mixed(p, x, r, 64, 16)
    with pytest.raises(ValueError, match="bhw.stft_cmask_istft takes a real signal"):
        bhw.stft_cmask_istft_iq(p, x.real.contiguous(), m, 64, 16)
    with pytest.raises(ValueError, match="bhw.stft_mask_istft_mixed takes a real signal"):
        bhw.stft_mask_istft_iq_mixed(p, x.real.contiguous(), torch.ones((60,), device="cuda"), 60, 16)
    with pytest.raises(ValueError, match="no fused I/Q transform takes it"):
        bhw.stft_mask_istft_iq(p, torch.zeros((2, 9000), dtype=torch.complex64, device="cuda"), torch.ones((4096,), device="cuda"), 4096, 16)
    with pytest.raises(ValueError, match="broadcast"):
        bhw.stft_cmask_istft_iq(p, x, torch.ones((3, 1, 64), dtype=torch.complex64, device="cuda"), 64, 16)
    with pytest.raises(ValueError, match=r"K = n_fft = 64"):
        bhw.stft_cmask_istft_iq(p, x, torch.ones((33,), dtype=torch.complex64, device="cuda"), 64, 16)
    with pytest.raises(ValueError, match="last axis"):
        bhw.stft_cmask_istft_iq(p, x, torch.ones((64, 63), dtype=torch.complex64, device="cuda").t(), 64, 16)
    with pytest.raises(ValueError, match="complex64 CUDA tensor"):
        bhw.stft_cmask_istft_iq(p, x, m.cpu(), 64, 16)
    with pytest.raises(ValueError, match="win_length < n_fft"):
        bhw.stft_cmask_istft_iq(p, x, m, 64, 16, win_length=50, center=False)
    with pytest.raises(ValueError, match="out must be"):
        bhw.stft_cmask_istft_iq(p, x, m, 64, 16, out=torch.zeros((2, 999), dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError, match="table must be"):
        bhw.stft_cmask_istft_iq(p, x, m, 64, 16, table=object())
    with pytest.raises(B.BhwError, match="overlap"):
        bhw.stft_cmask_istft_iq(p, x, m, 64, 16, out=x)
    out = torch.empty((2, 1000), dtype=torch.complex64, device="cuda")
    assert bhw.stft_cmask_istft_iq(p, x, m, 64, 16, out=out).data_ptr() == out.data_ptr() and not bool(torch.view_as_real(out).ne(0).any())
    torch.cuda.synchronize()
