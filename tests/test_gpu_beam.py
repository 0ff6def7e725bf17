"""The fused multichannel filter-and-sum kernels on the GPU (bhw_beam_fft_f32_* / bhw_beam_mfft_f32_* through
bhw.stft_beamform_istft / bhw.stft_beamform_istft_mixed).

The gate is exact: for every case of tests/beam_cases.py, library and table form, the output equals WORD FOR WORD (torch.equal on the
int32 views, so the sign of a zero counts) istft*(p, reference(stft*(p, x) per channel, g)) with reference() the contract's separately
rounded float32 products and its float32 sum in ascending channel order -- from the same call arguments.  The properties around it
(sentinels and NaN gaps, one channel against the complex-gain call, batch independence, broadcast weights, NaN locality, unit weights
on one channel, every table instance, graph capture) are held word for word too; one test per family holds the whole chain to float64
within twice torch's own float32 error.

Measured end to end on an MI355X: see DESIGN.md section 45."""
import ctypes

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import beam_cases as BC
import cmask_cases as CC
import table_source_cases as TS

pytestmark = pytest.mark.gpu

SENTINEL = 12345.5
GUARD = 64
NAN = float("nan")


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


def _inputs(torch, nb, C, Tin, F, K, seed=0):
    """x (B, C, T_in) and g (B, C, F, K) of beam_cases' generators, on the device."""
    return torch.from_numpy(BC.inputs(nb, C, Tin, seed)).cuda(), torch.from_numpy(BC.gains(nb, C, F, K, seed)).cuda()


def _layout(g, layout):
    """The weights tensor of a layout, and the same weights expanded to (B, C, F, K)."""
    if layout == "K":
        m = g[0, :, 0].contiguous()
        return m, m[:, None, :].expand(g.shape)
    if layout == "FK":
        m = g[0].contiguous()
    elif layout == "B1K":
        m = g[:, :, 0:1].contiguous()
    else:
        m = g
    return m, m.expand(g.shape)


def _kw(c):
    return dict(win_length=c["L"], center=c["center"], length=BC.geometry(c)[4], normalize=c["normalize"])


def _rows(p, c, x, table=None):
    """The forward call's rows of every channel, (B, C, F, K): the channels as further signals of one stft* call."""
    f = BC.family(c)
    stft = getattr(bhw if table is None else table, f.stft)
    nb, C, T = x.shape
    Y = stft(p, x.reshape(nb * C, T), c["n_fft"], c["hop"], win_length=c["L"], center=c["center"], pad_mode=c["pad_mode"])
    return Y.reshape(nb, C, Y.shape[-2], Y.shape[-1])


def _exact(torch, p, c, x, gfull, table=None):
    """The exact reference: the forward call's rows, the contract in separate float32 operations, the inverse call -- one source."""
    f = BC.family(c)
    istft = getattr(bhw if table is None else table, f.istft)
    return istft(p, BC.reference(_rows(p, c, x, table), gfull), c["n_fft"], c["hop"], **_kw(c))


def _raw_call(torch, p, c, x, gfull, table=None):
    """The C call on the case's own descriptors (padded strides): sentinels around out and in the gaps of its stride, NaN in every gap
    of the channel and batch strides of the input and of all three gain strides (both parts), so a stray read shows in the result."""
    f = BC.family(c)
    sa, ss, L, Tin, T, C, xcs, gs, gcs, gbs = BC.desc(c)
    nb, _, F, K = gfull.shape
    xc = xcs or Tin
    xs, os_ = sa.x_stride or C * xc, ss.x_stride or T
    xbuf = torch.full((nb * xs + C * xc,), NAN, device="cuda")
    xin = torch.as_strided(xbuf, (nb, C, Tin), (xs, xc, 1))
    xin.copy_(x)
    gbuf = torch.full((nb * max(gbs, 1) + C * max(gcs, 1) + F * max(gs, 1) + K,), complex(NAN, NAN), dtype=torch.complex64, device="cuda")
    rows = torch.as_strided(gbuf, (nb if gbs else 1, C, F if gs else 1, K), (gbs, gcs, gs, 1))
    rows.copy_(gfull[:rows.shape[0], :, :rows.shape[2]])
    flat = torch.full((2 * GUARD + nb * os_,), SENTINEL, device="cuda")
    obuf = flat[GUARD:GUARD + nb * os_].view(nb, os_)
    flags = B.OLA_NORMALIZE if c["normalize"] else 0
    dev = x.device.index
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert gbuf.data_ptr() % 8 == 0
    tail = (ctypes.byref(sa), ctypes.byref(ss), flags, ctypes.c_void_p(xbuf.data_ptr()), C, xcs, ctypes.c_void_p(gbuf.data_ptr()), gs, gcs,
            gbs, ctypes.c_void_p(obuf.data_ptr()))
    if table is None:
        B.check(getattr(B.lib(), f.device)(ctypes.byref(p), L, dev, stream, *tail))
    else:
        B.check(getattr(B.lib(), f.from_table)(table._live(), ctypes.byref(p), L, stream, *tail))
    torch.cuda.synchronize()
    assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + nb * os_:] == SENTINEL).all()), "a word around out was written"
    assert bool((obuf[:, T:] == SENTINEL).all()), "a gap of out was written"
    assert int(torch.isnan(xbuf).sum()) == xbuf.numel() - xin.numel() and torch.equal(xin, x)
    assert int(torch.isnan(torch.view_as_real(gbuf)).sum()) == 2 * (gbuf.numel() - rows.numel())
    return obuf[:, :T].contiguous()


def _call(torch, p, c, x, weights, gfull, table=None):
    if c.get("padded") or c["gains"] == "padded":
        return _raw_call(torch, p, c, x, gfull, table)
    return getattr(bhw, BC.family(c).call)(p, x, weights, c["n_fft"], c["hop"], pad_mode=c["pad_mode"], table=table, **_kw(c))


@pytest.mark.parametrize("cid", BC.case_ids())
def test_word_for_word_the_exact_reference(torch, cid):
    c = BC.case(cid)
    p = BC.params(c)
    _, _, _, Tin, T = BC.geometry(c)
    K = c["n_fft"] // 2 + 1
    x, g = _inputs(torch, c["B"], c["C"], Tin, c["F"], K)
    weights, gfull = _layout(g, c["gains"])
    want = _exact(torch, p, c, x, gfull)
    got = _call(torch, p, c, x, weights, gfull)
    assert got.dtype == torch.float32 and tuple(got.shape) == (c["B"], T)
    assert _same(torch, got, want), (cid, "library", _where(torch, got, want), BC.line(c))
    with bhw.ResidentTable(p) as tab:
        d = BC.parse(c, BC.line(c, table=tab._live()))
        assert d["table"] and list(d["kernels"]) == [f"k_beam_{c['family']}_table"], d["line"]
        wt = _exact(torch, p, c, x, gfull, table=tab)
        gt = _call(torch, p, c, x, weights, gfull, table=tab)
        torch.cuda.synchronize()
    assert _same(torch, gt, wt), (cid, "table", _where(torch, gt, wt))
    assert _same(torch, gt, got), "library against table"
    assert bool(torch.isfinite(got).all()) and (T == 0 or int(torch.unique(got.view(torch.int32)).numel()) > min(T, 64) // 2)
    if c["C"] >= 3 and T > 0:
        # the gate tells a wrong order of the sum: the descending sum gives other words through the same inverse call
        P = BC.products(_rows(p, c, x), gfull)
        other = getattr(bhw, BC.family(c).istft)(p, BC.descending(P), c["n_fft"], c["hop"], **_kw(c))
        assert not _same(torch, other, want)


TRIPLES = {}
for _t in TS.TABLES:
    for _w in TS.ROTATION[_t]:
        TRIPLES.setdefault(TS.triple(_t, _w), (_t, _w))
INSTANCE_SHAPES = {"fft": dict(family="fft", n_fft=64, L=57, hop=17, F=24, B=2, C=3, center=True, normalize=True, pad_mode="reflect", setup=None),
                   "mfft": dict(family="mfft", n_fft=60, L=57, hop=17, F=24, B=2, C=3, center=True, normalize=True, pad_mode="reflect", setup=None)}
INSTANCES = [(fam, t) for fam in INSTANCE_SHAPES for t in sorted(TRIPLES)]


@pytest.mark.parametrize("fam,triple", INSTANCES, ids=[f"{fam}-fmt{f}-nt{n}-mode{m}" for fam, (f, n, m) in INSTANCES])
def test_every_table_instance(torch, fam, triple):
    """k_beam_fft_table / k_beam_mfft_table <FMT, NT, MODE> for every triple the tables and weight sets of table_source_cases.py name, at
    n_fft 64 and 60: the describe line names the instance, and the result is the exact reference's from the same table."""
    tname, wname = TRIPLES[triple]
    p = TS.params(tname, wname)
    c = INSTANCE_SHAPES[fam]
    f = BC.family(c)
    n = c["n_fft"]
    L, col0, pad, Tin, T = BC.geometry(c)
    K = n // 2 + 1
    x, g = _inputs(torch, 2, 3, Tin, 24, K, seed=7)
    with bhw.ResidentTable(p, table_format=TS.LIMITS[TS.TABLES[tname][3]]) as tab:
        sa = B.make_stft(2, Tin, 24, 17, n, col0=col0, pad=pad, pad_mode=1, shift=p.dat_width - 1)
        ss = B.make_stft(2, T, 24, 17, n, col0=col0, pad=pad, shift=p.dat_width - 1)
        d = f.cmask.real.parse(f.describe(p, L, sa, ss, 3, normalize=True, g_stride=K, g_ch_stride=24 * K, g_batch_stride=72 * K,
                                          table=tab._live()))
        assert d["kernels"] == {f"k_beam_{fam}_table": tuple(str(v) for v in triple)}, d["line"]
        want = _exact(torch, p, c, x, g, table=tab)
        got = getattr(bhw, f.call)(p, x, g, n, 17, table=tab, **_kw(c))
        torch.cuda.synchronize()
    assert _same(torch, got, want) and bool(torch.isfinite(got).all()), _where(torch, got, want)


PROPERTY_SHAPES = [
    dict(id="fft-small", family="fft", setup=3, n_fft=64, L=49, hop=13, center=True, normalize=True, B=1, C=3, F=40, pad_mode="reflect", gains="BFK"),
    dict(id="fft-large", family="fft", setup=4, n_fft=2048, L=2048, hop=512, center=True, normalize=True, B=1, C=3, F=12, pad_mode="constant",
         gains="BFK"),
    dict(id="mfft-small-odd-M", family="mfft", setup=3, n_fft=90, L=71, hop=13, center=True, normalize=True, B=1, C=3, F=40, pad_mode="reflect",
         gains="BFK"),
    dict(id="mfft-large", family="mfft", setup=4, n_fft=2000, L=2000, hop=500, center=True, normalize=True, B=1, C=3, F=12, pad_mode="constant",
         gains="BFK"),
]
PROPERTY_IDS = [s["id"] for s in PROPERTY_SHAPES]


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=PROPERTY_IDS)
def test_one_channel_is_the_complex_gain_call(torch, shape):
    c = dict(shape, B=3, C=1)
    f = BC.family(c)
    p = BC.params(c)
    _, _, _, Tin, T = BC.geometry(c)
    F, K = c["F"], c["n_fft"] // 2 + 1
    x, g = _inputs(torch, 3, 1, Tin, F, K, seed=3)
    for normalize in (True, False):
        cn = dict(c, normalize=normalize)
        got = _call(torch, p, cn, x, g, g)
        cm = getattr(bhw, f.cmask_call)(p, x[:, 0], g[:, 0], c["n_fft"], c["hop"], pad_mode=c["pad_mode"], **_kw(cn))
        assert _same(torch, got, cm), (normalize, _where(torch, got, cm))
    one = getattr(bhw, f.call)(p, x[1], g[1, :, 0], c["n_fft"], c["hop"], pad_mode=c["pad_mode"], **_kw(c))      # (C, T) and (C, K)
    assert one.dim() == 1
    assert _same(torch, one, getattr(bhw, f.cmask_call)(p, x[1, 0], g[1, 0, 0], c["n_fft"], c["hop"], pad_mode=c["pad_mode"], **_kw(c)))


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=PROPERTY_IDS)
def test_an_output_depends_on_nothing_but_its_frames(torch, shape):
    """A signal alone and as signal 5 of 8; packed against padded strides (NaN in every gap); the (C, K), (C, F, K) and (B, C, 1, K)
    layouts against the same weights materialised to (B, C, F, K); an expand() view against its copy; a conjugate view against its
    copy."""
    c = dict(shape)
    p = BC.params(c)
    call = getattr(bhw, BC.family(c).call)
    _, _, _, Tin, T = BC.geometry(c)
    C, F, K = c["C"], c["F"], c["n_fft"] // 2 + 1
    x, g = _inputs(torch, 8, C, Tin, F, K, seed=5)
    alone = _call(torch, p, c, x[5:6].clone(), g[5:6].clone(), g[5:6])
    batch = _call(torch, p, dict(c, B=8), x, g, g)
    assert _same(torch, alone[0], batch[5])
    assert _same(torch, alone, _exact(torch, p, c, x[5:6], g[5:6]))
    padded = _call(torch, p, dict(c, B=3, padded=True, gains="padded"), x[4:7], None, g[4:7])
    assert _same(torch, padded[1], alone[0])
    for layout in ("K", "FK", "B1K"):
        weights, gfull = _layout(g[2:6], layout)
        assert weights.dim() == {"K": 2, "FK": 3, "B1K": 4}[layout]
        cb = dict(c, B=4)
        lean = _call(torch, p, cb, x[2:6], weights, gfull)
        full = _call(torch, p, cb, x[2:6], gfull.contiguous(), gfull)
        assert _same(torch, lean, full), layout
        view = _call(torch, p, cb, x[2:6], gfull, gfull)                # the expand() view itself: zero strides, nothing materialised
        assert gfull.stride(0) == 0 or gfull.stride(2) == 0
        assert _same(torch, view, full), layout
    one = call(p, x[5], g[5], c["n_fft"], c["hop"], pad_mode=c["pad_mode"], **_kw(c))
    assert one.dim() == 1 and _same(torch, one, alone[0])
    # channels that are a strided view of a wider buffer are read in place
    wide = torch.full((C, Tin + 9), NAN, device="cuda")
    wide[:, :Tin] = x[5]
    assert _same(torch, call(p, wide[:, :Tin], g[5], c["n_fft"], c["hop"], pad_mode=c["pad_mode"], **_kw(c)), one)
    lazy = g[5].conj()
    assert lazy.is_conj()
    assert _same(torch, call(p, x[5], lazy, c["n_fft"], c["hop"], pad_mode=c["pad_mode"], **_kw(c)),
                 call(p, x[5], lazy.resolve_conj(), c["n_fft"], c["hop"], pad_mode=c["pad_mode"], **_kw(c)))
    assert not _same(torch, call(p, x[5], lazy, c["n_fft"], c["hop"], pad_mode=c["pad_mode"], **_kw(c)), one)


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=PROPERTY_IDS)
def test_nan_and_infinity_reach_exactly_the_outputs_under_their_frames(torch, shape):
    c = dict(shape, B=3)
    p = BC.params(c)
    L, col0, pad, Tin, T = BC.geometry(c)
    hop, C, F, K = c["hop"], c["C"], c["F"], c["n_fft"] // 2 + 1
    t0 = pad - col0
    x, g = _inputs(torch, 3, C, Tin, F, K, seed=9)
    for normalize in (True, False):
        cn = dict(c, normalize=normalize)
        clean = _call(torch, p, cn, x, g, g)
        assert bool(torch.isfinite(clean).all())
        f = F // 2
        w = np.arange(T) + t0
        hit = np.zeros((3, T), dtype=bool)
        hit[1] = (w >= f * hop) & (w < f * hop + L)
        assert 0 < hit.sum() <= L
        keep = torch.from_numpy(~hit).cuda()
        for bad, part, ch in ((NAN, "real", 0), (NAN, "imag", C - 1), (float("inf"), "real", 1), (float("inf"), "imag", 1)):
            gn = g.clone()
            getattr(gn, part)[1, ch, f, 5] = bad
            got = _call(torch, p, cn, x, gn, gn)
            assert np.array_equal(~torch.isfinite(got).cpu().numpy(), hit), (normalize, bad, part, ch)
            assert _same(torch, got[keep], clean[keep])
        # a NaN sample of one channel: exactly the outputs under the frames whose window covers it
        for ch in (0, C - 1):
            xn = x.clone()
            ts = Tin // 2
            xn[1, ch, ts] = NAN
            fr = [q for q in range(F) if 0 <= ts + pad - q * hop - col0 < L]
            hx = np.zeros((3, T), dtype=bool)
            for q in fr:
                hx[1] |= (w >= q * hop) & (w < q * hop + L)
            got = _call(torch, p, cn, xn, g, g)
            assert fr and np.array_equal(~torch.isfinite(got).cpu().numpy(), hx), (normalize, ch)
            keepx = torch.from_numpy(~hx).cuda()
            assert _same(torch, got[keepx], clean[keepx])


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=PROPERTY_IDS)
def test_unit_weights_on_one_channel_and_zero_on_the_others_give_that_channels_round_trip(torch, shape):
    """Weights 1 + 0i on channel c and +0 + 0i on the others: the VALUES equal istft*(stft*(x_c)) (float comparison, up to the sign of
    a zero: a product with +0 is a zero of either sign, and added to a zero of the row it may turn that zero's sign; added to anything
    else it changes nothing).  Against the exact reference the words are equal as ever."""
    c = dict(shape, B=2)
    f = BC.family(c)
    p = BC.params(c)
    _, _, _, Tin, T = BC.geometry(c)
    C, F, K = c["C"], c["F"], c["n_fft"] // 2 + 1
    x, _ = _inputs(torch, 2, C, Tin, F, K, seed=17)
    for ch in range(C):
        w = torch.zeros((2, C, F, K), dtype=torch.complex64, device="cuda")
        w[:, ch] = 1.0
        got = _call(torch, p, c, x, w, w)
        back = getattr(bhw, f.istft)(p, _rows(p, c, x)[:, ch], c["n_fft"], c["hop"], **_kw(c))
        assert bool(torch.isfinite(got).all()) and bool((got == back).all()), ch
        assert _same(torch, got, _exact(torch, p, c, x, w)), ch


@pytest.mark.parametrize("fam", list(BC.FAMILIES))
def test_graph_capture(torch, fam):
    """The library form with no warm call, on a shape with several spans per signal; the table form on its first call; one stream, no
    parallel branches."""
    f = BC.FAMILIES[fam]
    call = getattr(bhw, f.call)
    p = B.make_params(B.WIN_BH5, 12, 32)
    n_fft = 512 if fam == "fft" else 400
    L, hop, T, nb, C = 400, 160, 48000, 2, 3
    kw = dict(win_length=L, length=T)
    F, K = 1 + T // hop, n_fft // 2 + 1
    x = torch.from_numpy(BC.inputs(nb, C, T, seed=11)).cuda()
    weights = torch.from_numpy(BC.gains(nb, C, F, K, seed=11)).cuda()
    with bhw.ResidentTable(p) as tab:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                lib = call(p, x, weights, n_fft, hop, **kw)                           # no warm call, no bhw_prepare_device
                tb = call(p, x, weights[0, :, 0], n_fft, hop, table=tab, **kw)        # the table form's first call
        torch.cuda.current_stream().wait_stream(s)
        x.copy_(torch.from_numpy(BC.inputs(nb, C, T, seed=12)).cuda())
        weights.copy_(torch.from_numpy(BC.gains(nb, C, F, K, seed=12)).cuda())
        lib.fill_(-1.0)
        tb.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        le = call(p, x, weights, n_fft, hop, **kw)
        te = call(p, x, weights[0, :, 0], n_fft, hop, table=tab, **kw)
        torch.cuda.synchronize()
    assert _same(torch, lib, le) and _same(torch, tb, te)
    assert not torch.equal(lib, tb) and bool(torch.isfinite(lib).all())


@pytest.mark.parametrize("shape", BC.E2E_SHAPES, ids=[s["id"] for s in BC.E2E_SHAPES])
def test_end_to_end_against_float64_within_twice_torch(torch, shape):
    """Noise in four channels, the maximum absolute error against the float64 reference (beam_cases.ref64) at most twice that of
    torch.istft((torch.stft(x_c) * G_c).sum(c)) evaluated by torch in float32."""
    f = BC.FAMILIES[shape["family"]]
    p = B.make_params(B.WIN_BH4, 12, 32)
    n_fft, L, hop, T, nb, C = (shape[k] for k in ("n_fft", "L", "hop", "T", "B", "C"))
    xn, gn = BC.e2e_inputs(shape)
    x, g = torch.from_numpy(xn).cuda(), torch.from_numpy(gn).cuda()
    v = bhw.window(p, L, dtype=torch.float32)
    got = getattr(bhw, f.call)(p, x, g, n_fft, hop, win_length=L, length=T)
    St = torch.stft(x.reshape(nb * C, T), n_fft, hop, L, window=v, center=True, pad_mode="reflect", return_complex=True)
    St = St.reshape(nb, C, St.shape[-2], St.shape[-1])
    yard = torch.istft((St * g.transpose(-1, -2)).sum(dim=1), n_fft, hop, L, window=v, center=True, length=T)
    ref = BC.ref64(xn, gn, v.cpu().numpy(), n_fft, hop, L)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    yerr = float(np.abs(yard.cpu().numpy().astype(np.float64) - ref).max())
    print(f"beam end to end {shape['id']} C={C}: fused max abs error {err:.3e}, torch.istft((torch.stft * G).sum) {yerr:.3e}, "
          f"ratio {err / yerr:.3f}")
    assert tuple(got.shape) == (nb, T) and err <= 2.0 * yerr, (err, yerr)


def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    x = torch.zeros((2, 3, 1000), device="cuda")
    w = torch.ones((3, 33), dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError, match="broadcast along the channels"):
        bhw.stft_beamform_istft(p, x, w[0:1].expand(3, 33), 64, 16)
    with pytest.raises(ValueError, match="do not broadcast"):
        bhw.stft_beamform_istft(p, x, torch.ones((3, 3, 2, 33), dtype=torch.complex64, device="cuda"), 64, 16)
    with pytest.raises(ValueError, match="last axis"):
        bhw.stft_beamform_istft(p, x, torch.ones((33, 3), dtype=torch.complex64, device="cuda").t(), 64, 16)
    with pytest.raises(ValueError, match="complex64 CUDA tensor"):
        bhw.stft_beamform_istft(p, x, w.cpu(), 64, 16)
    with pytest.raises(ValueError, match="out must be"):
        bhw.stft_beamform_istft(p, x, w, 64, 16, out=torch.zeros((2, 999), device="cuda"))
    with pytest.raises(ValueError, match="table must be"):
        bhw.stft_beamform_istft(p, x, w, 64, 16, table=object())
    with pytest.raises(B.BhwError, match="overlap"):
        bhw.stft_beamform_istft(p, x, w, 64, 16, out=x.view(-1)[1000:3000].view(2, 1000))       # inside channel 1 and 2 of signal 0
    out = torch.empty((2, 1000), device="cuda")
    assert bhw.stft_beamform_istft(p, x, w, 64, 16, out=out).data_ptr() == out.data_ptr() and not bool(out.ne(0).any())
    torch.cuda.synchronize()
