"""The fused STFT + complex gain + inverse STFT kernels on the GPU (bhw_cmask_fft_f32_* / bhw_cmask_mfft_f32_* through
bhw.stft_cmask_istft / bhw.stft_cmask_istft_mixed).

The gate is exact: for every case of tests/cmask_cases.py, library and table form, the output equals WORD FOR WORD (torch.equal on the
int32 views, so the sign of a zero counts) istft*(p, reference(stft*(p, x), g)) with reference() the four separately rounded float32
products of the contract on the real and imaginary planes -- from the same call arguments.  The properties around it (sentinels, batch
independence, broadcast gains, bins 0 and n_fft / 2, NaN locality, gi = +0 against the real call, unit gains, graph capture) are held
word for word too; one test holds the whole chain to float64 within twice torch's own float32 error.

Measured end to end on an MI355X (maximum absolute error against float64, fused / torch.istft(torch.stft * G) in float32): see
DESIGN.md section 43."""
import ctypes

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import cmask_cases as CC
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
    """x (B, T_in) fixed-seed noise with an offset; g (B, F, K) complex64 from cmask_cases.gains."""
    gen = torch.Generator(device="cuda").manual_seed(4300 + seed)
    x = torch.randn((nb, Tin), device="cuda", generator=gen) * 100.0 + 5.0
    return x, torch.from_numpy(CC.gains(nb, F, K, seed)).cuda()


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
    return dict(win_length=c["L"], center=c["center"], length=CC.geometry(c)[4], normalize=c["normalize"])


def _rows(p, c, x, table=None):
    f = CC.family(c)
    stft = getattr(bhw if table is None else table, f.stft)
    return stft(p, x, c["n_fft"], c["hop"], win_length=c["L"], center=c["center"], pad_mode=c["pad_mode"])


def _exact(torch, p, c, x, gfull, table=None):
    """The exact reference: the forward call's rows, the formula in separate float32 operations, the inverse call -- one source."""
    f = CC.family(c)
    istft = getattr(bhw if table is None else table, f.istft)
    return istft(p, CC.reference(_rows(p, c, x, table), gfull), c["n_fft"], c["hop"], **_kw(c))


def _raw_call(torch, p, c, x, gfull, table=None):
    """The C call on the case's own descriptors (padded strides): sentinels around out and in the gaps of its stride, NaN in the gaps of
    the input stride and in every gap of the gain strides (both parts), so a stray read shows in the result.  Returns (B, T)."""
    f = CC.family(c)
    sa, ss, L, Tin, T, gs, gbs = CC.desc(c)
    nb, F, K = gfull.shape
    xs, os_ = sa.x_stride or Tin, ss.x_stride or T
    xbuf = torch.full((nb, xs), float("nan"), device="cuda")
    xbuf[:, :Tin] = x
    gbuf = torch.full((nb * max(gbs, 1) + F * max(gs, 1) + K,), complex(float("nan"), float("nan")), dtype=torch.complex64, device="cuda")
    rows = torch.as_strided(gbuf, (nb if gbs else 1, F if gs else 1, K), (gbs, gs, 1))
    rows.copy_(gfull[:rows.shape[0], :rows.shape[1]])
    flat = torch.full((2 * GUARD + nb * os_,), SENTINEL, device="cuda")
    obuf = flat[GUARD:GUARD + nb * os_].view(nb, os_)
    flags = B.OLA_NORMALIZE if c["normalize"] else 0
    dev = x.device.index
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert gbuf.data_ptr() % 8 == 0
    tail = (ctypes.byref(sa), ctypes.byref(ss), flags, ctypes.c_void_p(xbuf.data_ptr()), ctypes.c_void_p(gbuf.data_ptr()), gs, gbs,
            ctypes.c_void_p(obuf.data_ptr()))
    if table is None:
        B.check(getattr(B.lib(), f.device)(ctypes.byref(p), L, dev, stream, *tail))
    else:
        B.check(getattr(B.lib(), f.from_table)(table._live(), ctypes.byref(p), L, stream, *tail))
    torch.cuda.synchronize()
    assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + nb * os_:] == SENTINEL).all()), "a word around out was written"
    assert bool((obuf[:, T:] == SENTINEL).all()), "a gap of out was written"
    parts = torch.view_as_real(gbuf)
    assert bool(torch.isnan(xbuf[:, Tin:]).all()) and int(torch.isnan(parts).sum()) == 2 * (gbuf.numel() - rows.numel())
    return obuf[:, :T].contiguous()


def _call(torch, p, c, x, mask, gfull, table=None):
    if c.get("padded") or c["gains"] == "padded":
        return _raw_call(torch, p, c, x, gfull, table)
    return getattr(bhw, CC.family(c).call)(p, x, mask, c["n_fft"], c["hop"], pad_mode=c["pad_mode"], table=table, **_kw(c))


@pytest.mark.parametrize("cid", CC.case_ids())
def test_word_for_word_the_exact_reference(torch, cid):
    c = CC.case(cid)
    p = CC.params(c)
    _, _, _, Tin, T = CC.geometry(c)
    K = c["n_fft"] // 2 + 1
    x, g = _inputs(torch, c["B"], Tin, c["F"], K)
    mask, gfull = _layout(g, c["gains"])
    want = _exact(torch, p, c, x, gfull)
    got = _call(torch, p, c, x, mask, gfull)
    assert got.dtype == torch.float32 and tuple(got.shape) == (c["B"], T)
    assert _same(torch, got, want), (cid, "library", _where(torch, got, want), CC.line(c))
    with bhw.ResidentTable(p) as tab:
        d = CC.parse(c, CC.line(c, table=tab._live()))
        assert d["table"] and list(d["kernels"]) == [f"k_cmask_{c['family']}_table"], d["line"]
        wt = _exact(torch, p, c, x, gfull, table=tab)
        gt = _call(torch, p, c, x, mask, gfull, table=tab)
        torch.cuda.synchronize()
    assert _same(torch, gt, wt), (cid, "table", _where(torch, gt, wt))
    assert _same(torch, gt, got), "library against table"
    assert bool(torch.isfinite(got).all()) and (T == 0 or int(torch.unique(got.view(torch.int32)).numel()) > min(T, 64) // 2)


TRIPLES = {}
for _t in TS.TABLES:
    for _w in TS.ROTATION[_t]:
        TRIPLES.setdefault(TS.triple(_t, _w), (_t, _w))
INSTANCE_SHAPES = {"fft": dict(family="fft", n_fft=64, L=57, hop=17, F=24, B=2, center=True, normalize=True, pad_mode="reflect", setup=None),
                   "mfft": dict(family="mfft", n_fft=60, L=57, hop=17, F=24, B=2, center=True, normalize=True, pad_mode="reflect", setup=None)}
INSTANCES = [(fam, t) for fam in INSTANCE_SHAPES for t in sorted(TRIPLES)]


@pytest.mark.parametrize("fam,triple", INSTANCES, ids=[f"{fam}-fmt{f}-nt{n}-mode{m}" for fam, (f, n, m) in INSTANCES])
def test_every_table_instance(torch, fam, triple):
    """k_cmask_fft_table / k_cmask_mfft_table <FMT, NT, MODE> for every triple the tables and weight sets of table_source_cases.py name,
    at n_fft 64 and 60: the describe line names the instance, and the result is the exact reference's from the same table."""
    tname, wname = TRIPLES[triple]
    p = TS.params(tname, wname)
    c = INSTANCE_SHAPES[fam]
    f = CC.family(c)
    n = c["n_fft"]
    L, col0, pad, Tin, T = CC.geometry(c)
    K = n // 2 + 1
    x, g = _inputs(torch, 2, Tin, 24, K, seed=7)
    with bhw.ResidentTable(p, table_format=TS.LIMITS[TS.TABLES[tname][3]]) as tab:
        sa = B.make_stft(2, Tin, 24, 17, n, col0=col0, pad=pad, pad_mode=1, shift=p.dat_width - 1)
        ss = B.make_stft(2, T, 24, 17, n, col0=col0, pad=pad, shift=p.dat_width - 1)
        d = f.real.parse(f.describe(p, L, sa, ss, normalize=True, g_stride=K, g_batch_stride=24 * K, table=tab._live()))
        assert d["kernels"] == {f"k_cmask_{fam}_table": tuple(str(v) for v in triple)}, d["line"]
        want = _exact(torch, p, c, x, g, table=tab)
        got = getattr(bhw, f.call)(p, x, g, n, 17, table=tab, **_kw(c))
        torch.cuda.synchronize()
    assert _same(torch, got, want) and bool(torch.isfinite(got).all()), _where(torch, got, want)


PROPERTY_SHAPES = [
    dict(id="fft-small", family="fft", setup=3, n_fft=64, L=49, hop=13, center=True, normalize=True, B=1, F=40, pad_mode="reflect", gains="BFK"),
    dict(id="fft-large", family="fft", setup=4, n_fft=2048, L=2048, hop=512, center=True, normalize=True, B=1, F=24, pad_mode="constant", gains="BFK"),
    dict(id="mfft-small-odd-M", family="mfft", setup=3, n_fft=90, L=71, hop=13, center=True, normalize=True, B=1, F=40, pad_mode="reflect",
         gains="BFK"),
    dict(id="mfft-large", family="mfft", setup=4, n_fft=2000, L=2000, hop=500, center=True, normalize=True, B=1, F=24, pad_mode="constant",
         gains="BFK"),
]
PROPERTY_IDS = [s["id"] for s in PROPERTY_SHAPES]


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=PROPERTY_IDS)
def test_an_output_depends_on_nothing_but_its_frames(torch, shape):
    """A signal alone and as signal 37 of 64; packed against padded strides (NaN pairs in every gap); the (K,), (F, K) and (B, 1, K)
    layouts against the same gains materialised to (B, F, K); an expand() view against its copy; a conjugate view against its copy."""
    c = dict(shape)
    p = CC.params(c)
    call = getattr(bhw, CC.family(c).call)
    _, _, _, Tin, T = CC.geometry(c)
    F, K = c["F"], c["n_fft"] // 2 + 1
    x, g = _inputs(torch, 64, Tin, F, K, seed=5)
    alone = _call(torch, p, c, x[37:38].clone(), g[37:38].clone(), g[37:38])
    batch = _call(torch, p, dict(c, B=64), x, g, g)
    assert _same(torch, alone[0], batch[37])
    assert _same(torch, alone, _exact(torch, p, c, x[37:38], g[37:38]))
    padded = _call(torch, p, dict(c, B=5, padded=True, gains="padded"), x[35:40], None, g[35:40])
    assert _same(torch, padded[2], alone[0])
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
    one = call(p, x[37], g[37], c["n_fft"], c["hop"], pad_mode=c["pad_mode"], **_kw(c))
    assert one.dim() == 1 and _same(torch, one, alone[0])
    lazy = g[37].conj()
    assert lazy.is_conj()
    assert _same(torch, call(p, x[37], lazy, c["n_fft"], c["hop"], pad_mode=c["pad_mode"], **_kw(c)),
                 call(p, x[37], lazy.resolve_conj(), c["n_fft"], c["hop"], pad_mode=c["pad_mode"], **_kw(c)))
    assert not _same(torch, call(p, x[37], lazy, c["n_fft"], c["hop"], pad_mode=c["pad_mode"], **_kw(c)), one)


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=PROPERTY_IDS)
def test_the_imaginary_gain_parts_at_bin_0_and_the_last_bin_do_not_leak(torch, shape):
    """Changing only gi at bins 0 and n_fft / 2 changes nothing beyond what the formula's real part says: re' = fl32(re * gr) -
    fl32(im * gi) with the stored im = +0 of those bins, so any finite gi gives the same words; the exact reference agrees for each."""
    c = dict(shape, B=2)
    p = CC.params(c)
    _, _, _, Tin, T = CC.geometry(c)
    F, K = c["F"], c["n_fft"] // 2 + 1
    x, g = _inputs(torch, 2, Tin, F, K, seed=13)
    Y = _rows(p, c, x)
    assert not bool(Y.imag[..., 0].ne(0).any()) and not bool(Y.imag[..., K - 1].ne(0).any())
    assert bool(g.imag[..., 0].ne(0).all()) and bool(g.imag[..., K - 1].ne(0).all())
    base = _call(torch, p, c, x, g, g)
    assert _same(torch, base, _exact(torch, p, c, x, g))
    for value in (0.0, -3.5, 1.0e30):
        g2 = g.clone()
        g2.imag[..., 0] = value
        g2.imag[..., K - 1] = -value
        got = _call(torch, p, c, x, g2, g2)
        assert _same(torch, got, _exact(torch, p, c, x, g2)), value
        assert bool((got == base).all()), value                             # float comparison: a -0 product may turn the sign of a zero
    # the real parts there do count
    g3 = g.clone()
    g3.real[..., 0] += 0.5
    assert not bool((_call(torch, p, c, x, g3, g3) == base).all())


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=PROPERTY_IDS)
def test_nan_and_infinity_reach_exactly_the_outputs_under_their_frames(torch, shape):
    c = dict(shape, B=3)
    p = CC.params(c)
    L, col0, pad, Tin, T = CC.geometry(c)
    hop, F, K = c["hop"], c["F"], c["n_fft"] // 2 + 1
    t0 = pad - col0
    x, g = _inputs(torch, 3, Tin, F, K, seed=9)
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
        for bad in (float("nan"), float("inf")):
            for part in ("real", "imag"):
                gn = g.clone()
                getattr(gn, part)[1, f, 5] = bad
                got = _call(torch, p, cn, x, gn, gn)
                assert np.array_equal(~torch.isfinite(got).cpu().numpy(), hit), (normalize, bad, part)
                assert _same(torch, got[keep], clean[keep])
        # a NaN sample: exactly the outputs under the frames whose window covers it
        xn = x.clone()
        ts = Tin // 2
        xn[1, ts] = float("nan")
        fr = [q for q in range(F) if 0 <= ts + pad - q * hop - col0 < L]
        hx = np.zeros((3, T), dtype=bool)
        for q in fr:
            hx[1] |= (w >= q * hop) & (w < q * hop + L)
        got = _call(torch, p, cn, xn, g, g)
        assert fr and np.array_equal(~torch.isfinite(got).cpu().numpy(), hx), normalize
        keep = torch.from_numpy(~hx).cuda()
        assert _same(torch, got[keep], clean[keep])


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=PROPERTY_IDS)
def test_zero_imaginary_parts_give_the_real_call_and_unit_gains_the_round_trip(torch, shape):
    """gi = +0 everywhere: on finite data the values == those of the real-gain call with gr (float comparison: fl32(im * +0) is a zero
    of either sign, which may turn the sign of a zero sum).  Gains 1 + 0i: istft*(stft*(x)) under the same comparison."""
    c = dict(shape, B=3)
    f = CC.family(c)
    p = CC.params(c)
    _, _, _, Tin, T = CC.geometry(c)
    F, K = c["F"], c["n_fft"] // 2 + 1
    x, g = _inputs(torch, 3, Tin, F, K, seed=17)
    gr = g.real.contiguous()
    g0 = torch.complex(gr, torch.zeros_like(gr))
    for normalize in (True, False):
        cn = dict(c, normalize=normalize)
        got = _call(torch, p, cn, x, g0, g0)
        real = getattr(bhw, f.real_call)(p, x, gr, c["n_fft"], c["hop"], pad_mode=c["pad_mode"], **_kw(cn))
        assert bool(torch.isfinite(got).all()) and bool((got == real).all()), normalize
        assert _same(torch, got, _exact(torch, p, cn, x, g0))
        ones = torch.ones_like(g)
        back = getattr(bhw, f.istft)(p, _rows(p, cn, x), c["n_fft"], c["hop"], **_kw(cn))
        unit = _call(torch, p, cn, x, ones, ones)
        assert bool((unit == back).all()) and _same(torch, unit, _exact(torch, p, cn, x, ones)), normalize


@pytest.mark.parametrize("fam", list(CC.FAMILIES))
def test_graph_capture(torch, fam):
    """The library form with no warm call, on a shape with several spans per signal; the table form on its first call; one stream, no
    parallel branches."""
    f = CC.FAMILIES[fam]
    call = getattr(bhw, f.call)
    p = B.make_params(B.WIN_BH5, 12, 32)
    n_fft = 512 if fam == "fft" else 400
    L, hop, T, nb = 400, 160, 48000, 4
    kw = dict(win_length=L, length=T)
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((nb, T), device="cuda", generator=gen) + 5.0
    F, K = 1 + T // hop, n_fft // 2 + 1
    sa = B.make_stft(nb, T, F, hop, n_fft, col0=(n_fft - L) // 2, pad=n_fft // 2, pad_mode=1, shift=31)
    ss = B.make_stft(nb, T, F, hop, n_fft, col0=(n_fft - L) // 2, pad=n_fft // 2, shift=31)
    assert f.real.parse(f.describe(p, L, sa, ss, normalize=True, g_stride=K, g_batch_stride=F * K))["spans"] > 2
    mask = torch.from_numpy(CC.gains(nb, F, K, seed=11)).cuda()
    with bhw.ResidentTable(p) as tab:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                lib = call(p, x, mask, n_fft, hop, **kw)                              # no warm call, no bhw_prepare_device
                tb = call(p, x, mask[0, 0], n_fft, hop, table=tab, **kw)              # the table form's first call
        torch.cuda.current_stream().wait_stream(s)
        x.copy_(torch.randn((nb, T), device="cuda", generator=gen) * 3.0 - 2.0)
        mask.copy_(torch.from_numpy(CC.gains(nb, F, K, seed=12)).cuda())
        lib.fill_(-1.0)
        tb.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        le = call(p, x, mask, n_fft, hop, **kw)
        te = call(p, x, mask[0, 0], n_fft, hop, table=tab, **kw)
        torch.cuda.synchronize()
    assert _same(torch, lib, le) and _same(torch, tb, te)
    assert not torch.equal(lib, tb) and bool(torch.isfinite(lib).all())


@pytest.mark.parametrize("shape", CC.E2E_SHAPES, ids=[s["id"] for s in CC.E2E_SHAPES])
def test_end_to_end_against_float64_within_twice_torch(torch, shape):
    """Noise in, the maximum absolute error against the float64 reference torch.istft(torch.stft(x64) * G64) at most twice that of the
    same expression evaluated by torch in float32."""
    f = CC.FAMILIES[shape["family"]]
    p = B.make_params(B.WIN_BH4, 12, 32)
    n_fft, L, hop, T = (shape[k] for k in ("n_fft", "L", "hop", "T"))
    xn, gn = CC.e2e_inputs(shape)
    x, g = torch.from_numpy(xn).cuda(), torch.from_numpy(gn).cuda()
    v = bhw.window(p, L, dtype=torch.float32)
    got = getattr(bhw, f.call)(p, x, g, n_fft, hop, win_length=L, length=T)
    St = torch.stft(x, n_fft, hop, L, window=v, center=True, pad_mode="reflect", return_complex=True)
    yard = torch.istft(St * g.transpose(-1, -2), n_fft, hop, L, window=v, center=True, length=T)
    x64, v64, g64 = x.double(), v.double(), g.to(torch.complex128)
    S64 = torch.stft(x64, n_fft, hop, L, window=v64, center=True, pad_mode="reflect", return_complex=True)
    ref = torch.istft(S64 * g64.transpose(-1, -2), n_fft, hop, L, window=v64, center=True, length=T)
    err = float((got.double() - ref).abs().max())
    yerr = float((yard.double() - ref).abs().max())
    print(f"cmask end to end {shape['id']}: fused max abs error {err:.3e}, torch.istft(torch.stft * G) {yerr:.3e}, ratio {err / yerr:.3f}")
    assert got.shape == x.shape and err <= 2.0 * yerr, (err, yerr)


def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    x = torch.zeros((2, 1000), device="cuda")
    m = torch.ones((33,), dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError, match="bhw.stft_mask_istft takes real gains"):
        bhw.stft_cmask_istft(p, x, m.real.contiguous(), 64, 16)
    with pytest.raises(ValueError, match="bhw.stft_cmask_istft_mixed takes it"):
        bhw.stft_cmask_istft(p, x, torch.ones((31,), dtype=torch.complex64, device="cuda"), 60, 16)
    with pytest.raises(ValueError, match="bhw.stft_cmask_istft takes it"):
        bhw.stft_cmask_istft_mixed(p, x, m, 64, 16)
    with pytest.raises(ValueError, match="stft_iq"):
        bhw.stft_cmask_istft(p, x.to(torch.complex64), m, 64, 16)
    with pytest.raises(ValueError, match="broadcast"):
        bhw.stft_cmask_istft(p, x, torch.ones((3, 1, 33), dtype=torch.complex64, device="cuda"), 64, 16)
    with pytest.raises(ValueError, match=r"\(K,\)"):
        bhw.stft_cmask_istft(p, x, torch.ones((32,), dtype=torch.complex64, device="cuda"), 64, 16)
    with pytest.raises(ValueError, match="last axis"):
        bhw.stft_cmask_istft(p, x, torch.ones((33, 63), dtype=torch.complex64, device="cuda").t(), 64, 16)
    with pytest.raises(ValueError, match="complex64 CUDA tensor"):
        bhw.stft_cmask_istft(p, x, m.cpu(), 64, 16)
    with pytest.raises(ValueError, match="complex64 CUDA tensor"):
        bhw.stft_cmask_istft(p, x, m.to(torch.complex128), 64, 16)
    with pytest.raises(ValueError, match="out must be"):
        bhw.stft_cmask_istft(p, x, m, 64, 16, out=torch.zeros((2, 999), device="cuda"))
    with pytest.raises(ValueError, match="table must be"):
        bhw.stft_cmask_istft(p, x, m, 64, 16, table=object())
    with pytest.raises(B.BhwError, match="overlap"):
        bhw.stft_cmask_istft(p, x, m, 64, 16, out=x)
    out = torch.empty((2, 1000), device="cuda")
    assert bhw.stft_cmask_istft(p, x, m, 64, 16, out=out).data_ptr() == out.data_ptr() and not bool(out.ne(0).any())
    torch.cuda.synchronize()
