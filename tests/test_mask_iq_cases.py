"""The generator, the reference and the float32 stand-in of tests/mask_iq_cases.py, with no GPU.

  - gains(): pairs -- unit phases times magnitudes in [0, 2] with the exact entries 0, 1, i and -1; real gains -- magnitudes in [0, 2]
    with exact 0 and 1; a function of its arguments alone.
  - reference(): the contract's separately rounded products, held word for word to explicit roundings in binary64 -- the same words
    from numpy and from eager torch, whatever the layout, the broadcasting or the order of anything else; a fused product is NOT the
    same words, so the gate would see a kernel that contracts; a conjugated or swapped gain is a gross error.
  - unshift(): a mask on a centred axis put in natural order is torch.fft.ifftshift, at an even and an odd n_fft.
  - standin32(): fft, reference(), ifft and overlap-add in float32 on the CPU.  On the inputs of the GPU suite's end-to-end test it
    meets that test's yardstick -- a maximum absolute error against float64 of at most twice that of torch.istft(torch.stft(x) * G) in
    complex64 -- so a float32 route can satisfy the bound; and on a real signal under a Hermitian mask its imaginary part stays within
    real_signal_bound(), the bound the GPU test holds the kernels to."""
import numpy as np
import pytest
import torch

import mask_iq_cases as MC


def _words(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _same(a, b):
    return np.array_equal(_words(a.real), _words(b.real)) and np.array_equal(_words(a.imag), _words(b.imag))


def test_the_gain_generators():
    g = MC.gains(3, 40, 64, seed=1)
    assert g.dtype == np.complex64 and g.shape == (3, 40, 64)
    assert _same(g, MC.gains(3, 40, 64, seed=1)) and not np.array_equal(g, MC.gains(3, 40, 64, seed=2))
    mag = np.abs(g.astype(np.complex128))
    assert mag.max() <= 2.0 + 1e-6 and mag.min() == 0.0 and 0.9 < mag.mean() < 1.1
    for value in (0.0, 1.0, 1.0j, -1.0):
        assert 0.02 < np.mean(g == np.complex64(value)) < 0.06, value
    for sr in (1, -1):
        for si in (1, -1):
            assert np.mean((np.sign(g.real) == sr) & (np.sign(g.imag) == si)) > 0.15
    assert np.median(np.abs(g - np.conj(g))) > 0.5 and np.median(np.abs(g - (g.imag + 1j * g.real))) > 0.3
    r = MC.gains(3, 40, 75, seed=1, gtype="real")
    assert r.dtype == np.float32 and r.shape == (3, 40, 75) and r.min() == 0.0 and r.max() <= 2.0
    for value in (0.0, 1.0):
        assert 0.02 < np.mean(r == np.float32(value)) < 0.06, value
    m, full = MC.layout(g, "B1K")
    assert m.shape == (3, 1, 64) and full.shape == g.shape and full.strides[1] == 0


def test_unshift_is_ifftshift_at_even_and_odd_sizes():
    for n in (16, 64, 25, 75):
        k = np.arange(n, dtype=np.float32)                                   # the gain of bin k is k
        centred = np.fft.fftshift(k)
        assert centred[(np.arange(n) + n // 2) % n].tolist() == k.tolist()  # bin k sits in column (k + n // 2) % n
        assert np.array_equal(MC.unshift(centred, n), k) and np.array_equal(MC.unshift(centred, n), np.fft.ifftshift(centred))
        t = torch.from_numpy(centred)
        assert torch.equal(MC.unshift(t, n), torch.from_numpy(k)) and torch.equal(torch.fft.fftshift(torch.from_numpy(k)), t)


def _rows(seed, shape):
    r = np.random.RandomState(seed)
    y = np.empty(shape, dtype=np.complex64)
    y.real = (r.standard_normal(shape) * 100.0).astype(np.float32)
    y.imag = (r.standard_normal(shape) * 100.0).astype(np.float32)
    return y


def test_the_reference_is_separately_rounded_products():
    f32, f64 = np.float32, np.float64
    y, g = _rows(3, (2, 30, 75)), MC.gains(2, 30, 75, seed=3)
    z = MC.reference(y, g)
    assert z.dtype == np.complex64
    # spelled out in binary64 with explicit roundings (a product of two float32 is exact in binary64, and a sum of two float32 rounded
    # to binary64 and then to float32 is the correctly rounded float32 sum: 53 >= 2 * 24 + 2)
    yr, yi, gr, gi = (a.astype(f64) for a in (y.real, y.imag, g.real, g.imag))
    re = ((yr * gr).astype(f32).astype(f64) - (yi * gi).astype(f32).astype(f64)).astype(f32)
    im = ((yr * gi).astype(f32).astype(f64) + (yi * gr).astype(f32).astype(f64)).astype(f32)
    assert np.array_equal(_words(z.real), _words(re)) and np.array_equal(_words(z.imag), _words(im))
    # a fused form -- one product exact, one rounding at the end -- differs in some words: the gate tells the two apart
    fused_re = ((yr * gr).astype(f32).astype(f64) - yi * gi).astype(f32)
    assert 0 < np.mean(_words(fused_re) != _words(re)) < 0.5
    # a real gain: one rounding per part
    r = MC.gains(2, 30, 75, seed=3, gtype="real")
    zr = MC.reference(y, r)
    assert np.array_equal(_words(zr.real), _words((yr * r.astype(f64)).astype(f32)))
    assert np.array_equal(_words(zr.imag), _words((yi * r.astype(f64)).astype(f32)))
    # eager torch on the planes says the same words
    for gains in (g, r):
        assert _same(MC.reference(y, gains), MC.reference(torch.from_numpy(y), torch.from_numpy(gains)).numpy())
    # within the rounding of a complex multiply of the library, but not promised equal to it
    lib = (torch.from_numpy(y) * torch.from_numpy(g)).numpy()
    scale = np.abs(y.astype(np.complex128)) * np.abs(g.astype(np.complex128))
    assert np.all(np.abs(lib.astype(np.complex128) - z.astype(np.complex128)) <= 4.0 * np.finfo(f32).eps * scale + 1e-30)
    # a conjugated or a swapped gain is a gross error, not an ulp
    for wrong in (np.conj(g), (g.imag + 1j * g.real).astype(np.complex64)):
        assert np.median(np.abs(MC.reference(y, wrong) - z)) > 10.0
    # no bin is special: the imaginary part of the gain counts at bin 0 and at n_fft / 2 as anywhere
    y64, g64 = _rows(4, (2, 5, 64)), MC.gains(2, 5, 64, seed=4)
    g2 = g64.copy()
    g2.imag[..., 0] += 0.5
    g2.imag[..., 32] -= 0.5
    d = MC.reference(y64, g2) != MC.reference(y64, g64)
    assert d[..., 0].all() and d[..., 32].all() and not d[..., 1:32].any() and not d[..., 33:].any()


def test_the_reference_does_not_depend_on_layout_broadcast_or_order():
    y = _rows(5, (4, 12, 60))
    for gtype in MC.GTYPES:
        g = MC.gains(4, 12, 60, seed=5, gtype=gtype)
        z = MC.reference(y, g)
        rows = np.stack([np.stack([MC.reference(y[b, f], g[b, f]) for f in reversed(range(12))][::-1]) for b in range(4)])
        assert _same(z, rows)
        zt = MC.reference(np.ascontiguousarray(y.transpose(2, 0, 1)), np.ascontiguousarray(g.transpose(2, 0, 1))).transpose(1, 2, 0)
        assert _same(z, zt)
        for name in ("K", "FK", "B1K"):
            m, full = MC.layout(g, name)
            a, b = MC.reference(y, m), MC.reference(y, np.ascontiguousarray(full))
            assert a.shape == y.shape and _same(a, b)
        assert np.array_equal(MC.reference(y, np.ones_like(g)), y) and not np.any(MC.reference(y, np.zeros_like(g)))
    g = MC.gains(4, 12, 60, seed=5)
    assert np.array_equal(MC.reference(y, -np.ones_like(g)), -y)
    assert np.array_equal(MC.reference(y, np.full_like(g, 1j)), (-y.imag + 1j * y.real).astype(np.complex64))
    # gi = +0 everywhere: the values of the real-gain formula (a zero of either sign apart)
    gr = np.ascontiguousarray(g.real)
    g0 = (gr + 0j).astype(np.complex64)
    assert np.array_equal(MC.reference(y, g0), MC.reference(y, gr))


def _window(L):
    return np.blackman(L).astype(np.float32) + np.float32(0.01)               # any float32 window: the stand-in has no library behind it


@pytest.mark.parametrize("gtype", MC.GTYPES)
@pytest.mark.parametrize("shape", MC.E2E_SHAPES, ids=[s["id"] for s in MC.E2E_SHAPES])
def test_a_float32_route_meets_the_end_to_end_yardstick(shape, gtype):
    n_fft, L, hop, T = shape["n_fft"], shape["L"], shape["hop"], shape["T"]
    x, g = MC.e2e_inputs(shape, gtype)
    assert x.dtype == np.complex64 and g.shape == (shape["B"], 1 + (T + 2 * (n_fft // 2) - n_fft) // hop, n_fft) and 100 <= shape["B"] * g.shape[1] <= 1000
    v = _window(L)
    ref = MC.ref64(x, g, v, n_fft, hop, L)
    got = MC.standin32(x, g, v, n_fft, hop, L)
    xt, vt, gt = torch.from_numpy(x), torch.from_numpy(v), torch.from_numpy(g)

    def chain(xx, vv, gg):
        S = torch.stft(xx, n_fft, hop, L, window=vv, center=True, pad_mode="reflect", onesided=False, return_complex=True)
        return torch.istft(S * gg.transpose(-1, -2), n_fft, hop, L, window=vv, center=True, length=T, onesided=False, return_complex=True)

    yard = chain(xt, vt, gt).numpy()
    ref_t = chain(xt.to(torch.complex128), vt.double(), gt.to(torch.complex128) if gtype == "pair" else gt.double()).numpy()
    assert float(np.abs(ref_t - ref).max()) <= 1e-9 * float(np.abs(ref).max())    # the numpy reference is torch's float64 chain
    err, yerr = float(np.abs(got - ref).max()), float(np.abs(yard - ref).max())
    print(f"mask iq stand-in {shape['id']} {gtype}: float32 stand-in max abs error {err:.3e}, torch.istft(torch.stft * G) {yerr:.3e}, "
          f"ratio {err / yerr:.3f}")
    assert got.shape == x.shape and got.dtype == np.complex64 and 0.0 < err <= 2.0 * yerr, (err, yerr)


@pytest.mark.parametrize("n_fft,L,hop,F", [(64, 49, 13, 40), (2048, 2048, 512, 24), (75, 61, 13, 40), (2000, 2000, 500, 24)])
def test_a_float32_route_keeps_a_real_signal_real_under_a_hermitian_mask(n_fft, L, hop, F):
    """The shapes of the GPU test's property cases: the stand-in's imaginary part is within real_signal_bound() of zero."""
    T = n_fft + hop * (F - 1) - 2 * (n_fft // 2)
    x, g = MC.real_signal_inputs(2, T, F, n_fft)
    assert not x.imag.any() and g.shape == (2, F, n_fft)
    k = np.arange(n_fft)
    assert np.array_equal(g, np.conj(g[..., (n_fft - k) % n_fft])) and np.abs(g.imag).max() > 0.5
    got = MC.standin32(x, g, _window(L), n_fft, hop, L)
    mag = np.abs(got).max(axis=-1)
    worst = np.abs(got.imag).max(axis=-1)
    bound = MC.real_signal_bound(n_fft, mag)
    print(f"real signal, stand-in, n_fft {n_fft}: max |imag| / (2^-24 log2 n max |out|) = {float((worst / mag).max()) / (2.0 ** -24 * np.log2(n_fft)):.3f}")
    assert (mag > 1.0).all() and (worst <= bound).all(), (worst, bound)
    # and a mask that is not Hermitian does not: the property is the mask's, not the route's
    g2 = MC.gains(2, F, n_fft, seed=9)
    bad = MC.standin32(x, g2, _window(L), n_fft, hop, L)
    assert np.abs(bad.imag).max() > 1000.0 * bound.max()
