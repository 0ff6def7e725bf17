"""The generator, the reference and the float32 stand-in of tests/cmask_cases.py, with no GPU.

  - gains(): unit phases times magnitudes in [0, 2], the exact entries 0, 1, i and -1, nonzero imaginary parts at bins 0 and n_fft / 2,
    a function of its arguments alone.
  - reference(): the contract's four separately rounded products -- the same words from numpy and from eager torch, whatever the
    layout, the broadcasting or the order of anything else; a fused product (binary64 arithmetic rounded once) is NOT the same words,
    so the test would see a kernel that contracts; a conjugated or swapped gain is a gross error.
  - standin32(): rfft, reference(), irfft and overlap-add in float32 on the CPU.  On the inputs of the GPU suite's end-to-end test it
    meets that test's yardstick -- a maximum absolute error against float64 of at most twice that of torch.istft(torch.stft(x) * G) in
    float32 -- so a float32 route can satisfy the bound; and the bits of reference() do not move when the stand-in orders its frames
    differently."""
import numpy as np
import pytest
import torch

import cmask_cases as CC


def _words(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def test_the_gain_generator():
    g = CC.gains(3, 40, 33, seed=1)
    assert g.dtype == np.complex64 and g.shape == (3, 40, 33)
    assert np.array_equal(_words(g), _words(CC.gains(3, 40, 33, seed=1))) and not np.array_equal(g, CC.gains(3, 40, 33, seed=2))
    mag = np.abs(g.astype(np.complex128))
    assert mag.max() <= 2.0 + 1e-6 and mag.min() == 0.0 and 0.9 < mag.mean() < 1.1
    inner = g[..., 1:-1]
    for value in (0.0, 1.0, 1.0j, -1.0):
        assert 0.02 < np.mean(inner == np.complex64(value)) < 0.06, value
    # every quadrant: a conjugation or a swap of the parts moves most entries by about their magnitude
    for sr in (1, -1):
        for si in (1, -1):
            assert np.mean((np.sign(g.real) == sr) & (np.sign(g.imag) == si)) > 0.15
    assert np.all(g.imag[..., 0] != 0.0) and np.all(g.imag[..., -1] != 0.0)
    assert np.median(np.abs(g - np.conj(g))) > 0.5 and np.median(np.abs(g - (g.imag + 1j * g.real))) > 0.3
    m, full = CC.layout(g, "B1K")
    assert m.shape == (3, 1, 33) and full.shape == g.shape and full.strides[1] == 0


def _rows(seed, shape):
    r = np.random.RandomState(seed)
    y = np.empty(shape, dtype=np.complex64)
    y.real = (r.standard_normal(shape) * 100.0).astype(np.float32)
    y.imag = (r.standard_normal(shape) * 100.0).astype(np.float32)
    return y


def test_the_reference_is_four_separately_rounded_products():
    y, g = _rows(3, (2, 30, 65)), CC.gains(2, 30, 65, seed=3)
    z = CC.reference(y, g)
    assert z.dtype == np.complex64
    f32, f64 = np.float32, np.float64
    # spelled out scalar by scalar in binary64 with explicit roundings (a product of two float32 is exact in binary64)
    yr, yi, gr, gi = (a.astype(f64) for a in (y.real, y.imag, g.real, g.imag))
    re = ((yr * gr).astype(f32).astype(f64) - (yi * gi).astype(f32).astype(f64)).astype(f32)
    im = ((yr * gi).astype(f32).astype(f64) + (yi * gr).astype(f32).astype(f64)).astype(f32)
    assert np.array_equal(_words(z.real), _words(re)) and np.array_equal(_words(z.imag), _words(im))
    # a fused form -- one product exact, one rounding at the end -- differs in some words: the gate tells the two apart
    fused_re = ((yr * gr).astype(f32).astype(f64) - yi * gi).astype(f32)
    assert 0 < np.mean(_words(fused_re) != _words(re)) < 0.5
    # eager torch on the planes says the same words
    zt = CC.reference(torch.from_numpy(y), torch.from_numpy(g)).numpy()
    assert np.array_equal(_words(z.real), _words(zt.real)) and np.array_equal(_words(z.imag), _words(zt.imag))
    # within the rounding of a complex multiply of the library, but not promised equal to it
    lib = (torch.from_numpy(y) * torch.from_numpy(g)).numpy()
    scale = np.abs(y.astype(np.complex128)) * np.abs(g.astype(np.complex128))
    assert np.all(np.abs(lib.astype(np.complex128) - z.astype(np.complex128)) <= 4.0 * np.finfo(f32).eps * scale + 1e-30)
    # a conjugated or a swapped gain is a gross error, not an ulp
    for wrong in (np.conj(g), (g.imag + 1j * g.real).astype(np.complex64)):
        bad = CC.reference(y, wrong)
        assert np.median(np.abs(bad - z)) > 10.0


def test_the_reference_does_not_depend_on_layout_broadcast_or_order():
    y, g = _rows(5, (4, 12, 33)), CC.gains(4, 12, 33, seed=5)
    z = CC.reference(y, g)
    # row by row, in reverse order, on a transposed copy: the same words
    rows = np.stack([np.stack([CC.reference(y[b, f], g[b, f]) for f in reversed(range(12))][::-1]) for b in range(4)])
    assert np.array_equal(_words(z.real), _words(rows.real)) and np.array_equal(_words(z.imag), _words(rows.imag))
    zt = CC.reference(np.ascontiguousarray(y.transpose(2, 0, 1)), np.ascontiguousarray(g.transpose(2, 0, 1))).transpose(1, 2, 0)
    assert np.array_equal(_words(z.real), _words(zt.real)) and np.array_equal(_words(z.imag), _words(zt.imag))
    for name in ("K", "FK", "B1K"):
        m, full = CC.layout(g, name)
        a, b = CC.reference(y, m), CC.reference(y, np.ascontiguousarray(full))
        assert a.shape == y.shape and np.array_equal(_words(a.real), _words(b.real)) and np.array_equal(_words(a.imag), _words(b.imag))
    # the exact entries: 0 gives zeros, 1 the row, -1 its negative, i the row turned (each product exact)
    one = CC.reference(y, np.ones_like(g))
    assert np.array_equal(one, y)
    assert np.array_equal(CC.reference(y, -np.ones_like(g)), -y)
    assert np.array_equal(CC.reference(y, np.full_like(g, 1j)), (-y.imag + 1j * y.real).astype(np.complex64))
    assert not np.any(CC.reference(y, np.zeros_like(g)))
    # bins whose stored imaginary part is +0 (0 and n_fft / 2): gi enters as fl32(0 * gi) = a zero, and the real part is fl32(re * gr)
    y0 = y.copy()
    y0.imag[..., 0] = 0.0
    z0 = CC.reference(y0, g)
    assert np.array_equal(z0.real[..., 0], y0.real[..., 0] * g.real[..., 0])


@pytest.mark.parametrize("shape", CC.E2E_SHAPES, ids=[s["id"] for s in CC.E2E_SHAPES])
def test_a_float32_route_meets_the_end_to_end_yardstick(shape):
    n_fft, L, hop, T = shape["n_fft"], shape["L"], shape["hop"], shape["T"]
    x, g = CC.e2e_inputs(shape)
    v = np.blackman(L).astype(np.float32) + np.float32(0.01)            # any float32 window: the stand-in has no library behind it
    ref = CC.ref64(x, g, v, n_fft, hop, L)
    got = CC.standin32(x, g, v, n_fft, hop, L)
    xt, vt, gt = torch.from_numpy(x), torch.from_numpy(v), torch.from_numpy(g)
    St = torch.stft(xt, n_fft, hop, L, window=vt, center=True, pad_mode="reflect", return_complex=True)
    yard = torch.istft(St * gt.transpose(-1, -2), n_fft, hop, L, window=vt, center=True, length=T).numpy()
    err, yerr = float(np.abs(got - ref).max()), float(np.abs(yard - ref).max())
    print(f"cmask stand-in {shape['id']}: float32 stand-in max abs error {err:.3e}, torch.istft(torch.stft * G) {yerr:.3e}, ratio {err / yerr:.3f}")
    assert got.shape == x.shape and 0.0 < err <= 2.0 * yerr, (err, yerr)
    # the masked rows do not depend on the order in which the stand-in sums its frames; only the sum's last bits may
    F = 1 + T // hop
    other = CC.standin32(x, g, v, n_fft, hop, L, order=list(reversed(range(F))))
    assert float(np.abs(other - got).max()) <= 4.0 * np.finfo(np.float32).eps * float(np.abs(ref).max())
