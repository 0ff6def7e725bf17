"""The generators, the reference and the float32 stand-in of tests/beam_cases.py, with no GPU.

  - reference(): the contract's products (cmask_cases.reference() per channel) and its float32 sum in ascending channel order, held
    word for word to explicit binary64-then-round arithmetic; the same words from numpy and from eager torch.
  - On the GPU tests' own inputs (inputs() and gains() of every case, through the stand-in's float32 rows) the ascending sum differs in
    some word from the descending sum at every C >= 3 and from a pairwise sum at every C >= 4, so the exact gate of
    tests/test_gpu_beam.py can tell a wrong order.  (At C = 2 the three orders are one addition; at C = 3 a pairwise sum IS the
    ascending one.)
  - C = 1 equals cmask_cases.reference().
  - standin32(): rfft per channel, reference(), irfft and overlap-add in float32 on the CPU.  On the inputs of the GPU suite's
    end-to-end test it meets that test's yardstick -- a maximum absolute error against float64 of at most twice that of
    torch.istft((torch.stft(x_c) * G_c).sum(c)) in float32 -- so a float32 route can satisfy the bound."""
import numpy as np
import pytest
import torch

import beam_cases as BC
import cmask_cases as CC


def _words(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _same(a, b):
    return np.array_equal(_words(a.real), _words(b.real)) and np.array_equal(_words(a.imag), _words(b.imag))


def _rows(seed, shape):
    r = np.random.RandomState(seed)
    y = np.empty(shape, dtype=np.complex64)
    y.real = (r.standard_normal(shape) * 100.0).astype(np.float32)
    y.imag = (r.standard_normal(shape) * 100.0).astype(np.float32)
    return y


def test_the_generators_are_functions_of_their_arguments():
    x = BC.inputs(2, 5, 300, seed=1)
    assert x.dtype == np.float32 and x.shape == (2, 5, 300) and np.array_equal(_words(x), _words(BC.inputs(2, 5, 300, seed=1)))
    assert not np.array_equal(x, BC.inputs(2, 5, 300, seed=2))
    sd = x.std(axis=(0, 2))
    assert np.all(np.abs(sd / np.array([50.0, 150.0, 250.0, 350.0, 50.0]) - 1.0) < 0.15)       # the channels differ in scale
    g = BC.gains(2, 5, 7, 33, seed=1)
    assert g.dtype == np.complex64 and g.shape == (2, 5, 7, 33) and _same(g, CC.gains(10, 7, 33, seed=1).reshape(2, 5, 7, 33))
    for name, dims in (("K", 2), ("FK", 3), ("B1K", 4), ("BFK", 4)):
        m, full = BC.layout(g, name)
        assert m.ndim == dims and full.shape == g.shape


def test_the_reference_is_the_products_and_a_float32_sum_in_ascending_channel_order():
    y, g = _rows(3, (2, 5, 30, 65)), BC.gains(2, 5, 30, 65, seed=3)
    z = BC.reference(y, g)
    assert z.dtype == np.complex64 and z.shape == (2, 30, 65)
    f32, f64 = np.float32, np.float64
    # spelled out in binary64 with explicit roundings (a product of two float32 and a sum of two float32 are exact in binary64)
    yr, yi, gr, gi = (a.astype(f64) for a in (y.real, y.imag, g.real, g.imag))
    pre = ((yr * gr).astype(f32).astype(f64) - (yi * gi).astype(f32).astype(f64)).astype(f32)
    pim = ((yr * gi).astype(f32).astype(f64) + (yi * gr).astype(f32).astype(f64)).astype(f32)
    re, im = pre[:, 0], pim[:, 0]
    for c in range(1, 5):
        re = (re.astype(f64) + pre[:, c].astype(f64)).astype(f32)
        im = (im.astype(f64) + pim[:, c].astype(f64)).astype(f32)
    assert np.array_equal(_words(z.real), _words(re)) and np.array_equal(_words(z.imag), _words(im))
    # a sum kept in binary64 and rounded once is NOT the same words: the gate sees a wider accumulator
    wide = pre.astype(f64).sum(axis=1).astype(f32)
    assert 0 < np.mean(_words(wide) != _words(re)) < 0.9
    # eager torch on the planes says the same words
    zt = BC.reference(torch.from_numpy(y), torch.from_numpy(g)).numpy()
    assert _same(z, zt)
    # the layouts broadcast: the same words as the materialised weights
    for name in ("K", "FK", "B1K"):
        m, full = BC.layout(g, name)
        assert _same(BC.reference(y, full), BC.reference(y, np.ascontiguousarray(full)))
    # channel 0 SETS the sum: a -0 product of the only channel stays -0
    y1 = np.zeros((1, 1, 1, 3), dtype=np.complex64)
    y1.real[...] = -0.0
    z1 = BC.reference(y1, np.ones((1, 1, 1, 3), dtype=np.complex64))
    assert np.all(np.signbit(z1.real))


def test_one_channel_is_the_complex_gain_reference():
    y, g = _rows(5, (3, 1, 12, 33)), BC.gains(3, 1, 12, 33, seed=5)
    assert _same(BC.reference(y, g), CC.reference(y[:, 0], g[:, 0]))
    yt, gt = torch.from_numpy(y), torch.from_numpy(g)
    assert _same(BC.reference(yt, gt).numpy(), CC.reference(yt[:, 0], gt[:, 0]).numpy())


@pytest.mark.parametrize("cid", [c["id"] for c in BC.CASES if c["C"] >= 3])
def test_on_the_gpu_tests_inputs_the_order_of_the_sum_shows(cid):
    c = BC.case(cid)
    L, col0, pad, Tin, T = BC.geometry(c)
    n, hop, C, F, K = c["n_fft"], c["hop"], c["C"], c["F"], c["n_fft"] // 2 + 1
    nb = min(c["B"], 2)                                                  # two signals say as much as sixty-four
    x, g = BC.inputs(c["B"], C, Tin)[:nb], BC.gains(c["B"], C, F, K)[:nb]
    # float32 rows of the case's own framing (the stand-in's transform, constant padding where the case is not centred)
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad)), mode="reflect" if c["pad_mode"] == "reflect" and pad and pad < Tin else "constant")
    v = np.zeros(n, dtype=np.float32)
    v[col0:col0 + L] = np.hanning(L + 2)[1:-1].astype(np.float32) + np.float32(0.01)
    idx = np.arange(n)[None, :] + hop * np.arange(F)[:, None]
    assert idx.max() < xp.shape[-1]
    Y = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(xp[:, :, idx] * v)), dim=-1).numpy()
    assert Y.dtype == np.complex64 and Y.shape == (nb, C, F, K)
    _, full = BC.layout(g, c["gains"] if c["gains"] != "padded" else "BFK")
    P = BC.products(Y, full)
    up, down = BC.reference(Y, full), BC.descending(P)
    assert not _same(up, down), "the descending sum gives the same words: the gate could not tell"
    assert np.allclose(up, down, rtol=1e-3, atol=1e-2)
    if C >= 4:
        pw = BC.pairwise(P)
        assert not _same(up, pw), "a pairwise sum gives the same words: the gate could not tell"
        assert np.allclose(up, pw, rtol=1e-3, atol=1e-2)


@pytest.mark.parametrize("shape", BC.E2E_SHAPES, ids=[s["id"] for s in BC.E2E_SHAPES])
def test_a_float32_route_meets_the_end_to_end_yardstick(shape):
    n_fft, L, hop, T, nb, C = (shape[k] for k in ("n_fft", "L", "hop", "T", "B", "C"))
    assert C == 4
    x, g = BC.e2e_inputs(shape)
    v = np.blackman(L).astype(np.float32) + np.float32(0.01)            # any float32 window: the stand-in has no library behind it
    ref = BC.ref64(x, g, v, n_fft, hop, L)
    got = BC.standin32(x, g, v, n_fft, hop, L)
    xt, vt, gt = torch.from_numpy(x), torch.from_numpy(v), torch.from_numpy(g)
    St = torch.stft(xt.reshape(nb * C, T), n_fft, hop, L, window=vt, center=True, pad_mode="reflect", return_complex=True)
    St = St.reshape(nb, C, St.shape[-2], St.shape[-1])
    yard = torch.istft((St * gt.transpose(-1, -2)).sum(dim=1), n_fft, hop, L, window=vt, center=True, length=T).numpy()
    err, yerr = float(np.abs(got - ref).max()), float(np.abs(yard - ref).max())
    print(f"beam stand-in {shape['id']}: float32 stand-in max abs error {err:.3e}, torch.istft((torch.stft * G).sum) {yerr:.3e}, "
          f"ratio {err / yerr:.3f}")
    assert got.shape == (nb, T) and 0.0 < err <= 2.0 * yerr, (err, yerr)
