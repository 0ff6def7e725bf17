"""The case table of the fused STFT + COMPLEX gain + inverse STFT fronts (bhw_cmask_fft_f32_*, bhw_cmask_mfft_f32_*): every case of
tests/mask_fft_cases.py and tests/mask_mfft_cases.py with the same geometry, padding mode and gain layout, and complex gains.  The
plan of a call IS the real-gain call's for the same arguments (the gains live in registers), so these are already the smallest shapes
that reach every plan class: 4 lanes x 64 spans at n_fft 16 and 18, one row per workgroup at 2048 and 2000, odd M at 18 / 50 / 250, the
group loop at n1500-l100-loop.  A gain stride counts (gr, gi) pairs here, so LAYOUTS and desc() are the siblings' as they stand.

A class is a predicate on the describe line (B.describe_cmask_fft / B.describe_cmask_mfft): the siblings' classes, the direct forms
restated under the new kernels' names, and "complex gains".

gains() is the generator of every test: unit-magnitude random phases times magnitudes in [0, 2], so a conjugation or a swapped part is
a gross error and not an ulp; some entries exactly 0, 1, i and -1; imaginary parts nonzero at bins 0 and n_fft / 2.  reference() states
the contract's formula as separate float32 operations on the real and imaginary planes, for numpy arrays and torch tensors alike.

tests/test_cmask_plan_coverage.py (no GPU) holds the table to the planner; tests/test_gpu_cmask.py runs every case, library and table,
word for word against stft*, reference() and istft*.
"""
from types import SimpleNamespace

import numpy as np

from blackman_harris_win_amd import binding as B

import mask_fft_cases as MF
import mask_mfft_cases as MM

FAMILIES = {
    "fft": SimpleNamespace(name="fft", real=MF, describe=B.describe_cmask_fft, describe_real=B.describe_mask_fft, sizes=[1 << k for k in range(4, 12)],
                           call="stft_cmask_istft", real_call="stft_mask_istft", stft="stft", istft="istft",
                           device="bhw_cmask_fft_f32_device", from_table="bhw_cmask_fft_f32_from_table", max_lds=40960),
    "mfft": SimpleNamespace(name="mfft", real=MM, describe=B.describe_cmask_mfft, describe_real=B.describe_mask_mfft, sizes=list(MM.SIZES),
                            call="stft_cmask_istft_mixed", real_call="stft_mask_istft_mixed", stft="stft_mixed", istft="istft_mixed",
                            device="bhw_cmask_mfft_f32_device", from_table="bhw_cmask_mfft_f32_from_table", max_lds=40000),
}
LAYOUTS, PAD_MODES = MF.LAYOUTS, MF.PAD_MODES


def family(c):
    return FAMILIES[c["family"]]


def params(c):
    return family(c).real.params(c["setup"])


def geometry(c):
    return family(c).real.geometry(c)


def desc(c):
    """(analysis descriptor, synthesis descriptor, L, T_in, T_out, g_stride, g_batch_stride): the sibling's, the strides in pairs."""
    return family(c).real.desc(c)


def line(c, table=None):
    sa, ss, L, _, _, gs, gbs = desc(c)
    return family(c).describe(params(c), L, sa, ss, normalize=c["normalize"], g_stride=gs, g_batch_stride=gbs, table=table)


def real_line(c, table=None):
    sa, ss, L, _, _, gs, gbs = desc(c)
    return family(c).describe_real(params(c), L, sa, ss, normalize=c["normalize"], g_stride=gs, g_batch_stride=gbs, table=table)


def parse(c, text):
    d = family(c).real.parse(text)
    d["complex_gains"] = ", complex gains: " in text
    return d


def _classes(fam):
    real = FAMILIES[fam].real
    cl = {name: pred for name, pred in real.CLASSES.items() if name not in ("direct form 1", "direct form 2")}
    cl["direct form 1"] = lambda c, d: d["kernels"].get(f"k_cmask_{fam}_direct") == ("1",)
    cl["direct form 2"] = lambda c, d: d["kernels"].get(f"k_cmask_{fam}_direct") == ("2",)
    cl["complex gains"] = lambda c, d: d["complex_gains"] and d["line"].startswith(f"cmask {fam} ")
    return cl


CLASSES = {fam: _classes(fam) for fam in FAMILIES}
CASES = [dict(c, family=fam, id=f"{fam}-{c['id']}", classes=tuple(c["classes"]) + ("complex gains",))
         for fam in FAMILIES for c in FAMILIES[fam].real.CASES]


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)


def gains(nb, F, K, seed=0):
    """(B, F, K) complex64, numpy, from the seed alone: magnitudes uniform in [0, 2] times unit phases uniform on the circle; about 4 %
    each exactly 0, 1, i and -1; then every zero imaginary part at bins 0 and K - 1 = n_fft / 2 replaced (0.75), so that gi is
    nonzero there."""
    r = np.random.RandomState(4300 + seed)
    mag = r.uniform(0.0, 2.0, (nb, F, K))
    ph = r.uniform(0.0, 2.0 * np.pi, (nb, F, K))
    g = np.empty((nb, F, K), dtype=np.complex64)
    g.real = (mag * np.cos(ph)).astype(np.float32)
    g.imag = (mag * np.sin(ph)).astype(np.float32)
    pick = r.uniform(0.0, 1.0, (nb, F, K))
    for lo, value in ((0.00, 0.0), (0.04, 1.0), (0.08, 1.0j), (0.12, -1.0)):
        g[(pick >= lo) & (pick < lo + 0.04)] = value
    for k in (0, K - 1):
        im = g.imag[..., k]
        im[im == 0.0] = 0.75
    return g


def layout(g, name):
    """The mask array of a layout, and the same gains broadcast to (B, F, K) (a view)."""
    if name == "K":
        m = g[0, 0].copy()
    elif name == "FK":
        m = g[0].copy()
    elif name == "B1K":
        m = g[:, 0:1].copy()
    else:
        m = g
    return m, np.broadcast_to(m, g.shape)


def reference(stft_rows, g):
    """The masked rows of the contract, as separate float32 operations on the planes:
        re' = fl32( fl32(re * gr) - fl32(im * gi) )        im' = fl32( fl32(re * gi) + fl32(im * gr) ).
    stft_rows, g: complex64 numpy arrays or torch tensors that broadcast; every product and every sum is one eager float32 operation,
    so nothing is fused and no library's complex multiply is asked how it rounds."""
    yr, yi, gr, gi = stft_rows.real, stft_rows.imag, g.real, g.imag
    a, b, c, d = yr * gr, yi * gi, yr * gi, yi * gr
    re, im = a - b, c + d
    if isinstance(re, np.ndarray):
        assert re.dtype == np.float32 and im.dtype == np.float32
        out = np.empty(re.shape, dtype=np.complex64)
        out.real, out.imag = re, im
        return out
    import torch
    assert re.dtype == torch.float32 and im.dtype == torch.float32
    return torch.complex(re, im)


# ---- a float32 stand-in on the CPU: rfft, the formula, irfft, weighted overlap-add (center=True, reflect) ---------------------------------

def _frames(x, v, n_fft, hop, L, dtype):
    nb, T = x.shape
    pad, col0 = n_fft // 2, (n_fft - L) // 2
    xp = np.pad(x.astype(dtype), ((0, 0), (pad, pad)), mode="reflect")
    F = 1 + (T + 2 * pad - n_fft) // hop
    vd = np.zeros(n_fft, dtype=dtype)
    vd[col0:col0 + L] = v.astype(dtype)
    idx = np.arange(n_fft)[None, :] + hop * np.arange(F)[:, None]
    return xp[:, idx] * vd, vd, F, pad


def _ola(rows, vd, hop, pad, T, order=None):
    """Windowed rows summed in binary64 in the frame order `order` (ascending by default), divided by the envelope."""
    nb, F, n_fft = rows.shape
    S, E = np.zeros((nb, (F - 1) * hop + n_fft)), np.zeros((F - 1) * hop + n_fft)
    v64 = vd.astype(np.float64)
    for f in (range(F) if order is None else order):
        S[:, f * hop:f * hop + n_fft] += (rows[:, f] * vd).astype(np.float64)
        E[f * hop:f * hop + n_fft] += v64 * v64
    S, E = S[:, pad:pad + T], E[pad:pad + T]
    return np.where(E > 0, S / np.where(E > 0, E, 1.0), 0.0)


def standin32(x, g, v, n_fft, hop, L, order=None):
    """float32 on the CPU: torch.fft.rfft of the windowed frames, reference(), torch.fft.irfft, overlap-add.  Returns float32 (B, T)."""
    import torch
    fr, vd, F, pad = _frames(x, v, n_fft, hop, L, np.float32)
    Y = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(fr)), dim=-1).numpy()
    assert Y.dtype == np.complex64
    Z = reference(Y, g)
    rows = torch.fft.irfft(torch.from_numpy(Z), n=n_fft, dim=-1).numpy()
    assert rows.dtype == np.float32
    return _ola(rows, vd, hop, pad, x.shape[1], order).astype(np.float32)


def ref64(x, g, v, n_fft, hop, L):
    """The float64 reference of the end-to-end yardstick: the same chain in binary64 with a binary64 complex multiply (the window values
    are the library's float32 ones, exact in binary64)."""
    fr, vd, F, pad = _frames(x, v, n_fft, hop, L, np.float64)
    rows = np.fft.irfft(np.fft.rfft(fr, axis=-1) * g.astype(np.complex128), n=n_fft, axis=-1)
    return _ola(rows, vd, hop, pad, x.shape[1])


E2E_SHAPES = [dict(id="fft-512-128", family="fft", n_fft=512, L=512, hop=128, T=8000, B=2),
              dict(id="fft-2048-512", family="fft", n_fft=2048, L=2048, hop=512, T=8000, B=2),
              dict(id="mfft-400-160", family="mfft", n_fft=400, L=400, hop=160, T=8000, B=2),
              dict(id="mfft-960-480", family="mfft", n_fft=960, L=960, hop=480, T=19200, B=2)]


def e2e_inputs(shape):
    """Noise and full complex gains of an end-to-end shape, numpy, from the shape alone."""
    r = np.random.RandomState(2100 + shape["n_fft"])
    x = r.standard_normal((shape["B"], shape["T"])).astype(np.float32)
    F, K = 1 + shape["T"] // shape["hop"], shape["n_fft"] // 2 + 1
    return x, gains(shape["B"], F, K, seed=shape["n_fft"])
