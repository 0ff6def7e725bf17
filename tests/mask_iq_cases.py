"""The case table of the fused STFT + real or complex gain + inverse STFT fronts for I/Q input (bhw_mask_cfft_f32_*,
bhw_cmask_cfft_f32_*, bhw_mask_cmfft_f32_*, bhw_cmask_cmfft_f32_*), in the manner of tests/cmask_cases.py.

The plan of a call IS the inverse I/Q call's for the synthesis descriptor, so the cases are every case of
tests/istft_cfft_cases.py and tests/istft_cmfft_cases.py -- already the smallest shapes that reach every span class, pass shape and
layout of the two inverse plans -- each with an analysis padding mode, a gain layout of mask_fft_cases.LAYOUTS with K = n_fft and a
gain type ("real": float32, "pair": complex64).  The parents' fftshift cases become shifted GAIN COLUMNS (n_fft 32 and 128 even; 25
and 1215 odd), and their odd-stride cases carry an odd x_stride on the input side too (two 4-byte loads a sample; every other case
takes the 8-byte load).

A class is a predicate on the describe line (B.describe_[c]mask_c[m]fft): the parents' span classes, the direct forms under the new
kernels' names, the analysis padding modes, the gain layouts, the gain type, the shift of the gain columns and the input load.

gains() is the generator of every test: unit phases times magnitudes in [0, 2], some entries exactly 0, 1, i and -1 (real gains:
magnitudes in [0, 2] with exact 0 and 1).  reference() states the contract's formula as separate float32 operations on the real and
imaginary planes, for numpy arrays and torch tensors alike.  standin32() is a float32 CPU route (torch.fft.fft, reference(),
torch.fft.ifft, overlap-add) and ref64() the float64 yardstick's reference.

tests/test_mask_iq_plan_coverage.py (no GPU) holds the table to the planner; tests/test_gpu_mask_iq.py runs every case, library and
table, word for word against stft_iq*, reference() and istft_iq*.
"""
import re
from types import SimpleNamespace

import numpy as np

from blackman_harris_win_amd import binding as B

import istft_cfft_cases as IC
import istft_cmfft_cases as IM
import mask_fft_cases as MF
import stft_cmfft_cases as SM

SETUPS, params_of, FORM1 = IC.SETUPS, IC.params, IC.FORM1
LAYOUTS, PAD_MODES = MF.LAYOUTS, MF.PAD_MODES

FAMILIES = {
    "cfft": SimpleNamespace(name="cfft", parent=IC, sizes=[1 << k for k in range(4, 12)], stft="stft_iq", istft="istft_iq",
                            describe_parent=B.describe_istft_cfft, real_sibling="fft"),
    "cmfft": SimpleNamespace(name="cmfft", parent=IM, sizes=[n for n in SM.SIZES if n >= 18], stft="stft_iq_mixed", istft="istft_iq_mixed",
                             describe_parent=B.describe_istft_cmfft, real_sibling="mfft"),
}
assert len(FAMILIES["cmfft"].sizes) == 91 and sum(n & 1 for n in FAMILIES["cmfft"].sizes) == 18
GTYPES = ("real", "pair")


def call_name(fam, gtype):
    """The Python call of a family and gain type."""
    return f"stft_{'c' if gtype == 'pair' else ''}mask_istft_iq{'_mixed' if fam == 'cmfft' else ''}"


def c_name(fam, gtype):
    """The stem of the C calls: bhw_<stem>_f32_device / _from_table, bhw_describe_<stem>."""
    return f"{'c' if gtype == 'pair' else ''}mask_{fam}"


def describe(fam, gtype):
    return getattr(B, "describe_" + c_name(fam, gtype))


def family(c):
    return FAMILIES[c["family"]]


def params(c):
    return params_of(c["setup"])


def geometry(c):
    """(L, col0, pad, T_in, T_out): the analysis input has torch.istft's default length for F frames, so stft_iq gives exactly F frames;
    the output has the case's length."""
    return family(c).parent.geometry(c)


def strides(c):
    """(input x_stride, output x_stride) in floats, 0 for packed.  padded: gaps behind every signal, on the 8-byte grid; odd: odd strides
    on both sides (and, in the GPU test, both buffers one float off the 8-byte grid): two 4-byte loads and stores a sample."""
    _, _, _, Tin, T = geometry(c)
    if c.get("odd"):
        return 2 * Tin + 5, 2 * T + 3
    if c.get("padded"):
        return 2 * (Tin + 3), 2 * (T + 5)
    return 0, 0


def desc(c):
    """(analysis descriptor, synthesis descriptor, L, T_in, T_out, g_stride, g_batch_stride), channels 2, K = n_fft; the gain strides
    count gains (floats, or pairs)."""
    L, col0, pad, Tin, T = geometry(c)
    n_fft, F = c["n_fft"], c["F"]
    shift = SETUPS[c["setup"]][2] - 1
    xs, os_ = strides(c)
    sa = B.make_stft(c["B"], Tin, F, c["hop"], n_fft, col0=col0, pad=pad, pad_mode=PAD_MODES[c["pad_mode"]], channels=2, shift=shift, x_stride=xs)
    ss = B.make_stft(c["B"], T, F, c["hop"], n_fft, col0=col0, pad=pad, channels=2, shift=shift, x_stride=os_)
    gs, gbs = LAYOUTS[c["gains"]](F, n_fft)
    return sa, ss, L, Tin, T, gs, gbs


def line(c, table=None):
    sa, ss, L, _, _, gs, gbs = desc(c)
    return describe(c["family"], c["gtype"])(params(c), L, sa, ss, normalize=c["normalize"], fftshift=bool(c.get("fftshift")), g_stride=gs,
                                             g_batch_stride=gbs, table=table)


def parent_line(c, table=None):
    """The inverse I/Q parent's line for the synthesis descriptor and the same flags."""
    _, ss, L = desc(c)[:3]
    return family(c).describe_parent(params(c), L, ss, normalize=c["normalize"], fftshift=bool(c.get("fftshift")), table=table)


def parse(c, text):
    """The parent's parser (the plan fields stand in the line in the inverse call's words), plus the analysis side and the gains."""
    d = family(c).parent.parse(text)
    m = re.search(r"analysis of (\d+) samples, pad (\d+) (reflect|constant)\)", text)
    d["T_in"], d["pad_in"], d["pad_mode"] = (int(m.group(1)), int(m.group(2)), m.group(3)) if m else (None, None, None)
    m = re.search(r"g_stride (\d+)", text)
    d["g_stride"] = int(m.group(1)) if m else 0
    m = re.search(r"g_batch_stride (\d+)", text)
    d["g_batch_stride"] = int(m.group(1)) if m else 0
    d["one_row_per_frame"] = "one gain row for every frame" in text
    d["one_set_per_signal"] = "for every signal" in text or "and every signal" in text
    d["both_ffts"] = "forward + inverse FFT" in text
    d["complex_gains"] = ", complex gains: " in text
    d["columns_shifted"] = ", gain columns shifted, " in text
    d["columns_in_order"] = ", gain columns in order, " in text
    return d


_PARENT_ONLY = ("direct form 1", "direct form 2", "bins shifted", "bins in order", "x off the 8-byte grid with an odd stride", "padded strides")


def _classes(fam):
    cl = {name: pred for name, pred in FAMILIES[fam].parent.CLASSES.items() if name not in _PARENT_ONLY and not name.startswith("bins ")}
    kernel = lambda c: f"k_{c_name(fam, c['gtype'])}_direct"
    cl.update({
        "direct form 1": lambda c, d: d["kernels"].get(kernel(c)) == ("1",),
        "direct form 2": lambda c, d: d["kernels"].get(kernel(c)) == ("2",),
        "analysis padded by reflection": lambda c, d: d["pad_mode"] == "reflect" and d["pad_in"] > 0,
        "analysis padded with zeros": lambda c, d: d["pad_mode"] == "constant" and d["pad_in"] > 0,
        "analysis not padded (center off)": lambda c, d: d["pad_in"] == 0 and d["pad"] == 0,
        "gains (B, F, K)": lambda c, d: (d["g_stride"], d["g_batch_stride"]) == (d["n_fft"], d["frames"] * d["n_fft"]),
        "gains (K,): one row for all": lambda c, d: d["one_row_per_frame"] and d["one_set_per_signal"] and not d["g_stride"]
        and not d["g_batch_stride"],
        "gains (F, K): the same for every signal": lambda c, d: d["g_stride"] == d["n_fft"] and not d["g_batch_stride"]
        and d["one_set_per_signal"] and d["frames"] > 1,
        "gains (B, 1, K): one row per signal": lambda c, d: d["one_row_per_frame"] and not d["g_stride"] and d["g_batch_stride"] == d["n_fft"],
        "padded gain strides with padded signal strides": lambda c, d: bool(c.get("padded")) and d["g_stride"] > d["n_fft"]
        and d["g_batch_stride"] > d["frames"] * d["g_stride"] and strides(c)[0] % 2 == 0 and strides(c)[0] > 0,
        "real gains": lambda c, d: c["gtype"] == "real" and not d["complex_gains"] and d["line"].startswith(f"mask {fam} "),
        "complex gains": lambda c, d: c["gtype"] == "pair" and d["complex_gains"] and d["line"].startswith(f"cmask {fam} "),
        "gain columns shifted, even n_fft": lambda c, d: d["columns_shifted"] and not d["columns_in_order"] and d["n_fft"] % 2 == 0,
        "gain columns shifted, odd n_fft": lambda c, d: d["columns_shifted"] and not d["columns_in_order"] and d["n_fft"] % 2 == 1,
        "gain columns in order": lambda c, d: d["columns_in_order"] and not d["columns_shifted"],
        "8-byte I/Q load (even input stride)": lambda c, d: strides(c)[0] % 2 == 0,
        "4-byte I/Q loads (odd input stride)": lambda c, d: strides(c)[0] % 2 == 1 and d["signals"] > 1,
    })
    if fam == "cfft":
        del cl["gain columns shifted, odd n_fft"]          # (a power of two is even)
    return cl


CLASSES = {fam: _classes(fam) for fam in FAMILIES}

# case id of the parent -> (analysis padding, gain layout, gain type, the classes the case is here for beyond the parent's)
_MASK = {
    "cfft": {
        "n16-l13": ("reflect", "BFK", "pair", ("analysis padded by reflection", "gains (B, F, K)", "complex gains", "gain columns in order",
                                               "8-byte I/Q load (even input stride)")),
        "n32-one-span-raw-shift": ("constant", "B1K", "real", ("analysis padded with zeros", "gains (B, 1, K): one row per signal", "real gains",
                                                               "gain columns shifted, even n_fft")),
        "n64-l49-short-odd": ("reflect", "K", "pair", ("gains (K,): one row for all", "4-byte I/Q loads (odd input stride)")),
        "n64-hop4-few-frames": ("constant", "FK", "real", ("gains (F, K): the same for every signal",)),    # T_in = 20 is below the pad
        "n128-l100-padded-long-shift": ("reflect", "padded", "pair", ("padded gain strides with padded signal strides",
                                                                      "gain columns shifted, even n_fft")),
        "n256-nocenter-form1": ("constant", "B1K", "real", ("analysis not padded (center off)",)),
        "n256-l100-hop300": ("reflect", "padded", "real", ("padded gain strides with padded signal strides",)),
        "n512-l400": ("constant", "BFK", "pair", ()),
        "n1024-l1000-raw": ("constant", "K", "real", ()),
        "n1024-grid-target": ("reflect", "FK", "pair", ()),
        "n2048-nocenter": ("reflect", "FK", "real", ()),
        "n2048-l100-loop": ("reflect", "B1K", "pair", ()),
        "n2048-hop16-heavy": ("reflect", "K", "pair", ()),
    },
    "cmfft": {
        "n18-l13": ("reflect", "BFK", "pair", ("analysis padded by reflection", "gains (B, F, K)", "complex gains", "gain columns in order",
                                               "8-byte I/Q load (even input stride)")),
        "n25-one-span-raw-shift": ("constant", "B1K", "real", ("analysis padded with zeros", "gains (B, 1, K): one row per signal", "real gains",
                                                               "gain columns shifted, odd n_fft")),
        "n27-l20-short-odd": ("reflect", "K", "pair", ("gains (K,): one row for all", "4-byte I/Q loads (odd input stride)")),
        "n48-hop4-few-frames": ("constant", "FK", "real", ("gains (F, K): the same for every signal",)),
        "n75-nocenter-form1": ("constant", "B1K", "pair", ("analysis not padded (center off)",)),
        "n100-l90-padded-long-shift": ("reflect", "padded", "pair", ("padded gain strides with padded signal strides",
                                                                     "gain columns shifted, even n_fft")),
        "n100-l40-hop300": ("reflect", "padded", "real", ("padded gain strides with padded signal strides",)),
        "n400": ("constant", "BFK", "pair", ()),
        "n1000-l900-raw": ("constant", "K", "real", ()),
        "n1215-nocenter-shift": ("constant", "FK", "pair", ("gain columns shifted, odd n_fft",)),
        "n1280-l1000": ("reflect", "BFK", "real", ()),
        "n1458": ("reflect", "B1K", "pair", ()),
        "n1536-l1200-shift": ("constant", "K", "real", ("gain columns shifted, even n_fft",)),
        "n2000-l100-loop": ("reflect", "B1K", "pair", ()),
        "n2000-hop16-heavy": ("reflect", "K", "real", ()),
        "n2025": ("reflect", "FK", "pair", ()),
    },
}

CASES = []
for _fam, _f in FAMILIES.items():
    for _c in _f.parent.CASES:
        if _c["n_fft"] not in _f.sizes:
            continue                                        # (n_fft 16 of the mixed family's table, if any: below the 91 sizes)
        _mode, _gains, _gtype, _more = _MASK[_fam][_c["id"]]
        CASES.append(dict(_c, family=_fam, id=f"{_fam}-{_c['id']}", pad_mode=_mode, gains=_gains, gtype=_gtype,
                          classes=tuple(n for n in _c["classes"] if n in CLASSES[_fam]) + _more))


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)


# ---- gains and the contract's formula -------------------------------------------------------------------------------------------------------

def gains(nb, F, K, seed=0, gtype="pair"):
    """(B, F, K) numpy from the seed alone.  pair: complex64, magnitudes uniform in [0, 2] times unit phases uniform on the circle, about
    4 % each exactly 0, 1, i and -1.  real: float32, the same magnitudes, about 4 % each exactly 0 and 1."""
    r = np.random.RandomState(4400 + seed)
    mag = r.uniform(0.0, 2.0, (nb, F, K))
    ph = r.uniform(0.0, 2.0 * np.pi, (nb, F, K))
    pick = r.uniform(0.0, 1.0, (nb, F, K))
    if gtype == "real":
        g = mag.astype(np.float32)
        g[pick < 0.04] = 0.0
        g[(pick >= 0.04) & (pick < 0.08)] = 1.0
        return g
    g = np.empty((nb, F, K), dtype=np.complex64)
    g.real = (mag * np.cos(ph)).astype(np.float32)
    g.imag = (mag * np.sin(ph)).astype(np.float32)
    for lo, value in ((0.00, 0.0), (0.04, 1.0), (0.08, 1.0j), (0.12, -1.0)):
        g[(pick >= lo) & (pick < lo + 0.04)] = value
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


def unshift(g, n_fft):
    """Gains on a centred axis (the gain of bin k in column (k + n_fft // 2) % n_fft, as stft_iq*(fftshift=True) lays out its bins),
    put in natural bin order (numpy or torch, last axis): a roll by n_fft // 2 towards lower indices, torch.fft.ifftshift."""
    h = n_fft // 2
    if isinstance(g, np.ndarray):
        return np.roll(g, -h, axis=-1)
    return g.roll(-h, dims=-1)


def _is_complex(g):
    return g.dtype == np.complex64 if isinstance(g, np.ndarray) else g.is_complex()


def reference(rows, g):
    """The masked rows of the contract, as separate float32 operations on the planes.  rows: complex64 (..., n_fft) in natural bin order.
    g real float32: (fl32(re * g), fl32(im * g)).  g complex64:
        re' = fl32( fl32(re * gr) - fl32(im * gi) )        im' = fl32( fl32(re * gi) + fl32(im * gr) ).
    numpy arrays or torch tensors that broadcast; every product and every sum is one eager float32 operation, so nothing is fused."""
    yr, yi = rows.real, rows.imag
    if _is_complex(g):
        gr, gi = g.real, g.imag
        a, b, c, d = yr * gr, yi * gi, yr * gi, yi * gr
        re, im = a - b, c + d
    else:
        re, im = yr * g, yi * g
    if isinstance(re, np.ndarray):
        assert re.dtype == np.float32 and im.dtype == np.float32
        out = np.empty(re.shape, dtype=np.complex64)
        out.real, out.imag = re, im
        return out
    import torch
    assert re.dtype == torch.float32 and im.dtype == torch.float32
    return torch.complex(re, im)


# ---- a float32 stand-in on the CPU: fft, the formula, ifft, weighted overlap-add (center=True, reflect) -----------------------------------

def _frames(x, v, n_fft, hop, L, dtype):
    nb, T = x.shape
    pad, col0 = n_fft // 2, (n_fft - L) // 2
    xp = np.pad(x.astype(dtype), ((0, 0), (pad, pad)), mode="reflect")
    F = 1 + (T + 2 * pad - n_fft) // hop
    real = np.float32 if dtype == np.complex64 else np.float64
    vd = np.zeros(n_fft, dtype=real)
    vd[col0:col0 + L] = v.astype(real)
    idx = np.arange(n_fft)[None, :] + hop * np.arange(F)[:, None]
    return xp[:, idx] * vd, vd, F, pad


def _ola(rows, vd, hop, pad, T):
    """Windowed complex rows summed in binary64 per part in ascending frame order, divided by the envelope."""
    nb, F, n_fft = rows.shape
    S, E = np.zeros((nb, (F - 1) * hop + n_fft), dtype=np.complex128), np.zeros((F - 1) * hop + n_fft)
    v64 = vd.astype(np.float64)
    for f in range(F):
        S[:, f * hop:f * hop + n_fft] += (rows[:, f] * vd).astype(np.complex128)
        E[f * hop:f * hop + n_fft] += v64 * v64
    S, E = S[:, pad:pad + T], E[pad:pad + T]
    return np.where(E > 0, S / np.where(E > 0, E, 1.0), 0.0)


def standin32(x, g, v, n_fft, hop, L):
    """float32 on the CPU: torch.fft.fft of the windowed frames, reference(), torch.fft.ifft, overlap-add.  x complex64 (B, T), g in
    natural bin order.  Returns complex64 (B, T)."""
    import torch
    fr, vd, F, pad = _frames(x, v, n_fft, hop, L, np.complex64)
    assert fr.dtype == np.complex64
    Y = torch.fft.fft(torch.from_numpy(np.ascontiguousarray(fr)), dim=-1).numpy()
    Z = reference(Y, g)
    rows = torch.fft.ifft(torch.from_numpy(Z), dim=-1).numpy()
    assert rows.dtype == np.complex64
    return _ola(rows, vd, hop, pad, x.shape[1]).astype(np.complex64)


def ref64(x, g, v, n_fft, hop, L):
    """The float64 reference of the end-to-end yardstick: the same chain in binary64 with a binary64 complex multiply (the window values
    are the library's float32 ones, exact in binary64)."""
    fr, vd, F, pad = _frames(x, v, n_fft, hop, L, np.complex128)
    rows = np.fft.ifft(np.fft.fft(fr, axis=-1) * g.astype(np.complex128 if _is_complex(g) else np.float64), axis=-1)
    return _ola(rows, vd, hop, pad, x.shape[1])


E2E_SHAPES = [dict(id="cfft-512-128", family="cfft", n_fft=512, L=512, hop=128, T=8000, B=2),
              dict(id="cfft-2048-512", family="cfft", n_fft=2048, L=2048, hop=512, T=51200, B=2),
              dict(id="cmfft-400-160", family="cmfft", n_fft=400, L=400, hop=160, T=8000, B=2),
              dict(id="cmfft-75-25", family="cmfft", n_fft=75, L=75, hop=25, T=3000, B=2)]


def e2e_inputs(shape, gtype="pair"):
    """Complex noise and full gains of an end-to-end shape, numpy, from the shape alone."""
    r = np.random.RandomState(2200 + shape["n_fft"])
    x = (r.standard_normal((shape["B"], shape["T"])) + 1j * r.standard_normal((shape["B"], shape["T"]))).astype(np.complex64)
    F = 1 + (shape["T"] + 2 * (shape["n_fft"] // 2) - shape["n_fft"]) // shape["hop"]
    return x, gains(shape["B"], F, shape["n_fft"], seed=shape["n_fft"], gtype=gtype)


# ---- a real signal under a Hermitian mask ---------------------------------------------------------------------------------------------------

# The imaginary part of the output is rounding error alone.  In units of u = 2^-24 * log2(n_fft) times the largest output magnitude of
# the signal (the error scale of a float32 FFT of n_fft points): the forward transform leaves at most about 1 u in the bins, the gains
# (magnitudes up to 2) double it and add two roundings of their own, and the inverse transform adds about 1 u: 3 u and a little.  The
# window and the envelope division act on both parts alike.  8 u is that with a margin of two and more for the sup norm; the float32
# CPU stand-in is held to the same bound in tests/test_mask_iq_cases.py.
REAL_SIGNAL_FACTOR = 8.0


def real_signal_bound(n_fft, magnitude):
    return REAL_SIGNAL_FACTOR * 2.0 ** -24 * np.log2(n_fft) * np.asarray(magnitude, dtype=np.float64)


def real_signal_inputs(nb, T, F, n_fft, seed=0):
    """x complex64 (B, T) with imaginary part +0, and complex64 gains (B, F, n_fft) with G[k] = conj(G[(n_fft - k) % n_fft]): the
    spectrum of a real signal stays that of a real signal."""
    r = np.random.RandomState(4450 + seed)
    x = (r.standard_normal((nb, T)) * 100.0 + 5.0).astype(np.float32).astype(np.complex64)
    g = gains(nb, F, n_fft, seed=seed + 1)
    k = np.arange(n_fft)
    mirror = (n_fft - k) % n_fft
    upper = k > mirror
    g[..., upper] = np.conj(g[..., mirror[upper]])
    g.imag[..., k == mirror] = 0.0
    assert np.array_equal(g, np.conj(g[..., mirror]))
    return x, g
