"""The case table of the fused multichannel filter-and-sum fronts (bhw_beam_fft_f32_*, bhw_beam_mfft_f32_*): every case of
tests/cmask_cases.py with the same geometry, padding mode and gain layout at C = 3 channels -- the plan of a call IS the complex-gain
call's for the B output signals (the channel sums live in registers), so these are already the smallest shapes that reach every plan
class, and an odd channel count makes a skipped or a doubled channel show -- then a few cases at C = 1, 2 and 8 and one at
BHW_BEAM_MAX_CH = 64 channels with two frames.

A class is a predicate on the describe line (B.describe_beam_fft / B.describe_beam_mfft): the siblings' plan classes, the direct forms
under the new kernels' names, the weight layouts as the line's three gain strides show them, and the channel counts.

inputs() and gains() are the generators of every test, numpy from the case alone, so the tests without a GPU see the GPU tests' own
inputs: noise with an offset whose scale differs from channel to channel (0.5, 1.5, 2.5 and 3.5 hundreds in turn), so that the float32
sum over the channels depends on its order, and cmask_cases.gains() per channel.  reference() states the contract as separate float32
operations, for numpy arrays and torch tensors alike: cmask_cases.reference() per channel, Z = P_0, then Z = Z + P_c per part in
ascending channel order.

tests/test_beam_plan_coverage.py (no GPU) holds the table to the planner; tests/test_gpu_beam.py runs every case, library and table,
word for word against stft* per channel, reference() and istft*.
"""
from types import SimpleNamespace

import numpy as np

from blackman_harris_win_amd import binding as B

import cmask_cases as CC

MAX_CH = B.BEAM_MAX_CH

FAMILIES = {
    "fft": SimpleNamespace(name="fft", cmask=CC.FAMILIES["fft"], describe=B.describe_beam_fft, sizes=CC.FAMILIES["fft"].sizes,
                           call="stft_beamform_istft", cmask_call="stft_cmask_istft", stft="stft", istft="istft",
                           device="bhw_beam_fft_f32_device", from_table="bhw_beam_fft_f32_from_table", max_lds=40960),
    "mfft": SimpleNamespace(name="mfft", cmask=CC.FAMILIES["mfft"], describe=B.describe_beam_mfft, sizes=CC.FAMILIES["mfft"].sizes,
                            call="stft_beamform_istft_mixed", cmask_call="stft_cmask_istft_mixed", stft="stft_mixed", istft="istft_mixed",
                            device="bhw_beam_mfft_f32_device", from_table="bhw_beam_mfft_f32_from_table", max_lds=40000),
}
PAD_MODES = CC.PAD_MODES

# the weight layouts: what (g_stride, g_ch_stride, g_batch_stride) are for C channels of F frames of K bins, in pairs
LAYOUTS = {
    "BFK": lambda C, F, K: (K, F * K, C * F * K),                   # full (B, C, F, K)
    "K": lambda C, F, K: (0, K, 0),                                 # (C, K): one row per channel for every frame and every signal
    "FK": lambda C, F, K: (K, F * K, 0),                            # (C, F, K): the same weights for every signal
    "B1K": lambda C, F, K: (0, K, C * K),                           # (B, C, 1, K): one row per channel and signal
    # full, gaps behind every row, every channel and every signal (NaN sentinels on the GPU)
    "padded": lambda C, F, K: (K + 7, F * (K + 7) + 5, C * (F * (K + 7) + 5) + 11),
}


def family(c):
    return FAMILIES[c["family"]]


def params(c):
    return CC.params(c)


def geometry(c):
    return CC.geometry(c)


def desc(c):
    """(analysis descriptor, synthesis descriptor, L, T_in, T_out, n_ch, x_ch_stride, g_stride, g_ch_stride, g_batch_stride).  padded:
    gaps behind every channel and every signal of the input, every output signal, every gain row, every channel's and every signal's
    gains."""
    sa, ss, L, Tin, T, _, _ = CC.desc(c)
    C, F, K = c["C"], c["F"], c["n_fft"] // 2 + 1
    xcs = Tin + 3 if c.get("padded") else 0
    sa.x_stride = C * (Tin + 3) + 2 if c.get("padded") else 0
    gs, gcs, gbs = LAYOUTS[c["gains"]](C, F, K)
    return sa, ss, L, Tin, T, C, xcs, gs, gcs, gbs


def line(c, table=None):
    sa, ss, L, _, _, C, xcs, gs, gcs, gbs = desc(c)
    return family(c).describe(params(c), L, sa, ss, C, normalize=c["normalize"], x_ch_stride=xcs, g_stride=gs, g_ch_stride=gcs,
                              g_batch_stride=gbs, table=table)


def cmask_line(c, table=None):
    """The complex-gain call's line for the same descriptors and the frame and batch strides of the gains (one channel)."""
    sa, ss, L, _, _, _, _, gs, _, gbs = desc(c)
    sa.x_stride = 0
    return family(c).cmask.describe(params(c), L, sa, ss, normalize=c["normalize"], g_stride=gs, g_batch_stride=gbs, table=table)


def parse(c, text):
    import re
    d = CC.parse(c, text)
    m = re.search(r"complex gains: channels (\d+), g_stride (\d+), g_ch_stride (\d+), g_batch_stride (\d+), ", text)
    d["channels"], d["g_stride"], d["g_ch_stride"], d["g_batch_stride"] = (int(v) for v in m.groups()) if m else (None, 0, 0, 0)
    return d


_LAYOUT_CLASS = {"BFK": "weights (B, C, F, K)", "K": "weights (C, K): one row per channel", "FK": "weights (C, F, K): the same for every signal",
                 "B1K": "weights (B, C, 1, K): one row per channel and signal", "padded": "padded weight strides with padded input and output strides"}


def _is_layout(name):
    return lambda c, d: (d["g_stride"], d["g_ch_stride"], d["g_batch_stride"]) == LAYOUTS[name](d["channels"], d["frames"], d["n_fft"] // 2 + 1)


def _dropped(name):
    """The siblings' classes this table restates: their gain layouts, their direct forms and their first words."""
    return name.startswith(("gains (", "padded gain strides", "direct form")) or name == "complex gains"


def _classes(fam):
    cl = {name: pred for name, pred in CC.CLASSES[fam].items() if not _dropped(name)}
    cl["direct form 1"] = lambda c, d: d["kernels"].get(f"k_beam_{fam}_direct") == ("1",)
    cl["direct form 2"] = lambda c, d: d["kernels"].get(f"k_beam_{fam}_direct") == ("2",)
    cl["beam line"] = lambda c, d: d["complex_gains"] and d["line"].startswith(f"beam {fam} ") and d["channels"] == c["C"]
    for name in LAYOUTS:
        cl[_LAYOUT_CLASS[name]] = _is_layout(name)
    for n in (1, 2, 3, 8, MAX_CH):
        cl[f"channels {n}"] = (lambda n: lambda c, d: d["channels"] == n)(n)
    return cl


CLASSES = {fam: _classes(fam) for fam in FAMILIES}


def _beam(c, C, suffix=None, **over):
    keep = tuple(n for n in c["classes"] if not _dropped(n))
    b = dict(c, C=C, id=f"{c['id']}-c{C}" + (suffix or ""), **over)
    direct = tuple(n for n in c["classes"] if n.startswith("direct form"))
    b["classes"] = keep + direct + ("beam line", _LAYOUT_CLASS[b["gains"]], f"channels {C}")
    return b


CASES = [_beam(c, 3) for c in CC.CASES]
# the other channel counts, on small shapes of both families: one channel (the complex-gain call), two, eight, and the most, two frames
_SMALL = {"fft": "fft-n64-l49-short", "mfft": "mfft-n18-l13"}
for _fam in FAMILIES:
    _s = CC.case(_SMALL[_fam])
    CASES += [_beam(_s, 1, gains="BFK"), _beam(_s, 2, gains="padded", padded=True), _beam(_s, 8, gains="FK")]
    CASES.append(_beam(dict(_s, F=2, B=2, pad_mode="constant", classes=()), MAX_CH, "-two-frames", gains="BFK"))   # (too short to reflect)


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)


def inputs(nb, C, Tin, seed=0):
    """x (B, C, T_in) float32, numpy, from the arguments alone: noise of 50, 150, 250 and 350 in turn over the channels, offset 5."""
    r = np.random.RandomState(4500 + seed)
    scale = (100.0 * (0.5 + np.arange(C) % 4)).reshape(1, C, 1)
    return (r.standard_normal((nb, C, Tin)) * scale + 5.0).astype(np.float32)


def gains(nb, C, F, K, seed=0):
    """(B, C, F, K) complex64, numpy: cmask_cases.gains() with the channels as further signals."""
    return CC.gains(nb * C, F, K, seed).reshape(nb, C, F, K)


def layout(g, name):
    """The weights array of a layout, and the same weights broadcast to (B, C, F, K) (a view)."""
    if name == "K":
        m = g[0, :, 0].copy()
    elif name == "FK":
        m = g[0].copy()
    elif name == "B1K":
        m = g[:, :, 0:1].copy()
    else:
        m = g
    full = m[:, None, :] if name == "K" else m
    return m, np.broadcast_to(full, g.shape)


def _add(a, b):
    """One float32 addition per part, numpy or torch."""
    re, im = a.real + b.real, a.imag + b.imag
    if isinstance(re, np.ndarray):
        assert re.dtype == np.float32 and im.dtype == np.float32
        out = np.empty(re.shape, dtype=np.complex64)
        out.real, out.imag = re, im
        return out
    import torch
    assert re.dtype == torch.float32 and im.dtype == torch.float32
    return torch.complex(re, im)


def products(rows_per_channel, g):
    """[P_0, ..., P_{C-1}]: cmask_cases.reference() of every channel (axis -3 of both arguments; g broadcasts over the others)."""
    C = rows_per_channel.shape[-3]
    assert g.shape[-3] == C
    return [CC.reference(rows_per_channel[..., c, :, :], g[..., c, :, :]) for c in range(C)]


def reference(rows_per_channel, g):
    """The summed rows of the contract, as separate float32 operations on the planes: P_c by cmask_cases.reference(), Z = P_0, then
    Z = fl32(Z + P_c) per part for c = 1 .. C - 1.  rows_per_channel (..., C, F, K) and g broadcastable to it, complex64 numpy arrays
    or torch tensors; returns (..., F, K)."""
    P = products(rows_per_channel, g)
    Z = P[0]
    for Pc in P[1:]:
        Z = _add(Z, Pc)
    return Z


def descending(P):
    Z = P[-1]
    for Pc in P[-2::-1]:
        Z = _add(Z, Pc)
    return Z


def pairwise(P):
    return P[0] if len(P) == 1 else _add(pairwise(P[:len(P) // 2]), pairwise(P[len(P) // 2:]))


# ---- a float32 stand-in on the CPU and the float64 reference, as cmask_cases has them, with the channel axis ----------------------------

def standin_rows(x, v, n_fft, hop, L):
    """float32 rows (B, C, F, K) on the CPU: torch.fft.rfft of the windowed frames of every channel (center=True, reflect)."""
    import torch
    nb, C, T = x.shape
    fr, vd, F, pad = CC._frames(x.reshape(nb * C, T), v, n_fft, hop, L, np.float32)
    Y = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(fr)), dim=-1).numpy()
    assert Y.dtype == np.complex64
    return Y.reshape(nb, C, F, -1), vd, pad


def standin32(x, g, v, n_fft, hop, L):
    """float32 on the CPU: rfft per channel, reference(), irfft, overlap-add.  x (B, C, T), g (B, C, F, K).  Returns float32 (B, T)."""
    import torch
    Y, vd, pad = standin_rows(x, v, n_fft, hop, L)
    Z = reference(Y, g)
    rows = torch.fft.irfft(torch.from_numpy(Z), n=n_fft, dim=-1).numpy()
    assert rows.dtype == np.float32
    return CC._ola(rows, vd, hop, pad, x.shape[-1]).astype(np.float32)


def ref64(x, g, v, n_fft, hop, L):
    """The float64 reference of the end-to-end yardstick: the same chain in binary64 with binary64 complex multiplies and sums."""
    nb, C, T = x.shape
    fr, vd, F, pad = CC._frames(x.reshape(nb * C, T), v, n_fft, hop, L, np.float64)
    Y = np.fft.rfft(fr, axis=-1).reshape(nb, C, F, -1)
    rows = np.fft.irfft((Y * g.astype(np.complex128)).sum(axis=1), n=n_fft, axis=-1)
    return CC._ola(rows, vd, hop, pad, T)


E2E_CH = 4
E2E_SHAPES = [dict(s, C=E2E_CH) for s in CC.E2E_SHAPES]


def e2e_inputs(shape):
    """Noise and full complex weights of an end-to-end shape, numpy, from the shape alone."""
    F, K = 1 + shape["T"] // shape["hop"], shape["n_fft"] // 2 + 1
    return inputs(shape["B"], shape["C"], shape["T"], seed=shape["n_fft"]), gains(shape["B"], shape["C"], F, K, seed=shape["n_fft"])
