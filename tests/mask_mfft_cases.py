"""The case table of the mixed-radix fused STFT + mask + inverse STFT front (bhw_mask_mfft_f32_*), in the manner of
tests/mask_fft_cases.py, whose gain layouts, padding modes and parser it reuses: the plan of the call IS the inverse mixed-radix call's
for the synthesis descriptor, so the cases are istft_mfft_cases.CASES with n_fft < 2048 (n2560-l100-loop, n4000 and n4050 drop out:
the mask kernel refuses their sizes), each with an analysis padding mode and a gain layout of its own, and one case more: the group
loop, which only 2560 reached there, at n_fft 1500.

A class is a predicate on the describe line of the call (B.describe_mask_mfft): the span and pass classes of
istft_mfft_cases.CLASSES, the direct forms under the mask kernel's name, and the padding and gain classes of mask_fft_cases.CLASSES.
Dropped by name, because only sizes of 2048 and above reach them:
  - "16 columns per lane": below 2048 the lanes per row are at least n_fft / 8, so a lane has at most 8 columns;
  - "the schedule 5x5x3x3x3x3 of n_fft 4050": 4050 is refused;
  - "a first radix-5 pass with a butterfly per lane": M / 5 = 256 lanes needs n_fft = 2560.
In their place stands "at most 8 columns per lane", the bound the kernel's ring is compiled for.

tests/test_mask_mfft_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds, that a sweep of the planner
over all 73 sizes emits no shape the table lacks and that every plan field is describe_istft_mfft's; tests/test_gpu_mask_mfft.py runs
every case, library and table, word for word against bhw.stft_mixed, a multiply and bhw.istft_mixed.
"""
from blackman_harris_win_amd import binding as B

import istft_mfft_cases as XC
import mask_fft_cases as MC

SETUPS, params, FORM1 = XC.SETUPS, XC.params, XC.FORM1
MAX_N = 2047
PAD_MODES, LAYOUTS = MC.PAD_MODES, MC.LAYOUTS
SIZES = [n for n in range(1, MAX_N + 1) if B.mfft_supported(n)]           # the 73 sizes the front takes
pass_shapes, layout = XC.pass_shapes, XC.layout


def geometry(c):
    """(L, col0, pad, T_in, T_out): the framing of torch.stft / torch.istft.  The analysis input has torch.istft's default length for F
    frames, so stft_mixed gives exactly F frames; the output has the case's length (`extra` past or short of it)."""
    return XC.geometry(c)


def desc(c):
    """(analysis descriptor, synthesis descriptor, L, T_in, T_out, g_stride, g_batch_stride).  padded: gaps behind every input signal,
    every output signal, every gain row and every signal's gains."""
    L, col0, pad, Tin, T = geometry(c)
    n_fft, F, K = c["n_fft"], c["F"], c["n_fft"] // 2 + 1
    shift = SETUPS[c["setup"]][2] - 1
    xs, os_ = (Tin + 3, T + 5) if c.get("padded") else (0, 0)
    sa = B.make_stft(c["B"], Tin, F, c["hop"], n_fft, col0=col0, pad=pad, pad_mode=PAD_MODES[c["pad_mode"]], shift=shift, x_stride=xs)
    ss = B.make_stft(c["B"], T, F, c["hop"], n_fft, col0=col0, pad=pad, shift=shift, x_stride=os_)
    gs, gbs = LAYOUTS[c["gains"]](F, K)
    return sa, ss, L, Tin, T, gs, gbs


def line(c, table=None):
    sa, ss, L, _, _, gs, gbs = desc(c)
    return B.describe_mask_mfft(params(c["setup"]), L, sa, ss, normalize=c["normalize"], g_stride=gs, g_batch_stride=gbs, table=table)


def parse(text):
    """mask_fft_cases.parse (the plan fields in the inverse call's words, the analysis side and the gains), plus the radices."""
    d = MC.parse(text)
    d["radices"] = [int(r) for r in d["schedule"].split("x")] if d["schedule"] else []
    return d


DROPPED = {
    "16 columns per lane": "below 2048 a row has at least n_fft / 8 lanes: at most 8 columns per lane",
    "the schedule 5x5x3x3x3x3 of n_fft 4050": "4050 is refused",
    "a first radix-5 pass with a butterfly per lane": "M / 5 = 256 needs n_fft 2560",
    "direct form 1": "restated under the mask kernel's name",
    "direct form 2": "restated under the mask kernel's name",
}
_MASK_CLASSES = ("analysis padded by reflection", "analysis padded with zeros", "analysis not padded (center off)", "gains (B, F, K)",
                 "gains (K,): one row for all", "gains (F, K): the same for every signal", "gains (B, 1, K): one row per signal",
                 "padded gain strides with padded output strides")
CLASSES = {name: pred for name, pred in XC.CLASSES.items() if name not in DROPPED}
CLASSES.update({name: MC.CLASSES[name] for name in _MASK_CLASSES})
CLASSES.update({
    "direct form 1": lambda c, d: d["kernels"].get("k_mask_mfft_direct") == ("1",),
    "direct form 2": lambda c, d: d["kernels"].get("k_mask_mfft_direct") == ("2",),
    "at most 8 columns per lane": lambda c, d: d["cpl"] <= 8,
})

# the group loop below 2048: one row per workgroup, hop above L, more spans than the grid has workgroups
_LOOP = dict(id="n1500-l100-loop", setup=4, n_fft=1500, L=100, hop=200, center=True, normalize=True, B=1, F=2047, extra=1500,
             classes=("more groups than workgroups (the group loop)", "one row per workgroup", "hop above L (zeros inside the signal)"))

_MASK = {
    "n18-l13": ("reflect", "BFK", ("analysis padded by reflection", "gains (B, F, K)", "at most 8 columns per lane")),
    "n20-one-span-raw": ("constant", "B1K", ("analysis padded with zeros", "gains (B, 1, K): one row per signal")),
    "n30-l24-short": ("reflect", "K", ("gains (K,): one row for all",)),
    "n50-hop4-few": ("constant", "FK", ("gains (F, K): the same for every signal",)),          # T_in = 20 is below the pad: no reflection
    "n54-l40-padded-long": ("reflect", "padded", ("padded gain strides with padded output strides",)),
    "n96-nocenter-form1": ("constant", "B1K", ("analysis not padded (center off)",)),
    "n250-l100-hop300": ("reflect", "padded", ()),
    "n400": ("constant", "BFK", ()),
    "n480-l400-raw": ("reflect", "FK", ()),
    "n1000-raw": ("constant", "K", ()),
    "n1200-nocenter": ("reflect", "FK", ("a pass with two trips",)),
    "n1200-hop8-heavy": ("reflect", "BFK", ()),
    "n1536": ("constant", "B1K", ()),
    "n1500-l100-loop": ("reflect", "B1K", ()),
    "bench-64x998x201": ("reflect", "BFK", ()),
}

CASES = []
for _c in XC.CASES:
    if _c["id"] == "n2560-l100-loop":
        _c = _LOOP                                         # the class it was there for, at a size the front takes
    if _c["n_fft"] > MAX_N:
        continue
    _mode, _gains, _more = _MASK[_c["id"]]
    CASES.append(dict(_c, pad_mode=_mode, gains=_gains, classes=tuple(n for n in _c["classes"] if n in CLASSES) + _more))


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
