"""The case table of the fused STFT + mask + inverse STFT front (bhw_mask_fft_f32_*), in the manner of tests/istft_fft_cases.py, whose
geometry helpers, parser and class predicates it imports: the plan of the call IS the inverse call's for the synthesis descriptor, so
the cases are istft_fft_cases.CASES without n4096 (which the mask kernel does not take), each with an analysis padding mode and a gain
layout of its own.

A class is a predicate on the describe line of the call (B.describe_mask_fft): the span classes of istft_fft_cases.CLASSES (without
the 4096 schedule and its 16 columns per lane), the direct forms under the mask kernel's name, the analysis padding modes, and the
gain layouts as the line's strides show them.

tests/test_mask_fft_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds, that a sweep of the planner
emits no shape the table lacks and that every plan field is describe_istft_fft's; tests/test_gpu_mask_fft.py runs every case, library
and table, word for word against bhw.stft, a multiply and bhw.istft.
"""
import re

from blackman_harris_win_amd import binding as B

import istft_fft_cases as IC

SETUPS, params, FORM1 = IC.SETUPS, IC.params, IC.FORM1
MAX_N = 2048
PAD_MODES = {"reflect": 1, "constant": 0}      # BHW_PAD_REFLECT, BHW_PAD_CONSTANT

# the gain layouts: what (g_stride, g_batch_stride) are for F frames of K bins
LAYOUTS = {
    "BFK": lambda F, K: (K, F * K),                        # full (B, F, K)
    "K": lambda F, K: (0, 0),                              # one row for every frame and every signal
    "FK": lambda F, K: (K, 0),                             # (F, K): the same gains for every signal
    "B1K": lambda F, K: (0, K),                            # (B, 1, K): one row per signal
    "padded": lambda F, K: (K + 7, F * (K + 7) + 11),      # full, gaps behind every row and every signal (NaN sentinels on the GPU)
}


def geometry(c):
    """(L, col0, pad, T_in, T_out): the framing of torch.stft / torch.istft.  The analysis input has torch.istft's default length for F
    frames, so stft gives exactly F frames; the output has the case's length (`extra` past or short of it)."""
    L, col0, pad, full, T = IC.geometry(c)
    return L, col0, pad, full, T


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
    return B.describe_mask_fft(params(c["setup"]), L, sa, ss, normalize=c["normalize"], g_stride=gs, g_batch_stride=gbs, table=table)


def parse(text):
    """istft_fft_cases.parse (the plan fields stand in the line in the inverse call's words), plus the analysis side and the gains."""
    d = IC.parse(text)
    m = re.search(r"analysis of (\d+) samples, pad (\d+) (reflect|constant)\)", text)
    d["T_in"], d["pad_in"], d["pad_mode"] = (int(m.group(1)), int(m.group(2)), m.group(3)) if m else (None, None, None)
    m = re.search(r"g_stride (\d+)", text)
    d["g_stride"] = int(m.group(1)) if m else 0
    m = re.search(r"g_batch_stride (\d+)", text)
    d["g_batch_stride"] = int(m.group(1)) if m else 0
    d["one_row_per_frame"] = "one gain row for every frame" in text
    d["one_set_per_signal"] = "for every signal" in text or "and every signal" in text
    d["both_ffts"] = "forward + inverse FFT" in text
    return d


_DROPPED = ("schedule 4x4x4x4x4x2 (n_fft 4096)", "16 columns per lane", "direct form 1", "direct form 2")
CLASSES = {name: pred for name, pred in IC.CLASSES.items() if name not in _DROPPED}
CLASSES.update({
    "direct form 1": lambda c, d: d["kernels"].get("k_mask_fft_direct") == ("1",),
    "direct form 2": lambda c, d: d["kernels"].get("k_mask_fft_direct") == ("2",),
    "analysis padded by reflection": lambda c, d: d["pad_mode"] == "reflect" and d["pad_in"] > 0,
    "analysis padded with zeros": lambda c, d: d["pad_mode"] == "constant" and d["pad_in"] > 0,
    "analysis not padded (center off)": lambda c, d: d["pad_in"] == 0 and d["pad"] == 0,
    "gains (B, F, K)": lambda c, d: (d["g_stride"], d["g_batch_stride"]) == (d["n_fft"] // 2 + 1, d["frames"] * (d["n_fft"] // 2 + 1)),
    "gains (K,): one row for all": lambda c, d: d["one_row_per_frame"] and d["one_set_per_signal"] and not d["g_stride"]
    and not d["g_batch_stride"],
    "gains (F, K): the same for every signal": lambda c, d: d["g_stride"] == d["n_fft"] // 2 + 1 and not d["g_batch_stride"]
    and d["one_set_per_signal"] and d["frames"] > 1,
    "gains (B, 1, K): one row per signal": lambda c, d: d["one_row_per_frame"] and not d["g_stride"]
    and d["g_batch_stride"] == d["n_fft"] // 2 + 1,
    "padded gain strides with padded output strides": lambda c, d: bool(c.get("padded")) and d["g_stride"] > d["n_fft"] // 2 + 1
    and d["g_batch_stride"] > d["frames"] * d["g_stride"],
})

_MASK = {
    "n16-l13": ("reflect", "BFK", ("analysis padded by reflection", "gains (B, F, K)")),
    "n32-one-span-raw": ("constant", "B1K", ("analysis padded with zeros", "gains (B, 1, K): one row per signal")),
    "n64-l49-short": ("reflect", "K", ("gains (K,): one row for all",)),
    "n64-hop4-few-frames": ("constant", "FK", ("gains (F, K): the same for every signal",)),    # T_in = 20 is below the pad: no reflection
    "n128-l100-padded-long": ("reflect", "padded", ("padded gain strides with padded output strides",)),
    "n256-nocenter-form1": ("constant", "B1K", ("analysis not padded (center off)",)),
    "n256-l100-hop300": ("reflect", "padded", ()),
    "n512-l400": ("constant", "BFK", ()),
    "n1024-l1000-raw": ("constant", "K", ()),
    "n2048-nocenter": ("reflect", "FK", ()),
    "n2048-l100-loop": ("reflect", "B1K", ()),
    "n2048-hop16-heavy": ("reflect", "BFK", ()),
    "bench-64x998x257": ("reflect", "BFK", ()),
}

CASES = []
for _c in IC.CASES:
    if _c["n_fft"] > MAX_N:
        continue
    _mode, _gains, _more = _MASK[_c["id"]]
    CASES.append(dict(_c, pad_mode=_mode, gains=_gains, classes=tuple(n for n in _c["classes"] if n in CLASSES) + _more))


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
