"""The case table of the fused inverse complex FFT + overlap-add front for I/Q output (bhw_istft_cfft_f32_*), in the manner of
tests/istft_fft_cases.py: the call shapes that between them reach every class its planner (bhwp_istft_cfft_plan) can emit, and the
classes each shape is there for.  The shapes are those of istft_fft_cases.py wherever n_fft <= 2048 (the smallest that reach each
class); "S set by the grid target" has the smallest shape the planner admits.

A class is a predicate on the describe line of the call (B.describe_istft_cfft), which names the kernel instance, the radix schedule,
the lanes per row, the spans a workgroup runs side by side, the complex columns per lane, the span length S, the halo, the spans per
signal, the groups, the grid, the LDS bytes and whether the bins are shifted.

tests/test_istft_cfft_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds, that a sweep of the
planner emits no (schedule, spans per workgroup, columns per lane) shape the table lacks, that the lanes and passes are those of
bhwp_stft_cfft_plan, and that every span's frame list is exactly the frames that reach its outputs; tests/test_gpu_istft_iq.py runs
every case, library and table, against numpy in float64.
"""
import re

from blackman_harris_win_amd import binding as B

import plan_cases as PC
from stft_cfft_cases import SCHEDULES, MAX_GRID

SETUPS, params, FORM1 = PC.SETUPS, PC.params, PC.FORM1
TARGET_GROUPS, HALO_FACTOR = 1024, 4       # kIfftTargetGroups, kIfftHaloFactor

_FIELDS = {
    "signals": r"(\d+) signals", "frames": r" x (\d+) frames", "rows": r"= (\d+) rows", "n_fft": r"n_fft (\d+)",
    "m": r"inverse complex FFT of (\d+) points", "lpf": r"(\d+) lanes per row", "fy": r"x (\d+) spans per workgroup",
    "cpl": r"(\d+) columns per lane", "S": r"spans of S = (\d+) frames", "halo": r"\+ halo (\d+)", "spans": r"\((\d+) spans per signal",
    "trips": r"up to (\d+) frames a span", "repeated": r"(\d+)% of the transforms repeated", "groups": r"(\d+) groups",
    "grid": r"grid (\d+) x 256 lanes", "lds": r"(\d+) bytes of LDS", "L": r"L = (\d+)", "col0": r"col0 (\d+)", "pad": r"pad (\d+)",
    "t0": r"t0 = (\d+)",
}


def parse(line):
    d = {"line": line}
    for name, pat in _FIELDS.items():
        m = re.search(pat, line)
        if m:
            d[name] = int(m.group(1))
    m = re.search(r"in passes ([0-9x]+) \(no split\),", line)
    d["schedule"] = m.group(1) if m else None
    d["kernels"] = {k: tuple(a.split(",")) for k, a in re.findall(r"(k_\w+)<([\w,]+)>", line)}
    d["table"] = any("_table" in k for k in d["kernels"])
    d["normalize"] = "normalised by" in line
    d["shifted"] = "bins shifted" in line
    d["in_order"] = "bins in order" in line
    d["heavy"] = "heavy overlap" in line
    return d


def geometry(c):
    """(L, col0, pad, default length, length) of a case: the framing of torch.istft; `extra` samples past (or, negative, short of)
    torch's default length."""
    n_fft, L, hop, F = c["n_fft"], c["L"], c["hop"], c["F"]
    pad = n_fft // 2 if c["center"] else 0
    col0 = (n_fft - L) // 2
    full = n_fft + hop * (F - 1) - 2 * pad
    return L, col0, pad, full, full + c.get("extra", 0)


def strides(c):
    """(x_stride, y_stride, y_batch_stride) of a case in floats, 0 for packed.  padded: gaps behind every spectrum row, every signal of
    Y and every signal of x (sentinels in the GPU test), all on the 8-byte grid; odd: an odd x_stride (and, in the GPU test, x one
    float off the 8-byte grid): two 4-byte stores per sample."""
    T, n_fft, F = geometry(c)[4], c["n_fft"], c["F"]
    xs, ys, ybs = 0, 0, 0
    if c.get("padded"):
        xs, ys = 2 * (T + 5), 2 * n_fft + 6
        ybs = F * ys + 10
    if c.get("odd"):
        xs = 2 * T + 3
    return xs, ys, ybs


def desc(c):
    """The bhw_stft of a case (channels 2): (descriptor, L, col0, pad, length)."""
    L, col0, pad, _, T = geometry(c)
    xs, ys, ybs = strides(c)
    s = B.make_stft(c["B"], T, c["F"], c["hop"], c["n_fft"], col0=col0, pad=pad, channels=2, shift=SETUPS[c["setup"]][2] - 1, x_stride=xs,
                    y_stride=ys, y_batch_stride=ybs)
    return s, L, col0, pad, T


def line(c, table=None):
    s, L = desc(c)[:2]
    return B.describe_istft_cfft(params(c["setup"]), L, s, normalize=c["normalize"], fftshift=bool(c.get("fftshift")), table=table)


def span_frames(d, hop, F, T, s):
    """Span s of a signal, from the plan's S and t0 (bhwp_istft_span): its outputs [wlo, whi) on the axis w = t + t0 and the frames
    [f_lo, f_hi) the kernel walks for it."""
    L, S, t0 = d["L"], d["S"], d["t0"]
    hop = min(hop, t0 + T)
    wlo, whi = max(s * S * hop, t0), min((s + 1) * S * hop, t0 + T)
    if whi <= wlo:
        return wlo, wlo, 0, 0
    f_lo = (wlo - L) // hop + 1 if wlo >= L else 0
    f_hi = min((whi - 1) // hop + 1, F)
    return wlo, whi, min(f_lo, f_hi), f_hi


CLASSES = {f"schedule {s} (n_fft {n})": (lambda c, d, n=n, s=s: d["n_fft"] == n and d["schedule"] == s) for n, s in SCHEDULES.items()}
CLASSES.update({
    "4 columns per lane": lambda c, d: d["cpl"] == 4,
    "8 columns per lane": lambda c, d: d["cpl"] == 8,
    "one row per workgroup": lambda c, d: d["fy"] == 1,
    "several rows per workgroup": lambda c, d: d["fy"] > 1,
    "a signal in one span": lambda c, d: d["spans"] == 1,
    "a signal cut into several spans, halo frames recomputed": lambda c, d: d["spans"] > 1 and d["halo"] > 0 and d["S"] < d["frames"]
    and d["repeated"] > 0,
    "a span shorter than its halo": lambda c, d: d["spans"] > 1 and d["S"] < d["halo"],
    "a ragged last span": lambda c, d: d["spans"] > 1 and (d["t0"] + geometry(c)[4]) % (d["S"] * c["hop"]) != 0,
    "slots of one workgroup in different signals": lambda c, d: d["fy"] > 1 and d["signals"] > 1 and d["spans"] % d["fy"] != 0,
    "an idle slot in the last group": lambda c, d: d["fy"] > 1 and (d["signals"] * d["spans"]) % d["fy"] != 0,
    "more groups than workgroups (the group loop)": lambda c, d: d["groups"] > d["grid"] == MAX_GRID,
    "S set by the grid target": lambda c, d: d["S"] > HALO_FACTOR * d["halo"] and d["S"] > 1 and d["groups"] >= TARGET_GROUPS,
    "L below n_fft": lambda c, d: c["L"] < c["n_fft"],
    "L = n_fft": lambda c, d: c["L"] == c["n_fft"],
    "center on": lambda c, d: d["pad"] == c["n_fft"] // 2,
    "center off": lambda c, d: d["pad"] == 0,
    "hop above L (zeros inside the signal)": lambda c, d: c["hop"] > c["L"] and d["halo"] == 0 and c["F"] > 1,
    "hop not dividing L": lambda c, d: c["L"] % c["hop"] != 0 and c["hop"] < c["L"],
    "length past the frames' extent": lambda c, d: d["t0"] + geometry(c)[4] > (c["F"] - 1) * c["hop"] + c["L"],
    "length short of torch's default": lambda c, d: c.get("extra", 0) < 0,
    "normalised": lambda c, d: d["normalize"],
    "raw": lambda c, d: not d["normalize"],
    "padded strides": lambda c, d: bool(c.get("padded")) and strides(c)[0] % 2 == 0,
    "direct form 1": lambda c, d: d["kernels"].get("k_istft_cfft_direct") == ("1",),
    "direct form 2": lambda c, d: d["kernels"].get("k_istft_cfft_direct") == ("2",),
    "bins shifted": lambda c, d: d["shifted"] and not d["in_order"],
    "bins in order": lambda c, d: d["in_order"] and not d["shifted"],
    "x off the 8-byte grid with an odd stride": lambda c, d: bool(c.get("odd")) and strides(c)[0] % 2 == 1 and d["signals"] > 1,
    "heavy overlap named in the line": lambda c, d: d["heavy"],
})

CASES = [
    dict(id="n16-l13", setup=1, n_fft=16, L=13, hop=5, center=True, normalize=True, B=3, F=18,
         classes=("schedule 4x4 (n_fft 16)", "4 columns per lane", "several rows per workgroup", "L below n_fft", "center on", "hop not dividing L",
                  "a signal cut into several spans, halo frames recomputed", "slots of one workgroup in different signals", "normalised",
                  "an idle slot in the last group", "bins in order")),
    dict(id="n32-one-span-raw-shift", setup=0, n_fft=32, L=32, hop=16, center=True, normalize=False, B=5, F=4, fftshift=True,
         classes=("schedule 4x4x2 (n_fft 32)", "a signal in one span", "L = n_fft", "raw", "direct form 2", "bins shifted")),
    dict(id="n64-l49-short-odd", setup=3, n_fft=64, L=49, hop=13, center=True, normalize=True, B=3, F=40, extra=-9, odd=True,
         classes=("schedule 4x4x4 (n_fft 64)", "a ragged last span", "length short of torch's default",
                  "x off the 8-byte grid with an odd stride")),
    dict(id="n64-hop4-few-frames", setup=3, n_fft=64, L=64, hop=4, center=True, normalize=True, B=2, F=6, extra=90,
         classes=("a span shorter than its halo",)),
    dict(id="n128-l100-padded-long-shift", setup=2, n_fft=128, L=100, hop=37, center=True, normalize=True, B=4, F=50, extra=300, padded=True,
         fftshift=True, classes=("schedule 4x4x4x2 (n_fft 128)", "padded strides", "length past the frames' extent", "bins shifted")),
    dict(id="n256-nocenter-form1", setup=FORM1, n_fft=256, L=256, hop=64, center=False, normalize=True, B=2, F=44,
         classes=("schedule 4x4x4x4 (n_fft 256)", "center off", "direct form 1")),
    dict(id="n256-l100-hop300", setup=2, n_fft=256, L=100, hop=300, center=True, normalize=True, B=3, F=5, padded=True,
         classes=("hop above L (zeros inside the signal)",)),
    dict(id="n512-l400", setup=0, n_fft=512, L=400, hop=160, center=True, normalize=True, B=2, F=26,
         classes=("schedule 4x4x4x4x2 (n_fft 512)", "a signal cut into several spans, halo frames recomputed")),
    dict(id="n1024-l1000-raw", setup=4, n_fft=1024, L=1000, hop=300, center=True, normalize=False, B=3, F=15,
         classes=("schedule 4x4x4x4x4 (n_fft 1024)", "one row per workgroup", "raw")),
    dict(id="n1024-grid-target", setup=4, n_fft=1024, L=1024, hop=512, center=True, normalize=True, B=8, F=700,
         classes=("S set by the grid target",)),
    dict(id="n2048-nocenter", setup=4, n_fft=2048, L=2048, hop=512, center=False, normalize=True, B=1, F=20,
         classes=("schedule 4x4x4x4x4x2 (n_fft 2048)", "8 columns per lane", "one row per workgroup", "center off")),
    dict(id="n2048-l100-loop", setup=4, n_fft=2048, L=100, hop=200, center=True, normalize=True, B=1, F=2047, extra=1000,
         classes=("more groups than workgroups (the group loop)",)),
    dict(id="n2048-hop16-heavy", setup=4, n_fft=2048, L=2048, hop=16, center=True, normalize=True, B=1, F=1100,
         classes=("heavy overlap named in the line",)),
]


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
