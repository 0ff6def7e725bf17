"""The case table of the fused inverse FFT + overlap-add front (bhw_istft_fft_f32_*), in the manner of tests/stft_fft_cases.py: the
call shapes that between them reach every class its planner (bhwp_istft_fft_plan) can emit, and the classes each shape is there for.

A class is a predicate on the describe line of the call (B.describe_istft_fft), which names the kernel instance, the radix schedule,
the lanes per row, the spans a workgroup runs side by side, the columns per lane, the span length S, the halo, the spans per signal,
the groups, the grid and the LDS bytes.

tests/test_istft_fft_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds, that a sweep of the planner
emits no (schedule, spans per workgroup, columns per lane) shape the table lacks, and that every span's frame list is exactly the
frames that reach its outputs; tests/test_gpu_istft_fft.py runs every case, library and table, against numpy in float64.
"""
import re

from blackman_harris_win_amd import binding as B

import plan_cases as PC
from stft_fft_cases import SCHEDULES, MAX_GRID

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
    m = re.search(r"in pre-split \+ passes ([0-9x]+),", line)
    d["schedule"] = m.group(1) if m else None
    d["kernels"] = {k: tuple(a.split(",")) for k, a in re.findall(r"(k_\w+)<([\w,]+)>", line)}
    d["table"] = any("_table" in k for k in d["kernels"])
    d["normalize"] = "normalised by" in line
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


def desc(c):
    """The bhw_stft of a case: (descriptor, L, col0, pad, length).  padded: gaps behind every spectrum row, every signal of Y and
    every signal of x (sentinels in the GPU test)."""
    L, col0, pad, _, T = geometry(c)
    n_fft, F = c["n_fft"], c["F"]
    xs, ys, ybs = 0, 0, 0
    if c.get("padded"):
        xs, ys = T + 5, n_fft + 2 + 6
        ybs = F * ys + 10
    s = B.make_stft(c["B"], T, F, c["hop"], n_fft, col0=col0, pad=pad, shift=SETUPS[c["setup"]][2] - 1, x_stride=xs, y_stride=ys,
                    y_batch_stride=ybs)
    return s, L, col0, pad, T


def line(c, table=None):
    s, L = desc(c)[:2]
    return B.describe_istft_fft(params(c["setup"]), L, s, normalize=c["normalize"], table=table)


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
    "16 columns per lane": lambda c, d: d["cpl"] == 16,
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
    "padded strides": lambda c, d: bool(c.get("padded")),
    "direct form 1": lambda c, d: d["kernels"].get("k_istft_fft_direct") == ("1",),
    "direct form 2": lambda c, d: d["kernels"].get("k_istft_fft_direct") == ("2",),
    "heavy overlap named in the line": lambda c, d: d["heavy"],
    "the inverse of the benchmarked batch (64 x 998 x 257, 400 / 512 / 160)": lambda c, d: (d["signals"], d["frames"], d["n_fft"], d["L"], d["fy"])
    == (64, 998, 512, 400, 4) and c["hop"] == 160,
})

CASES = [
    dict(id="n16-l13", setup=1, n_fft=16, L=13, hop=5, center=True, normalize=True, B=3, F=18,
         classes=("schedule 4x2 (n_fft 16)", "4 columns per lane", "several rows per workgroup", "L below n_fft", "center on", "hop not dividing L",
                  "a signal cut into several spans, halo frames recomputed", "slots of one workgroup in different signals", "normalised",
                  "an idle slot in the last group")),
    dict(id="n32-one-span-raw", setup=0, n_fft=32, L=32, hop=16, center=True, normalize=False, B=5, F=4,
         classes=("schedule 4x4 (n_fft 32)", "8 columns per lane", "a signal in one span", "L = n_fft", "raw", "direct form 2")),
    dict(id="n64-l49-short", setup=3, n_fft=64, L=49, hop=13, center=True, normalize=True, B=3, F=40, extra=-9,
         classes=("schedule 4x4x2 (n_fft 64)", "a ragged last span", "length short of torch's default")),
    dict(id="n64-hop4-few-frames", setup=3, n_fft=64, L=64, hop=4, center=True, normalize=True, B=2, F=6, extra=90,
         classes=("a span shorter than its halo",)),
    dict(id="n128-l100-padded-long", setup=2, n_fft=128, L=100, hop=37, center=True, normalize=True, B=4, F=50, extra=300, padded=True,
         classes=("schedule 4x4x4 (n_fft 128)", "padded strides", "length past the frames' extent")),
    dict(id="n256-nocenter-form1", setup=FORM1, n_fft=256, L=256, hop=64, center=False, normalize=True, B=2, F=44,
         classes=("schedule 4x4x4x2 (n_fft 256)", "center off", "direct form 1")),
    dict(id="n256-l100-hop300", setup=2, n_fft=256, L=100, hop=300, center=True, normalize=True, B=3, F=5, padded=True,
         classes=("hop above L (zeros inside the signal)",)),
    dict(id="n512-l400", setup=0, n_fft=512, L=400, hop=160, center=True, normalize=True, B=2, F=26,
         classes=("schedule 4x4x4x4 (n_fft 512)", "a signal cut into several spans, halo frames recomputed")),
    dict(id="n1024-l1000-raw", setup=4, n_fft=1024, L=1000, hop=300, center=True, normalize=False, B=3, F=15,
         classes=("schedule 4x4x4x4x2 (n_fft 1024)", "raw")),
    dict(id="n2048-nocenter", setup=4, n_fft=2048, L=2048, hop=512, center=False, normalize=True, B=1, F=20,
         classes=("schedule 4x4x4x4x4 (n_fft 2048)", "one row per workgroup", "center off")),
    dict(id="n2048-l100-loop", setup=4, n_fft=2048, L=100, hop=200, center=True, normalize=True, B=1, F=2047, extra=1000,
         classes=("more groups than workgroups (the group loop)",)),
    dict(id="n2048-hop16-heavy", setup=4, n_fft=2048, L=2048, hop=16, center=True, normalize=True, B=1, F=1100,
         classes=("heavy overlap named in the line",)),
    dict(id="n4096", setup=0, n_fft=4096, L=4096, hop=1024, center=True, normalize=True, B=2, F=8,
         classes=("schedule 4x4x4x4x4x2 (n_fft 4096)", "16 columns per lane")),
    dict(id="bench-64x998x257", setup=0, n_fft=512, L=400, hop=160, center=True, normalize=True, B=64, F=998,
         classes=("the inverse of the benchmarked batch (64 x 998 x 257, 400 / 512 / 160)", "S set by the grid target")),
]


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
