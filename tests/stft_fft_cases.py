"""The case table of the fused window + FFT front (bhw_stft_fft_f32_*), in the manner of tests/plan_cases.py: the call shapes that
between them reach every class its planner (bhwp_stft_fft_plan) can emit, and the classes each shape is there for.

A class is a predicate on the describe line of the call (B.describe_stft_fft), which names the kernel instance, the radix schedule, the
lanes per row, the rows a workgroup runs side by side, the columns per lane, the groups, the grid and the LDS bytes.

tests/test_stft_fft_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds, and that a sweep of the
planner over every supported n_fft emits no (schedule, rows per workgroup, columns per lane) shape the table lacks;
tests/test_gpu_stft_fft.py runs every case, library and table, against numpy.fft.rfft in float64 of the float32 rows.
"""
import re

from blackman_harris_win_amd import binding as B

import plan_cases as PC

SETUPS, params, FORM1 = PC.SETUPS, PC.params, PC.FORM1
SCHEDULES = {16: "4x2", 32: "4x4", 64: "4x4x2", 128: "4x4x4", 256: "4x4x4x2", 512: "4x4x4x4", 1024: "4x4x4x4x2", 2048: "4x4x4x4x4",
             4096: "4x4x4x4x4x2"}
MAX_GRID = 2048                            # kFftMaxGrid

_FIELDS = {
    "signals": r"(\d+) signals", "frames": r" x (\d+) frames", "rows": r"= (\d+) rows", "n_fft": r"n_fft (\d+)", "m": r"complex FFT of (\d+) points",
    "lpf": r"(\d+) lanes per row", "fy": r"x (\d+) rows per workgroup", "cpl": r"(\d+) columns per lane", "groups": r"(\d+) groups",
    "grid": r"grid (\d+) x 256 lanes", "lds": r"(\d+) bytes of LDS", "L": r"L = (\d+)", "col0": r"col0 (\d+)", "pad": r"pad (\d+)",
}


def parse(line):
    d = {"line": line}
    for name, pat in _FIELDS.items():
        m = re.search(pat, line)
        if m:
            d[name] = int(m.group(1))
    m = re.search(r"in passes ([0-9x]+) \+ split", line)
    d["schedule"] = m.group(1) if m else None
    d["kernels"] = {k: tuple(a.split(",")) for k, a in re.findall(r"(k_\w+)<([\w,]+)>", line)}
    d["table"] = any("_table" in k for k in d["kernels"])
    d["detrend"] = "constant detrend" in line
    d["reflect"] = " reflect," in line
    return d


def desc(c):
    """The bhw_stft of a case: (descriptor, L, frames, col0, pad, detrend).  mode None: no padding (center=False); detrend: the Welch
    segments (col0 0, F = 1 + (T - L) / hop).  padded: gaps behind every spectrum row and signal (sentinels in the GPU test) and behind
    every signal of x."""
    n_fft, L, hop, nb, T = c["n_fft"], c["L"], c["hop"], c["B"], c["T"]
    K2 = n_fft + 2
    if c["detrend"]:
        pad, col0, mode = 0, 0, B.PAD_CONSTANT
        frames = 1 + (T - L) // hop
    else:
        pad = n_fft // 2 if c["mode"] else 0
        col0 = (n_fft - L) // 2
        mode = B.PAD_REFLECT if c["mode"] == "reflect" else B.PAD_CONSTANT
        frames = 1 + (T + 2 * pad - n_fft) // hop
    xs, ys, ybs = 0, 0, 0
    if c.get("padded"):
        xs, ys = T + 5, K2 + 6
        ybs = frames * ys + 10
    s = B.make_stft(nb, T, frames, hop, n_fft, col0=col0, pad=pad, pad_mode=mode, shift=SETUPS[c["setup"]][2] - 1, x_stride=xs, y_stride=ys,
                    y_batch_stride=ybs)
    return s, L, frames, col0, pad, bool(c["detrend"])


def line(c, table=None):
    s, L, _, _, _, det = desc(c)
    return B.describe_stft_fft(params(c["setup"]), L, s, detrend=det, table=table)


CLASSES = {f"schedule {s} (n_fft {n})": (lambda c, d, n=n, s=s: d["n_fft"] == n and d["schedule"] == s) for n, s in SCHEDULES.items()}
CLASSES.update({
    "one row per workgroup": lambda c, d: d["fy"] == 1,
    "several rows per workgroup": lambda c, d: d["fy"] > 1,
    "64 rows per workgroup (4 lanes per row)": lambda c, d: d["fy"] == 64 and d["lpf"] == 4,
    "4 columns per lane": lambda c, d: d["cpl"] == 4,
    "8 columns per lane": lambda c, d: d["cpl"] == 8,
    "16 columns per lane": lambda c, d: d["cpl"] == 16,
    "a ragged last group": lambda c, d: d["fy"] > 1 and d["rows"] % d["fy"] != 0,
    "a whole last group": lambda c, d: d["fy"] > 1 and d["rows"] % d["fy"] == 0,
    "one group": lambda c, d: d["groups"] == 1 and d["grid"] == 1,
    "more groups than workgroups (the group loop)": lambda c, d: d["groups"] > d["grid"] == MAX_GRID,
    "L below n_fft": lambda c, d: c["L"] < c["n_fft"],
    "L = n_fft": lambda c, d: c["L"] == c["n_fft"],
    "reflect padding": lambda c, d: not d["detrend"] and d["pad"] > 0 and d["reflect"],
    "constant padding": lambda c, d: not d["detrend"] and d["pad"] > 0 and not d["reflect"],
    "no padding, no detrending": lambda c, d: not d["detrend"] and d["pad"] == 0,
    "no padding, the window off column 0": lambda c, d: not d["detrend"] and d["pad"] == 0 and d["col0"] > 0,
    "detrend": lambda c, d: d["detrend"],
    "detrend, L below 64 (idle partial sums)": lambda c, d: d["detrend"] and c["L"] < 64,
    "detrend, L above 64 and not a multiple of 64": lambda c, d: d["detrend"] and c["L"] > 64 and c["L"] % 64 != 0,
    "detrend, several rows per wave of the mean": lambda c, d: d["detrend"] and d["fy"] > 4,
    "padded strides": lambda c, d: bool(c.get("padded")),
    "direct form 1": lambda c, d: d["kernels"].get("k_stft_fft_direct") == ("1",),
    "direct form 2": lambda c, d: d["kernels"].get("k_stft_fft_direct") == ("2",),
    "the benchmarked batch (64 x 160000, 400 / 512 / 160, detrended)": lambda c, d: (d["signals"], d["frames"], d["n_fft"], d["fy"]) == (64, 998, 512, 4)
    and d["detrend"],
})

CASES = [
    dict(id="n16-l13-detrend", setup=1, n_fft=16, L=13, hop=5, mode=None, detrend=True, B=3, T=100,
         classes=("schedule 4x2 (n_fft 16)", "several rows per workgroup", "64 rows per workgroup (4 lanes per row)", "4 columns per lane",
                  "a ragged last group", "one group", "L below n_fft", "detrend", "detrend, L below 64 (idle partial sums)",
                  "detrend, several rows per wave of the mean")),
    dict(id="n32-reflect", setup=0, n_fft=32, L=32, hop=16, mode="reflect", detrend=False, B=5, T=500,
         classes=("schedule 4x4 (n_fft 32)", "8 columns per lane", "reflect padding", "L = n_fft", "direct form 2")),
    dict(id="n64-l49-constant", setup=3, n_fft=64, L=49, hop=13, mode="constant", detrend=False, B=3, T=150,
         classes=("schedule 4x4x2 (n_fft 64)", "constant padding")),
    dict(id="n128-l100-detrend-padded", setup=2, n_fft=128, L=100, hop=37, mode=None, detrend=True, B=4, T=2000, padded=True,
         classes=("schedule 4x4x4 (n_fft 128)", "padded strides", "detrend, L above 64 and not a multiple of 64")),
    dict(id="n256-nopad-form1", setup=FORM1, n_fft=256, L=256, hop=64, mode=None, detrend=False, B=2, T=3000,
         classes=("schedule 4x4x4x2 (n_fft 256)", "no padding, no detrending", "direct form 1")),
    dict(id="n256-l200-nopad-col0", setup=2, n_fft=256, L=200, hop=100, mode=None, detrend=False, B=3, T=1000, padded=True,
         classes=("no padding, the window off column 0",)),
    dict(id="n512-l400-reflect", setup=0, n_fft=512, L=400, hop=160, mode="reflect", detrend=False, B=2, T=4000,
         classes=("schedule 4x4x4x4 (n_fft 512)", "a whole last group")),
    dict(id="n1024-l1000-detrend", setup=4, n_fft=1024, L=1000, hop=300, mode=None, detrend=True, B=3, T=5000,
         classes=("schedule 4x4x4x4x2 (n_fft 1024)",)),
    dict(id="n2048-hop16-loop", setup=4, n_fft=2048, L=2048, hop=16, mode="reflect", detrend=False, B=1, T=34000,
         classes=("schedule 4x4x4x4x4 (n_fft 2048)", "one row per workgroup", "more groups than workgroups (the group loop)")),
    dict(id="n4096-detrend", setup=0, n_fft=4096, L=4096, hop=5000, mode=None, detrend=True, B=2, T=20000,
         classes=("schedule 4x4x4x4x4x2 (n_fft 4096)", "16 columns per lane")),
    dict(id="bench-64x160000", setup=0, n_fft=512, L=400, hop=160, mode=None, detrend=True, B=64, T=160000,
         classes=("the benchmarked batch (64 x 160000, 400 / 512 / 160, detrended)",)),
]


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
