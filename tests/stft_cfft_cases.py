"""The case table of the fused window + complex FFT front for I/Q input (bhw_stft_cfft_f32_*), in the manner of
tests/stft_fft_cases.py: the call shapes that between them reach every class its planner (bhwp_stft_cfft_plan) can emit, and the
classes each shape is there for.

A class is a predicate on the describe line of the call (B.describe_stft_cfft), which names the kernel instance, the radix schedule,
the lanes per row, the rows a workgroup runs side by side, the complex columns per lane, the groups, the grid, the LDS bytes, the
output form and whether the bins are shifted.

tests/test_stft_cfft_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds, that a sweep of the
planner over every supported n_fft emits no shape the table lacks, and that the plan of n complex points has the lanes, rows and
passes of the real plan of 2n points; tests/test_gpu_stft_iq.py runs every case, library and table, against numpy.fft.fft in float64
of the float32 rows.
"""
import re

from blackman_harris_win_amd import binding as B

import plan_cases as PC

SETUPS, params, FORM1 = PC.SETUPS, PC.params, PC.FORM1
SCHEDULES = {16: "4x4", 32: "4x4x2", 64: "4x4x4", 128: "4x4x4x2", 256: "4x4x4x4", 512: "4x4x4x4x2", 1024: "4x4x4x4x4",
             2048: "4x4x4x4x4x2"}
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
    m = re.search(r"in passes ([0-9x]+) \(no split\)", line)
    d["schedule"] = m.group(1) if m else None
    d["kernels"] = {k: tuple(a.split(",")) for k, a in re.findall(r"(k_\w+)<([\w,]+)>", line)}
    d["table"] = any("_table" in k for k in d["kernels"])
    d["detrend"] = "constant detrend" in line
    d["reflect"] = " reflect," in line
    d["power"] = "power rows" in line
    d["shifted"] = "bins shifted" in line
    return d


def row_floats(c):
    """The floats of an output row: n_fft powers or n_fft complex64 bins."""
    return c["n_fft"] if c.get("power") else 2 * c["n_fft"]


def pad_gaps(c):
    """The gaps of a padded case, in floats, behind every output row and every signal: even for complex64 rows, odd for power rows
    (no evenness rule)."""
    return (5, 7) if c.get("power") else (6, 10)


def desc(c):
    """The bhw_stft of a case (channels 2): (descriptor, L, frames, col0, pad, detrend).  mode None: no padding (center=False);
    detrend: the Welch segments (col0 0, F = 1 + (T - L) / hop).  padded: gaps of pad_gaps(c) floats behind every output row and every
    signal (sentinels in the GPU test) and of 5 complex samples behind every signal of x."""
    n_fft, L, hop, nb, T = c["n_fft"], c["L"], c["hop"], c["B"], c["T"]
    W = row_floats(c)
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
        xs, (rgap, sgap) = 2 * (T + 5), pad_gaps(c)
        ys = W + rgap
        ybs = frames * ys + sgap
    s = B.make_stft(nb, T, frames, hop, n_fft, col0=col0, pad=pad, pad_mode=mode, channels=2, shift=SETUPS[c["setup"]][2] - 1, x_stride=xs,
                    y_stride=ys, y_batch_stride=ybs)
    return s, L, frames, col0, pad, bool(c["detrend"])


def line(c, table=None):
    s, L, _, _, _, det = desc(c)
    return B.describe_stft_cfft(params(c["setup"]), L, s, detrend=det, power=bool(c.get("power")), fftshift=bool(c.get("fftshift")), table=table)


CLASSES = {f"schedule {s} (n_fft {n})": (lambda c, d, n=n, s=s: d["n_fft"] == n and d["schedule"] == s) for n, s in SCHEDULES.items()}
CLASSES.update({
    "one row per workgroup": lambda c, d: d["fy"] == 1,
    "several rows per workgroup": lambda c, d: d["fy"] > 1,
    "64 rows per workgroup (4 lanes per row)": lambda c, d: d["fy"] == 64 and d["lpf"] == 4,
    "4 columns per lane": lambda c, d: d["cpl"] == 4,
    "8 columns per lane": lambda c, d: d["cpl"] == 8,
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
    "direct form 1": lambda c, d: d["kernels"].get("k_stft_cfft_direct") == ("1",),
    "direct form 2": lambda c, d: d["kernels"].get("k_stft_cfft_direct") == ("2",),
    "power output": lambda c, d: d["power"],
    "power output, shifted bins": lambda c, d: d["power"] and d["shifted"],
    "spectrum output, shifted bins": lambda c, d: not d["power"] and d["shifted"],
    "spectrum output, bins in order": lambda c, d: not d["power"] and not d["shifted"],
})

# power / fftshift: the output form the describe line of the case names; the GPU test runs the spectrum form of every case for the
# accuracy figure and the named form against it, word for word.
CASES = [
    dict(id="n16-l13-detrend", setup=1, n_fft=16, L=13, hop=5, mode=None, detrend=True, B=3, T=100,
         classes=("schedule 4x4 (n_fft 16)", "several rows per workgroup", "64 rows per workgroup (4 lanes per row)", "4 columns per lane",
                  "a ragged last group", "one group", "L below n_fft", "detrend", "detrend, L below 64 (idle partial sums)",
                  "detrend, several rows per wave of the mean", "spectrum output, bins in order")),
    dict(id="n32-reflect", setup=0, n_fft=32, L=32, hop=16, mode="reflect", detrend=False, B=5, T=500,
         classes=("schedule 4x4x2 (n_fft 32)", "reflect padding", "L = n_fft", "direct form 2", "a whole last group")),
    dict(id="n64-l49-constant-power", setup=3, n_fft=64, L=49, hop=13, mode="constant", detrend=False, B=3, T=150, power=True,
         classes=("schedule 4x4x4 (n_fft 64)", "constant padding", "power output")),
    dict(id="n128-l100-detrend-padded-shift", setup=2, n_fft=128, L=100, hop=37, mode=None, detrend=True, B=4, T=2000, padded=True, fftshift=True,
         classes=("schedule 4x4x4x2 (n_fft 128)", "padded strides", "detrend, L above 64 and not a multiple of 64",
                  "spectrum output, shifted bins")),
    dict(id="n256-nopad-form1", setup=FORM1, n_fft=256, L=256, hop=64, mode=None, detrend=False, B=2, T=3000,
         classes=("schedule 4x4x4x4 (n_fft 256)", "no padding, no detrending", "direct form 1")),
    dict(id="n256-l200-nopad-col0-power-shift", setup=2, n_fft=256, L=200, hop=100, mode=None, detrend=False, B=3, T=1000, padded=True, power=True,
         fftshift=True, classes=("no padding, the window off column 0", "padded strides", "power output, shifted bins")),
    dict(id="n512-l400-reflect", setup=0, n_fft=512, L=400, hop=160, mode="reflect", detrend=False, B=2, T=4000,
         classes=("schedule 4x4x4x4x2 (n_fft 512)", "a whole last group")),
    dict(id="n1024-l1000-detrend", setup=4, n_fft=1024, L=1000, hop=300, mode=None, detrend=True, B=3, T=5000,
         classes=("schedule 4x4x4x4x4 (n_fft 1024)", "one row per workgroup")),
    dict(id="n1024-hop8-loop", setup=4, n_fft=1024, L=1024, hop=8, mode="reflect", detrend=False, B=1, T=17500,
         classes=("more groups than workgroups (the group loop)",)),
    dict(id="n2048-detrend", setup=0, n_fft=2048, L=2048, hop=2500, mode=None, detrend=True, B=2, T=10000,
         classes=("schedule 4x4x4x4x4x2 (n_fft 2048)", "8 columns per lane")),
]


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
