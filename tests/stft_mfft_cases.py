"""The case table of the mixed-radix fused window + FFT front (bhw_stft_mfft_f32_*), in the manner of tests/stft_cfft_cases.py: the
call shapes that between them reach every class its planner (bhwp_stft_mfft_plan) can emit, and the classes each shape is there for.

A class is a predicate on the describe line of the call (B.describe_stft_mfft), which names the kernel instance, the radix schedule,
the lanes per row, the rows a workgroup runs side by side, the columns per lane, the groups, the grid, the LDS bytes and the output
form.  95 values of n_fft are supported, so unlike the power-of-two tables a shape is not a value of n_fft: it is what the kernel's
text branches on.  pass_shapes() gives, for every pass of a schedule, (radix, place, lanes): the place is "first" (no twiddles),
"middle" (i mod Ns by the float multiply) or "last" (k = i), the lanes "idle" (fewer butterflies than lanes on the row), "exact" or
"several" (a lane takes more than one trip).

tests/test_stft_mfft_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds, and that a sweep of the
planner over every supported n_fft emits no pass shape, lane layout or column layout the table's cases do not hold, with at most 16
columns per lane and 64 KiB of LDS everywhere; tests/test_gpu_stft_mixed.py runs every case, library and table, against numpy.fft.rfft
in float64 of the float32 rows.
"""
import re

from blackman_harris_win_amd import binding as B

import plan_cases as PC

SETUPS, params, FORM1 = PC.SETUPS, PC.params, PC.FORM1
MAX_GRID = 2048                            # kFftMaxGrid
BANK_FILTERS = 80                          # the bank of the bank case: mel_weights(n_fft, 80, 16000)

_FIELDS = {
    "signals": r"(\d+) signals", "frames": r" x (\d+) frames", "rows": r"= (\d+) rows", "n_fft": r"n_fft (\d+)", "m": r"complex FFT of (\d+) points",
    "lpf": r"(\d+) lanes per row", "fy": r"x (\d+) rows per workgroup", "cpl": r"(\d+) columns per lane", "groups": r"(\d+) groups",
    "grid": r"grid (\d+) x 256 lanes", "lds": r"(\d+) bytes of LDS", "L": r"L = (\d+)", "col0": r"col0 (\d+)", "pad": r"pad (\d+)",
    "filters": r"\((\d+) filters", "weights": r"(\d+) weights",
}


def parse(line):
    d = {"line": line}
    for name, pat in _FIELDS.items():
        m = re.search(pat, line)
        if m:
            d[name] = int(m.group(1))
    m = re.search(r"in passes ([0-9x]+) \+ split", line)
    d["schedule"] = m.group(1) if m else None
    d["radices"] = [int(r) for r in d["schedule"].split("x")] if m else []
    d["kernels"] = {k: tuple(a.split(",")) for k, a in re.findall(r"(k_\w+)<([\w,]+)>", line)}
    d["table"] = any("_table" in k for k in d["kernels"])
    d["detrend"] = "constant detrend" in line
    d["reflect"] = " reflect," in line
    d["form"] = "bank" if "bank rows" in line else "power" if "power rows" in line else "spectrum" if "spectrum rows" in line else None
    return d


def pass_shapes(d):
    """{(radix, place, lanes)} of the passes of a parsed line."""
    M, lpf, Ns, out = d["m"], d["lpf"], 1, set()
    for r in d["radices"]:
        Q = M // r
        place = "first" if Ns == 1 else "last" if Ns == Q else "middle"
        lanes = "idle" if Q < lpf else "exact" if Q == lpf else "several"
        out.add((r, place, lanes))
        Ns *= r
    assert Ns == M, d["line"]
    return out


def layout(d):
    """What the row steps branch on: (4 lanes per row, one row per workgroup, a lane without its last column, 16 columns per lane)."""
    return (d["lpf"] == 4, d["fy"] == 1, d["n_fft"] % d["lpf"] != 0, d["cpl"] == 16)


def row_floats(c):
    """The floats of an output row: K complex64 bins, K powers or the bank's filters."""
    K = c["n_fft"] // 2 + 1
    return {"spectrum": 2 * K, "power": K, "bank": BANK_FILTERS}[c.get("form", "spectrum")]


def pad_gaps(c):
    """The gaps of a padded case, in floats, behind every output row and every signal: even for complex64 rows, odd otherwise."""
    return (6, 10) if c.get("form", "spectrum") == "spectrum" else (5, 7)


def fbank(c):
    """The BhwFbank of a bank case for the describe call: the counts of the bank the GPU test builds, bhw.mel_weights(n_fft, 80, 16000)
    in its sparse form, with no device arrays (host arithmetic only)."""
    if c.get("form") != "bank":
        return None
    from blackman_harris_win_amd import selector
    first, offset, weight = selector.fbank_bands(selector.mel_weights(c["n_fft"], BANK_FILTERS, 16000))
    return B.make_fbank(len(first), c["n_fft"] // 2 + 1, weight.size, None, None, None)


def desc(c):
    """The bhw_stft of a case: (descriptor, L, frames, col0, pad, detrend).  mode None: no padding (center=False); detrend: the Welch
    segments (col0 0, F = 1 + (T - L) / hop).  padded: gaps of pad_gaps(c) floats behind every output row and every signal (sentinels
    in the GPU test) and of 5 samples behind every signal of x."""
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
        xs, (rgap, sgap) = T + 5, pad_gaps(c)
        ys = W + rgap
        ybs = frames * ys + sgap
    s = B.make_stft(nb, T, frames, hop, n_fft, col0=col0, pad=pad, pad_mode=mode, shift=SETUPS[c["setup"]][2] - 1, x_stride=xs, y_stride=ys,
                    y_batch_stride=ybs)
    return s, L, frames, col0, pad, bool(c["detrend"])


def line(c, table=None):
    s, L, _, _, _, det = desc(c)
    form = c.get("form", "spectrum")
    return B.describe_stft_mfft(params(c["setup"]), L, s, detrend=det, power=form != "spectrum", fbank=fbank(c), table=table)


def _has(*rs):
    return lambda c, d: set(d["radices"]) == set(rs)


CLASSES = {
    "a schedule of only 3s": _has(3),
    "a schedule of only 5s": _has(5),
    "a schedule of 5s and 3s together": lambda c, d: {5, 3} <= set(d["radices"]),
    "a schedule with radix-4 passes": lambda c, d: 4 in d["radices"],
    "a schedule with a last radix-2 pass": lambda c, d: d["radices"][-1] == 2 and 2 not in d["radices"][:-1],
    "a schedule with neither (M odd)": lambda c, d: d["m"] % 2 == 1 and 4 not in d["radices"] and 2 not in d["radices"],
    "the schedule 5x5x4x2 of n_fft 400": lambda c, d: d["n_fft"] == 400 and d["schedule"] == "5x5x4x2",
    "the schedule 5x3x4x4 of n_fft 480": lambda c, d: d["n_fft"] == 480 and d["schedule"] == "5x3x4x4",
    "the schedule 3x3 of n_fft 18": lambda c, d: d["n_fft"] == 18 and d["schedule"] == "3x3",
    "the schedule 5x5x3x3x3x3 of n_fft 4050": lambda c, d: d["n_fft"] == 4050 and d["schedule"] == "5x5x3x3x3x3",
    "64 rows per workgroup (4 lanes per row)": lambda c, d: d["fy"] == 64 and d["lpf"] == 4,
    "several rows per workgroup": lambda c, d: 1 < d["fy"] < 64,
    "two rows per workgroup": lambda c, d: d["fy"] == 2,
    "one row per workgroup": lambda c, d: d["fy"] == 1,
    "n_fft not a multiple of the lanes (a lane without its last column)": lambda c, d: d["n_fft"] % d["lpf"] != 0,
    "n_fft a multiple of the lanes, columns per lane not a power of two": lambda c, d: d["n_fft"] % d["lpf"] == 0 and d["cpl"] & (d["cpl"] - 1),
    "6 columns per lane": lambda c, d: d["cpl"] == 6,
    "16 columns per lane": lambda c, d: d["cpl"] == 16,
    "a pass with idle lanes": lambda c, d: any(s[2] == "idle" for s in pass_shapes(d)),
    "a pass with two trips": lambda c, d: any(s[2] == "several" for s in pass_shapes(d)),
    "a first radix-3 pass of several trips": lambda c, d: (3, "first", "several") in pass_shapes(d),
    "a first radix-5 pass with a butterfly per lane": lambda c, d: (5, "first", "exact") in pass_shapes(d),
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
    "padded strides": lambda c, d: bool(c.get("padded")),
    "direct form 1": lambda c, d: d["kernels"].get("k_stft_mfft_direct") == ("1",),
    "direct form 2": lambda c, d: d["kernels"].get("k_stft_mfft_direct") == ("2",),
    "spectrum output": lambda c, d: d["form"] == "spectrum",
    "power output": lambda c, d: d["form"] == "power",
    "bank output": lambda c, d: d["form"] == "bank" and d["filters"] == BANK_FILTERS,
}

# form: the output form the describe line of the case names; the GPU test runs the spectrum form of every case for the accuracy figure
# and the named form against it, word for word.
CASES = [
    dict(id="n18-l13-detrend", setup=1, n_fft=18, L=13, hop=5, mode=None, detrend=True, B=3, T=100,
         classes=("a schedule of only 3s", "the schedule 3x3 of n_fft 18", "64 rows per workgroup (4 lanes per row)", "a ragged last group",
                  "one group", "L below n_fft", "detrend", "detrend, L below 64 (idle partial sums)", "a schedule with neither (M odd)",
                  "n_fft not a multiple of the lanes (a lane without its last column)", "spectrum output")),
    dict(id="n20-reflect", setup=0, n_fft=20, L=20, hop=7, mode="reflect", detrend=False, B=5, T=500,
         classes=("a schedule with a last radix-2 pass", "reflect padding", "L = n_fft", "direct form 2")),
    dict(id="n30-l24-constant-power", setup=3, n_fft=30, L=24, hop=7, mode="constant", detrend=False, B=3, T=150, form="power",
         classes=("a schedule of 5s and 3s together", "constant padding", "power output")),
    dict(id="n50-nopad", setup=2, n_fft=50, L=50, hop=11, mode=None, detrend=False, B=2, T=300,
         classes=("a schedule of only 5s", "no padding, no detrending", "a pass with idle lanes")),
    dict(id="n54-l40-reflect", setup=1, n_fft=54, L=40, hop=9, mode="reflect", detrend=False, B=2, T=200,
         classes=("a first radix-3 pass of several trips",)),
    dict(id="n96-l80-detrend-padded", setup=2, n_fft=96, L=80, hop=37, mode=None, detrend=True, B=4, T=2000, padded=True,
         classes=("a schedule with radix-4 passes", "padded strides", "detrend, L above 64 and not a multiple of 64", "6 columns per lane",
                  "n_fft a multiple of the lanes, columns per lane not a power of two", "several rows per workgroup")),
    dict(id="n400-reflect-bank", setup=0, n_fft=400, L=400, hop=160, mode="reflect", detrend=False, B=2, T=4000, form="bank",
         classes=("the schedule 5x5x4x2 of n_fft 400", "a whole last group", "bank output")),
    dict(id="n480-l400-nopad-col0-power", setup=2, n_fft=480, L=400, hop=100, mode=None, detrend=False, B=3, T=2000, padded=True, form="power",
         classes=("the schedule 5x3x4x4 of n_fft 480", "no padding, the window off column 0", "padded strides", "power output")),
    dict(id="n1000-detrend", setup=4, n_fft=1000, L=1000, hop=300, mode=None, detrend=True, B=3, T=5000,
         classes=("two rows per workgroup", "detrend, L above 64 and not a multiple of 64")),
    dict(id="n1200-hop8-loop", setup=4, n_fft=1200, L=1200, hop=8, mode="reflect", detrend=False, B=1, T=17500,
         classes=("one row per workgroup", "more groups than workgroups (the group loop)")),
    dict(id="n1536-nopad-form1", setup=FORM1, n_fft=1536, L=1536, hop=512, mode=None, detrend=False, B=2, T=6000,
         classes=("direct form 1",)),
    dict(id="n2560-l2000-constant", setup=4, n_fft=2560, L=2000, hop=1300, mode="constant", detrend=False, B=2, T=6000,
         classes=("a first radix-5 pass with a butterfly per lane",)),
    dict(id="n4000-detrend", setup=0, n_fft=4000, L=4000, hop=5000, mode=None, detrend=True, B=2, T=10000,
         classes=("16 columns per lane", "a pass with two trips")),
    dict(id="n4050-reflect", setup=0, n_fft=4050, L=4050, hop=500, mode="reflect", detrend=False, B=2, T=17500,
         classes=("the schedule 5x5x3x3x3x3 of n_fft 4050", "a schedule with neither (M odd)", "16 columns per lane")),
]


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
