"""The case table of the mixed-radix fused window + complex FFT front for I/Q input (bhw_stft_cmfft_f32_*), in the manner of
tests/stft_cfft_cases.py: the call shapes that between them reach every class its planner (bhwp_stft_cmfft_plan) can emit, and the
classes each shape is there for.

A class is a predicate on the describe line of the call (B.describe_stft_cmfft), which has the words of the power-of-two I/Q line
(stft_cfft_cases.parse reads it) with the mixed-radix schedule and the entries of the twiddle table.

tests/test_stft_cmfft_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds, and that a sweep of the
planner over all 91 supported n_fft emits no pass shape and no row layout the table lacks; tests/test_gpu_stft_iq_mixed.py runs every
case, library and table, against numpy.fft.fft in float64 of the float32 rows.
"""
import re

from blackman_harris_win_amd import binding as B

import plan_cases as PC
import stft_cfft_cases as CC

SETUPS, params, FORM1 = PC.SETUPS, PC.params, PC.FORM1
MAX_GRID = CC.MAX_GRID
row_floats, pad_gaps, desc = CC.row_floats, CC.pad_gaps, CC.desc
SIZES = [n for n in range(1, 5000) if B.cmfft_supported(n)]


def parse(line):
    d = CC.parse(line)
    d["radices"] = [int(r) for r in d["schedule"].split("x")] if d["schedule"] else []
    m = re.search(r"(\d+) twiddles", line)
    d["fold"] = int(m.group(1)) if m else None
    return d


def pass_shapes(d):
    """{(radix, place, lanes)} of the passes of a parsed line: Q = n / radix butterflies on lpf lanes."""
    n, lpf, Ns, out = d["m"], d["lpf"], 1, set()
    for r in d["radices"]:
        Q = n // r
        place = "first" if Ns == 1 else "last" if Ns == Q else "middle"
        lanes = "idle" if Q < lpf else "exact" if Q == lpf else "several"
        out.add((r, place, lanes))
        Ns *= r
    assert Ns == n, d["line"]
    return out


def trips(d):
    """The trips of the lane loop in each pass: ceil(Q / lpf)."""
    return [-(-(d["m"] // r) // d["lpf"]) for r in d["radices"]]


def layout(d):
    """What the row steps branch on: (one row per workgroup, a lane without its last column, an odd n (the full twiddle table), 8
    columns per lane)."""
    return (d["fy"] == 1, d["n_fft"] % d["lpf"] != 0, d["n_fft"] % 2 == 1, d["cpl"] == 8)


def line(c, table=None):
    s, L, _, _, _, det = desc(c)
    return B.describe_stft_cmfft(params(c["setup"]), L, s, detrend=det, power=bool(c.get("power")), fftshift=bool(c.get("fftshift")), table=table)


CLASSES = {f"a radix-{r} pass": (lambda c, d, r=r: r in d["radices"]) for r in (5, 3, 4, 2)}
CLASSES.update({
    "no radix-2 or radix-4 pass (odd n)": lambda c, d: d["n_fft"] % 2 == 1 and not {2, 4} & set(d["radices"]),
    "seven passes": lambda c, d: len(d["radices"]) == 7,
    "odd n: the full twiddle table": lambda c, d: d["n_fft"] % 2 == 1 and d["fold"] == d["n_fft"],
    "even n: the folded twiddle table": lambda c, d: d["n_fft"] % 2 == 0 and d["fold"] == d["n_fft"] // 2,
    "a lane without its last column": lambda c, d: d["cpl"] * d["lpf"] > d["n_fft"],
    "cpl * lpf = n exactly": lambda c, d: d["cpl"] * d["lpf"] == d["n_fft"],
    "32 rows per workgroup": lambda c, d: d["fy"] == 32,
    "several rows per workgroup": lambda c, d: 1 < d["fy"] < 32,
    "one row per workgroup": lambda c, d: d["fy"] == 1,
    "3 columns per lane": lambda c, d: d["cpl"] == 3,
    "5 columns per lane": lambda c, d: d["cpl"] == 5,
    "8 columns per lane": lambda c, d: d["cpl"] == 8,
    "a pass with idle lanes": lambda c, d: any(lanes == "idle" for _, _, lanes in pass_shapes(d)),
    "a pass of two trips": lambda c, d: 2 in trips(d),
    "a radix-5 first pass on exactly lpf butterflies, a radix-4 last pass of several trips":
        lambda c, d: {(5, "first", "exact"), (4, "last", "several")} <= pass_shapes(d),
    "a ragged last group": lambda c, d: d["fy"] > 1 and d["rows"] % d["fy"] != 0,
    "a whole last group": lambda c, d: d["fy"] > 1 and d["rows"] % d["fy"] == 0,
    "one group": lambda c, d: d["groups"] == 1 and d["grid"] == 1,
    "more groups than workgroups (the group loop)": lambda c, d: d["groups"] > d["grid"] == MAX_GRID and d["fy"] >= 2,
    "reflect padding": lambda c, d: not d["detrend"] and d["pad"] > 0 and d["reflect"],
    "constant padding": lambda c, d: not d["detrend"] and d["pad"] > 0 and not d["reflect"],
    "no padding, the window off column 0": lambda c, d: not d["detrend"] and d["pad"] == 0 and d["col0"] > 0,
    "detrend, L below 64 (idle partial sums)": lambda c, d: d["detrend"] and c["L"] < 64,
    "detrend, L above 64 and not a multiple of 64": lambda c, d: d["detrend"] and c["L"] > 64 and c["L"] % 64 != 0,
    "padded strides": lambda c, d: bool(c.get("padded")),
    "direct form 1": lambda c, d: d["kernels"].get("k_stft_cmfft_direct") == ("1",),
    "direct form 2": lambda c, d: d["kernels"].get("k_stft_cmfft_direct") == ("2",),
    "power output": lambda c, d: d["power"],
    "power output, shifted bins": lambda c, d: d["power"] and d["shifted"],
    "spectrum output, shifted bins": lambda c, d: not d["power"] and d["shifted"],
    "spectrum output, shifted bins, odd n": lambda c, d: not d["power"] and d["shifted"] and d["n_fft"] % 2 == 1,
    "spectrum output, bins in order": lambda c, d: not d["power"] and not d["shifted"],
})

# power / fftshift: the output form the describe line of the case names; the GPU test runs the spectrum form of every case for the
# accuracy figure and the named form against it, word for word.
CASES = [
    dict(id="n18-l13-detrend", setup=1, n_fft=18, L=13, hop=5, mode=None, detrend=True, B=3, T=100,
         classes=("a radix-3 pass", "a radix-2 pass", "even n: the folded twiddle table", "a lane without its last column", "32 rows per workgroup",
                  "3 columns per lane", "a pass with idle lanes", "a ragged last group", "detrend, L below 64 (idle partial sums)",
                  "spectrum output, bins in order")),
    dict(id="n25-reflect-shift", setup=0, n_fft=25, L=25, hop=9, mode="reflect", detrend=False, B=1, T=280, fftshift=True,
         classes=("a radix-5 pass", "no radix-2 or radix-4 pass (odd n)", "odd n: the full twiddle table", "32 rows per workgroup", "reflect padding",
                  "direct form 2", "a whole last group", "one group", "spectrum output, shifted bins, odd n")),
    dict(id="n27-l20-nopad-col0-power-shift", setup=2, n_fft=27, L=20, hop=10, mode=None, detrend=False, B=3, T=300, padded=True, power=True,
         fftshift=True, classes=("no radix-2 or radix-4 pass (odd n)", "no padding, the window off column 0", "padded strides",
                                 "power output, shifted bins")),
    dict(id="n48-l37-constant-power", setup=3, n_fft=48, L=37, hop=13, mode="constant", detrend=False, B=3, T=150, power=True,
         classes=("a radix-4 pass", "cpl * lpf = n exactly", "several rows per workgroup", "3 columns per lane", "constant padding", "power output")),
    dict(id="n75-form1", setup=FORM1, n_fft=75, L=75, hop=20, mode="constant", detrend=False, B=2, T=1000,
         classes=("odd n: the full twiddle table", "several rows per workgroup", "direct form 1", "a pass with idle lanes")),
    dict(id="n100-l90-detrend-padded-shift", setup=2, n_fft=100, L=90, hop=37, mode=None, detrend=True, B=4, T=2000, padded=True, fftshift=True,
         classes=("padded strides", "detrend, L above 64 and not a multiple of 64", "spectrum output, shifted bins", "a lane without its last column")),
    dict(id="n400-reflect", setup=0, n_fft=400, L=400, hop=160, mode="reflect", detrend=False, B=2, T=4000,
         classes=("a radix-5 pass", "a radix-4 pass", "several rows per workgroup", "a whole last group")),
    dict(id="n400-hop1-loop", setup=4, n_fft=400, L=400, hop=1, mode="reflect", detrend=False, B=1, T=4200,
         classes=("more groups than workgroups (the group loop)", "a ragged last group")),
    dict(id="n1000-l900-detrend", setup=4, n_fft=1000, L=900, hop=300, mode=None, detrend=True, B=3, T=5000,
         classes=("one row per workgroup", "a radix-2 pass", "a pass of two trips")),
    dict(id="n1215-nopad", setup=2, n_fft=1215, L=1215, hop=400, mode=None, detrend=False, B=2, T=4000,
         classes=("5 columns per lane", "one row per workgroup", "odd n: the full twiddle table")),
    dict(id="n1280-l1000-constant", setup=0, n_fft=1280, L=1000, hop=700, mode="constant", detrend=False, B=2, T=3000,
         classes=("a radix-5 first pass on exactly lpf butterflies, a radix-4 last pass of several trips", "cpl * lpf = n exactly",
                  "5 columns per lane")),
    dict(id="n1458-detrend", setup=4, n_fft=1458, L=1458, hop=900, mode=None, detrend=True, B=2, T=5000,
         classes=("seven passes", "a radix-3 pass", "a pass of two trips")),
    dict(id="n1536-l1200-nopad-power", setup=0, n_fft=1536, L=1200, hop=384, mode=None, detrend=False, B=2, T=4000, power=True,
         classes=("cpl * lpf = n exactly", "even n: the folded twiddle table", "no padding, the window off column 0")),
    dict(id="n2000-l1500-reflect", setup=4, n_fft=2000, L=1500, hop=500, mode="reflect", detrend=False, B=2, T=6000,
         classes=("8 columns per lane", "even n: the folded twiddle table", "a lane without its last column", "reflect padding")),
    dict(id="n2025-detrend", setup=0, n_fft=2025, L=2025, hop=2500, mode=None, detrend=True, B=2, T=10000,
         classes=("8 columns per lane", "a lane without its last column", "odd n: the full twiddle table", "a pass of two trips")),
]


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
