"""The case table of the fused inverse mixed-radix complex FFT + overlap-add front for I/Q output (bhw_istft_cmfft_f32_*), in the
manner of tests/istft_cfft_cases.py and tests/stft_cmfft_cases.py, whose parsers and class predicates it imports: the call shapes that
between them reach every class its planner (bhwp_istft_cmfft_plan) can emit, and the classes each shape is there for.

A class is a predicate on the describe line of the call (B.describe_istft_cmfft), which has the words and fields of
describe_istft_cfft's line with the mixed-radix schedule and the entries of the twiddle table.  The classes are
  - the span classes of istft_cfft_cases.CLASSES (spans, halo, groups, grid, window, hop, length, normalisation, strides, the shift),
    without its power-of-two schedules, its power-of-two column counts, its kernel names and the grid-target class (whose smallest
    shape is 8 x 700 rows of 1024 and adds no branch of the kernel: S is a number the span walk takes as it comes);
  - the pass and layout classes of stft_cmfft_cases.CLASSES (radix, odd n, seven passes, the two forms of the twiddle table, a missing
    last column, the rows per workgroup, the columns per lane);
  - this kernel's own: the shift at an even and at an odd n, a hop above n_fft, the direct forms.

tests/test_istft_cmfft_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds, that a sweep of the
planner over all 91 supported n_fft emits no pass shape, layout or slot count the table lacks, and that every span's frame list is
exactly the frames that reach its outputs; tests/test_gpu_istft_iq_mixed.py runs every case, library and table, against numpy in
float64.
"""
import re

from blackman_harris_win_amd import binding as B

import istft_cfft_cases as IC
import stft_cmfft_cases as MC

SETUPS, params, FORM1 = IC.SETUPS, IC.params, IC.FORM1
MAX_GRID, TARGET_GROUPS, HALO_FACTOR = MC.MAX_GRID, IC.TARGET_GROUPS, IC.HALO_FACTOR
geometry, strides, desc, span_frames = IC.geometry, IC.strides, IC.desc, IC.span_frames
pass_shapes, trips, layout, SIZES = MC.pass_shapes, MC.trips, MC.layout, MC.SIZES


def parse(line):
    """istft_cfft_cases.parse, plus the radices of the schedule and the twiddle entries as stft_cmfft_cases.parse gives them."""
    d = IC.parse(line)
    d["radices"] = [int(r) for r in d["schedule"].split("x")] if d["schedule"] else []
    m = re.search(r"(\d+) twiddles", line)
    d["fold"] = int(m.group(1)) if m else None
    return d


def line(c, table=None):
    s, L = desc(c)[:2]
    return B.describe_istft_cmfft(params(c["setup"]), L, s, normalize=c["normalize"], fftshift=bool(c.get("fftshift")), table=table)


_SPAN = ("a signal in one span", "a signal cut into several spans, halo frames recomputed", "a span shorter than its halo", "a ragged last span",
         "slots of one workgroup in different signals", "an idle slot in the last group", "more groups than workgroups (the group loop)",
         "L below n_fft", "L = n_fft", "center on", "center off", "hop above L (zeros inside the signal)", "hop not dividing L",
         "length past the frames' extent", "length short of torch's default", "normalised", "raw", "padded strides", "bins shifted",
         "bins in order", "x off the 8-byte grid with an odd stride", "heavy overlap named in the line")
_PASS = ("a radix-5 pass", "a radix-3 pass", "a radix-4 pass", "a radix-2 pass", "no radix-2 or radix-4 pass (odd n)", "seven passes",
         "odd n: the full twiddle table", "even n: the folded twiddle table", "a lane without its last column", "cpl * lpf = n exactly",
         "32 rows per workgroup", "several rows per workgroup", "one row per workgroup", "3 columns per lane", "5 columns per lane",
         "8 columns per lane", "a pass with idle lanes", "a pass of two trips")

CLASSES = {name: IC.CLASSES[name] for name in _SPAN}
CLASSES.update({name: MC.CLASSES[name] for name in _PASS})
CLASSES.update({
    "bins shifted, even n": lambda c, d: d["shifted"] and d["n_fft"] % 2 == 0,
    "bins shifted, odd n": lambda c, d: d["shifted"] and d["n_fft"] % 2 == 1,
    "hop above n_fft (the ring's base steps by hop mod n_fft)": lambda c, d: c["hop"] > c["n_fft"],
    "direct form 1": lambda c, d: d["kernels"].get("k_istft_cmfft_direct") == ("1",),
    "direct form 2": lambda c, d: d["kernels"].get("k_istft_cmfft_direct") == ("2",),
})

# B * F: at least 50 rows (the GPU test's ratio gate lets single rows weigh below that), a few thousand at most
CASES = [
    dict(id="n18-l13", setup=1, n_fft=18, L=13, hop=5, center=True, normalize=True, B=3, F=18,
         classes=("a radix-3 pass", "a radix-2 pass", "even n: the folded twiddle table", "a lane without its last column", "32 rows per workgroup",
                  "3 columns per lane", "a pass with idle lanes", "L below n_fft", "center on", "hop not dividing L",
                  "a signal cut into several spans, halo frames recomputed", "slots of one workgroup in different signals", "normalised",
                  "an idle slot in the last group", "bins in order")),
    dict(id="n25-one-span-raw-shift", setup=0, n_fft=25, L=25, hop=12, center=True, normalize=False, B=13, F=4, extra=-1, fftshift=True,
         classes=("a radix-5 pass", "no radix-2 or radix-4 pass (odd n)", "odd n: the full twiddle table", "a signal in one span", "L = n_fft",
                  "raw", "direct form 2", "bins shifted", "bins shifted, odd n")),
    dict(id="n27-l20-short-odd", setup=3, n_fft=27, L=20, hop=7, center=True, normalize=True, B=3, F=40, extra=-9, odd=True,
         classes=("no radix-2 or radix-4 pass (odd n)", "a ragged last span", "length short of torch's default",
                  "x off the 8-byte grid with an odd stride")),
    dict(id="n48-hop4-few-frames", setup=3, n_fft=48, L=48, hop=4, center=True, normalize=True, B=9, F=6, extra=90,
         classes=("a radix-4 pass", "cpl * lpf = n exactly", "several rows per workgroup", "3 columns per lane", "a span shorter than its halo",
                  "length past the frames' extent")),
    dict(id="n75-nocenter-form1", setup=FORM1, n_fft=75, L=75, hop=29, center=False, normalize=True, B=2, F=44,
         classes=("odd n: the full twiddle table", "several rows per workgroup", "center off", "direct form 1", "a pass with idle lanes",
                  "hop not dividing L")),
    dict(id="n100-l90-padded-long-shift", setup=2, n_fft=100, L=90, hop=37, center=True, normalize=True, B=4, F=50, extra=300, padded=True,
         fftshift=True, classes=("padded strides", "length past the frames' extent", "bins shifted", "bins shifted, even n",
                                 "a lane without its last column")),
    dict(id="n100-l40-hop300", setup=2, n_fft=100, L=40, hop=300, center=True, normalize=True, B=11, F=5, padded=True,
         classes=("hop above L (zeros inside the signal)", "hop above n_fft (the ring's base steps by hop mod n_fft)", "padded strides")),
    dict(id="n400", setup=0, n_fft=400, L=400, hop=160, center=True, normalize=True, B=2, F=26,
         classes=("a radix-5 pass", "a radix-4 pass", "several rows per workgroup", "a signal cut into several spans, halo frames recomputed")),
    dict(id="n1000-l900-raw", setup=4, n_fft=1000, L=900, hop=300, center=True, normalize=False, B=3, F=17,
         classes=("one row per workgroup", "a radix-2 pass", "a pass of two trips", "raw")),
    dict(id="n1215-nocenter-shift", setup=2, n_fft=1215, L=1215, hop=400, center=False, normalize=True, B=5, F=12, fftshift=True,
         classes=("5 columns per lane", "one row per workgroup", "odd n: the full twiddle table", "center off", "bins shifted, odd n")),
    dict(id="n1280-l1000", setup=0, n_fft=1280, L=1000, hop=700, center=True, normalize=True, B=7, F=8,
         classes=("cpl * lpf = n exactly", "5 columns per lane")),
    dict(id="n1458", setup=4, n_fft=1458, L=1458, hop=365, center=True, normalize=True, B=5, F=12,
         classes=("seven passes", "a radix-3 pass", "a pass of two trips")),
    dict(id="n1536-l1200-shift", setup=0, n_fft=1536, L=1200, hop=384, center=True, normalize=True, B=4, F=16, fftshift=True,
         classes=("cpl * lpf = n exactly", "even n: the folded twiddle table", "bins shifted, even n")),
    dict(id="n2000-l100-loop", setup=4, n_fft=2000, L=100, hop=200, center=True, normalize=True, B=1, F=2047, extra=1000,
         classes=("more groups than workgroups (the group loop)", "8 columns per lane", "a lane without its last column")),
    dict(id="n2000-hop16-heavy", setup=4, n_fft=2000, L=2000, hop=16, center=True, normalize=True, B=1, F=1100,
         classes=("heavy overlap named in the line",)),
    dict(id="n2025", setup=0, n_fft=2025, L=2025, hop=506, center=True, normalize=True, B=5, F=12,
         classes=("8 columns per lane", "a lane without its last column", "odd n: the full twiddle table", "a pass of two trips")),
]


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
