"""The case table of the fused inverse mixed-radix FFT + overlap-add front (bhw_istft_mfft_f32_*), in the manner of
tests/istft_fft_cases.py and tests/stft_mfft_cases.py, whose parsers and class predicates it imports: the call shapes that between them
reach every class its planner (bhwp_istft_mfft_plan) can emit, and the classes each shape is there for.

A class is a predicate on the describe line of the call (B.describe_istft_mfft), which has the words and fields of
describe_istft_fft's line with the mixed-radix schedule text.  The classes are
  - the span classes of istft_fft_cases.CLASSES (spans, halo, groups, grid, window, hop, length, normalisation, strides), without its
    power-of-two schedules, its power-of-two column counts (4 and 8 columns per lane come from n_fft = lpf * cpl, which never holds
    here), its kernel names and its benchmarked batch;
  - the per-pass shape and layout classes of stft_mfft_cases.CLASSES (radix; first / middle / last; idle / exact / several trips; the
    lane and column layout);
  - two of this kernel's own: M odd, where the pre-split has no self-mirrored bin, and a lane whose last ring column is missing.

tests/test_istft_mfft_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds, that a sweep of the
planner over every supported n_fft emits no pass shape, layout, slot count or column count the table lacks, and that every span's frame
list is exactly the frames that reach its outputs; tests/test_gpu_istft_mixed.py runs every case, library and table, against numpy in
float64.
"""
from blackman_harris_win_amd import binding as B

import istft_fft_cases as IC
import stft_mfft_cases as MC

SETUPS, params, FORM1 = IC.SETUPS, IC.params, IC.FORM1
MAX_GRID, TARGET_GROUPS, HALO_FACTOR = MC.MAX_GRID, IC.TARGET_GROUPS, IC.HALO_FACTOR
geometry, span_frames, pass_shapes, layout = IC.geometry, IC.span_frames, MC.pass_shapes, MC.layout


def parse(line):
    """istft_fft_cases.parse, plus the radices of the schedule as stft_mfft_cases.parse gives them."""
    d = IC.parse(line)
    d["radices"] = [int(r) for r in d["schedule"].split("x")] if d["schedule"] else []
    return d


def desc(c):
    """istft_fft_cases.desc: (descriptor, L, col0, pad, length).  Its padded gaps are even, as complex64 rows need."""
    return IC.desc(c)


def line(c, table=None):
    s, L = desc(c)[:2]
    return B.describe_istft_mfft(params(c["setup"]), L, s, normalize=c["normalize"], table=table)


_SPAN = ("a signal in one span", "a signal cut into several spans, halo frames recomputed", "a span shorter than its halo", "a ragged last span",
         "slots of one workgroup in different signals", "an idle slot in the last group", "more groups than workgroups (the group loop)",
         "S set by the grid target", "L below n_fft", "L = n_fft", "center on", "center off", "hop above L (zeros inside the signal)",
         "hop not dividing L", "length past the frames' extent", "length short of torch's default", "normalised", "raw", "padded strides",
         "heavy overlap named in the line")
_PASS = ("a schedule of only 3s", "a schedule of only 5s", "a schedule of 5s and 3s together", "a schedule with radix-4 passes",
         "a schedule with a last radix-2 pass", "a schedule with neither (M odd)", "the schedule 5x5x4x2 of n_fft 400",
         "the schedule 5x3x4x4 of n_fft 480", "the schedule 3x3 of n_fft 18", "the schedule 5x5x3x3x3x3 of n_fft 4050",
         "64 rows per workgroup (4 lanes per row)", "several rows per workgroup", "two rows per workgroup", "one row per workgroup",
         "n_fft not a multiple of the lanes (a lane without its last column)",
         "n_fft a multiple of the lanes, columns per lane not a power of two", "6 columns per lane", "16 columns per lane",
         "a pass with idle lanes", "a pass with two trips", "a first radix-3 pass of several trips",
         "a first radix-5 pass with a butterfly per lane")

CLASSES = {name: IC.CLASSES[name] for name in _SPAN}
CLASSES.update({name: MC.CLASSES[name] for name in _PASS})
CLASSES.update({
    "M odd (no self-mirrored bin)": lambda c, d: d["m"] % 2 == 1,
    "M even (bin M / 2 is its own mirror)": lambda c, d: d["m"] % 2 == 0,
    "a lane's last ring column missing": lambda c, d: d["lpf"] * d["cpl"] > d["n_fft"] > d["lpf"] * (d["cpl"] - 1),
    "hop above n_fft (the ring's base steps by hop mod n_fft)": lambda c, d: c["hop"] > c["n_fft"],
    "direct form 1": lambda c, d: d["kernels"].get("k_istft_mfft_direct") == ("1",),
    "direct form 2": lambda c, d: d["kernels"].get("k_istft_mfft_direct") == ("2",),
    "the inverse of the mixed-radix benchmarked batch (64 x 998 x 201, 400 / 400 / 160)": lambda c, d: (d["signals"], d["frames"], d["n_fft"],
                                                                                                        d["L"], d["fy"]) == (64, 998, 400, 400, 4)
    and c["hop"] == 160,
})

CASES = [
    dict(id="n18-l13", setup=1, n_fft=18, L=13, hop=5, center=True, normalize=True, B=3, F=18,
         classes=("the schedule 3x3 of n_fft 18", "a schedule of only 3s", "a schedule with neither (M odd)", "M odd (no self-mirrored bin)",
                  "64 rows per workgroup (4 lanes per row)", "a lane's last ring column missing",
                  "n_fft not a multiple of the lanes (a lane without its last column)", "L below n_fft", "center on", "hop not dividing L",
                  "a signal cut into several spans, halo frames recomputed", "slots of one workgroup in different signals", "normalised",
                  "an idle slot in the last group")),
    dict(id="n20-one-span-raw", setup=0, n_fft=20, L=20, hop=10, center=True, normalize=False, B=5, F=4,
         classes=("a schedule with a last radix-2 pass", "M even (bin M / 2 is its own mirror)", "a signal in one span", "L = n_fft", "raw",
                  "direct form 2")),
    dict(id="n30-l24-short", setup=3, n_fft=30, L=24, hop=7, center=True, normalize=True, B=3, F=40, extra=-9,
         classes=("a schedule of 5s and 3s together", "M odd (no self-mirrored bin)", "a ragged last span", "length short of torch's default")),
    dict(id="n50-hop4-few", setup=3, n_fft=50, L=50, hop=4, center=True, normalize=True, B=2, F=6, extra=90,
         classes=("a schedule of only 5s", "a pass with idle lanes", "a span shorter than its halo", "length past the frames' extent")),
    dict(id="n54-l40-padded-long", setup=2, n_fft=54, L=40, hop=9, center=True, normalize=True, B=4, F=50, extra=300, padded=True,
         classes=("a first radix-3 pass of several trips", "padded strides", "length past the frames' extent")),
    dict(id="n96-nocenter-form1", setup=FORM1, n_fft=96, L=96, hop=37, center=False, normalize=True, B=2, F=44,
         classes=("a schedule with radix-4 passes", "6 columns per lane", "n_fft a multiple of the lanes, columns per lane not a power of two",
                  "several rows per workgroup", "center off", "direct form 1", "hop not dividing L")),
    dict(id="n250-l100-hop300", setup=2, n_fft=250, L=100, hop=300, center=True, normalize=True, B=3, F=5, padded=True,
         classes=("hop above L (zeros inside the signal)", "hop above n_fft (the ring's base steps by hop mod n_fft)",
                  "M odd (no self-mirrored bin)", "padded strides")),
    dict(id="n400", setup=0, n_fft=400, L=400, hop=160, center=True, normalize=True, B=2, F=26,
         classes=("the schedule 5x5x4x2 of n_fft 400", "a signal cut into several spans, halo frames recomputed")),
    dict(id="n480-l400-raw", setup=4, n_fft=480, L=400, hop=100, center=True, normalize=False, B=3, F=15,
         classes=("the schedule 5x3x4x4 of n_fft 480", "raw", "L below n_fft")),
    dict(id="n1000-raw", setup=4, n_fft=1000, L=1000, hop=300, center=True, normalize=False, B=3, F=15,
         classes=("two rows per workgroup", "raw")),
    dict(id="n1200-nocenter", setup=4, n_fft=1200, L=1200, hop=300, center=False, normalize=True, B=1, F=20,
         classes=("one row per workgroup", "center off")),
    dict(id="n1200-hop8-heavy", setup=4, n_fft=1200, L=1200, hop=8, center=True, normalize=True, B=1, F=1100,
         classes=("heavy overlap named in the line",)),
    dict(id="n1536", setup=0, n_fft=1536, L=1536, hop=512, center=True, normalize=True, B=2, F=8,
         classes=("a schedule with radix-4 passes",)),
    dict(id="n2560-l100-loop", setup=4, n_fft=2560, L=100, hop=200, center=True, normalize=True, B=1, F=2047, extra=1000,
         classes=("more groups than workgroups (the group loop)", "a first radix-5 pass with a butterfly per lane")),
    dict(id="n4000", setup=0, n_fft=4000, L=4000, hop=1000, center=True, normalize=True, B=2, F=8,
         classes=("16 columns per lane", "a pass with two trips")),
    dict(id="n4050", setup=0, n_fft=4050, L=4050, hop=1000, center=True, normalize=True, B=2, F=8,
         classes=("the schedule 5x5x3x3x3x3 of n_fft 4050", "M odd (no self-mirrored bin)", "16 columns per lane",
                  "a lane's last ring column missing")),
    dict(id="bench-64x998x201", setup=0, n_fft=400, L=400, hop=160, center=True, normalize=True, B=64, F=998,
         classes=("the inverse of the mixed-radix benchmarked batch (64 x 998 x 201, 400 / 400 / 160)", "S set by the grid target")),
]


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
