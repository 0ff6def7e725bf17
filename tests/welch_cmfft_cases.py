"""The case table of the fused Welch PSD for I/Q input at a mixed-radix n_fft (bhw_welch_cmfft_f32_*), in the manner of
tests/welch_cfft_cases.py: the call shapes that between them reach every branch the kernel's text takes (bhw_welch_cmfft.hip) and
every class its planner (bhwp_welch_cmfft_plan) can emit, and the classes each shape is there for.

A class is a predicate on the describe line of the call (B.describe_welch_cmfft): bhw_describe_stft_cmfft's fields in the same words
(without the output form; stft_cmfft_cases.parse reads them), plus the chunk, the runs, the frames and groups of a run, the
accumulators a lane carries, the chunks and blocks per signal and the workspace bytes (welch_cfft_cases' fields).  The layout is
lpf = the smallest power of two >= n / 4, clamped to 4..256, lanes on a row and fy = 256 / lpf rows side by side: fy 32 for n_fft 18
.. 30, 16 up to 60 (whole chunks per group, nothing carried) and 8, 4, 2, 1 from 72 on (carried sums, ceil(n_fft / 256)
accumulators, 8 at 2025).

tests/test_welch_cmfft_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds, that a sweep of the
planner over all 91 supported n_fft emits no class the table lacks, and that the shared fields equal describe_stft_cmfft's;
tests/test_gpu_welch_iq_mixed.py runs every case, library and table, shifted and not, word for word against the contract restated on
bhw.stft_iq_mixed's rows.
"""
from blackman_harris_win_amd import binding as B

import plan_cases as PC
import stft_cmfft_cases as MC
import welch_cfft_cases as WC

SETUPS, params, FORM1, N16 = PC.SETUPS, PC.params, PC.FORM1, PC.N16
CHUNK, BLOCK, MAX_GRID = B.WELCH_FFT_CHUNK, B.WELCH_BLOCK, MC.MAX_GRID
SIZES = [n for n in MC.SIZES if n < 2048]
frames_to_samples, desc, workspace_doubles = WC.frames_to_samples, WC.desc, WC.workspace_doubles


def parse(line):
    d = MC.parse(line)
    d.update({k: v for k, v in WC.parse(line).items() if k in WC._FIELDS or k == "joins"})
    return d


def schedule(n):
    """The planner's rule as text: the radix-5 passes of n, its radix-3 passes, the radix-4 passes, one radix-2 pass."""
    out = []
    for r in (5, 3, 4, 2):
        while n % r == 0:
            out.append(str(r))
            n //= r
    assert n == 1
    return "x".join(out)


def layout(n):
    """(lpf, fy) of n_fft n: the header's rule."""
    lpf = 4
    while lpf < 256 and 4 * lpf < n:
        lpf *= 2
    return lpf, 256 // lpf


def line(c, table=None, fftshift=False):
    s, L, _, det = desc(c)
    return B.describe_welch_cmfft(params(c["setup"]), L, s, detrend=det, fftshift=fftshift, table=table)


def regime(d):
    """What the accumulating epilogue branches on, a function of n_fft alone: the rows side by side (whole chunks per group from 16
    on, carried sums below), the groups of a run and the accumulators a lane carries."""
    return (d["fy"], d["gpr"], d["acc"])


CLASSES = {
    "fy 32, two chunks per group": lambda c, d: d["fy"] == 2 * CHUNK and d["gpr"] == 1 and d["acc"] == 0,
    "fy equal to the chunk": lambda c, d: d["fy"] == CHUNK and d["gpr"] == 1 and d["acc"] == 0,
    "fy equal to the chunk, odd n": lambda c, d: d["fy"] == CHUNK and d["n_fft"] % 2 == 1,
    "fy 8, one accumulator, most lanes idle": lambda c, d: d["fy"] == 8 and d["acc"] == 1 and d["n_fft"] < 128,
    "fy 8, odd n": lambda c, d: d["fy"] == 8 and d["n_fft"] % 2 == 1,
    "fy 4": lambda c, d: d["fy"] == 4 and d["gpr"] == 4 and d["acc"] == 1,
    "fy 2, 2 accumulators": lambda c, d: d["fy"] == 2 and d["gpr"] == 8 and d["acc"] == 2,
    "fy 1 (sixteen groups per run)": lambda c, d: d["fy"] == 1 and d["gpr"] == CHUNK,
    "3 accumulators per lane": lambda c, d: d["acc"] == 3,
    "4 accumulators per lane": lambda c, d: d["acc"] == 4,
    "5 accumulators per lane": lambda c, d: d["acc"] == 5,
    "6 accumulators per lane, a last radix-2 pass": lambda c, d: d["acc"] == 6 and d["radices"][-1] == 2,
    "7 accumulators per lane": lambda c, d: d["acc"] == 7,
    "8 accumulators per lane, even n": lambda c, d: d["acc"] == 8 and d["n_fft"] % 2 == 0,
    "8 accumulators per lane, odd n, 8 columns per lane": lambda c, d: d["acc"] == 8 and d["n_fft"] % 2 == 1 and d["cpl"] == 8,
    "carried sums, odd n, fy 1": lambda c, d: d["fy"] == 1 and d["n_fft"] % 2 == 1,
    "seven passes": lambda c, d: len(d["radices"]) == 7,
    "a ragged last chunk": lambda c, d: d["frames"] % CHUNK != 0 and d["frames"] > CHUNK,
    "a whole last chunk": lambda c, d: d["frames"] % CHUNK == 0,
    "exactly one chunk": lambda c, d: d["frames"] == CHUNK and d["chunks"] == 1,
    "F below a chunk": lambda c, d: d["frames"] < CHUNK and d["chunks"] == 1,
    "F = 1": lambda c, d: d["frames"] == 1,
    "F = 15": lambda c, d: d["frames"] == 15,
    "two or more runs per signal": lambda c, d: d["runs"] >= 2 * d["signals"],
    "a run whose second chunk is padding": lambda c, d: d["fy"] == 2 * CHUNK and -(-d["frames"] // CHUNK) % 2 == 1,
    "one block (one join launch)": lambda c, d: d["blocks"] == 1 and d["joins"] == 1,
    "several blocks (two join launches)": lambda c, d: d["blocks"] > 1 and d["joins"] == 2,
    "two blocks, the second of 3 frames": lambda c, d: d["blocks"] == 2 and d["frames"] - BLOCK == 3,
    "three blocks": lambda c, d: d["blocks"] == 3,
    "more runs than workgroups (the run loop)": lambda c, d: d["runs"] > d["grid"] == MAX_GRID,
    "513 blocks through the join": lambda c, d: d["blocks"] == 513,
    "one signal": lambda c, d: d["signals"] == 1,
    "several signals": lambda c, d: d["signals"] > 1,
    "a padded p_stride": lambda c, d: bool(c.get("padded")),
    "detrend": lambda c, d: d["detrend"],
    "no padding, no detrending": lambda c, d: not d["detrend"] and d["pad"] == 0,
    "L below n_fft": lambda c, d: c["L"] < c["n_fft"],
    "a centred, reflect-padded descriptor": lambda c, d: not d["detrend"] and d["pad"] > 0 and d["reflect"],
    "direct form 1": lambda c, d: d["kernels"].get("k_welch_cmfft_direct") == ("1",),
    "direct form 2": lambda c, d: d["kernels"].get("k_welch_cmfft_direct") == ("2",),
}

CASES = [
    dict(id="n18-2x70", setup=1, n_fft=18, L=18, hop=4, mode=None, detrend=False, B=2, F=70,
         classes=("fy 32, two chunks per group", "a ragged last chunk", "two or more runs per signal", "a run whose second chunk is padding",
                  "one block (one join launch)", "several signals", "no padding, no detrending")),
    dict(id="n45-l40-detrend-1x16", setup=3, n_fft=45, L=40, hop=8, mode=None, detrend=True, B=1, F=16,
         classes=("fy equal to the chunk", "fy equal to the chunk, odd n", "exactly one chunk", "a whole last chunk", "one signal", "detrend",
                  "L below n_fft")),
    dict(id="n60-3x17", setup=2, n_fft=60, L=60, hop=8, mode=None, detrend=False, B=3, F=17,
         classes=("fy equal to the chunk", "a ragged last chunk")),
    dict(id="n75-l60-detrend-2x33", setup=0, n_fft=75, L=60, hop=32, mode=None, detrend=True, B=2, F=33,
         classes=("fy 8, one accumulator, most lanes idle", "fy 8, odd n", "direct form 2")),
    dict(id="n200-l160-detrend-2x40", setup=FORM1, n_fft=200, L=160, hop=64, mode=None, detrend=True, B=2, F=40,
         classes=("fy 4", "direct form 1")),
    dict(id="n400-3x259", setup=0, n_fft=400, L=400, hop=160, mode=None, detrend=False, B=3, F=259,
         classes=("fy 2, 2 accumulators", "several blocks (two join launches)", "two blocks, the second of 3 frames")),
    dict(id="n600-2x19", setup=2, n_fft=600, L=600, hop=150, mode=None, detrend=False, B=2, F=19,
         classes=("fy 1 (sixteen groups per run)", "3 accumulators per lane")),
    dict(id="n1000-1x21-padded", setup=4, n_fft=1000, L=1000, hop=250, mode=None, detrend=False, B=1, F=21, padded=True,
         classes=("4 accumulators per lane", "a padded p_stride")),
    dict(id="n1215-l1000-detrend-1x18", setup=4, n_fft=1215, L=1000, hop=300, mode=None, detrend=True, B=1, F=18,
         classes=("5 accumulators per lane", "carried sums, odd n, fy 1")),
    dict(id="n1458-detrend-2x17", setup=4, n_fft=1458, L=1458, hop=400, mode=None, detrend=True, B=2, F=17,
         classes=("seven passes",)),
    dict(id="n1536-1x20", setup=0, n_fft=1536, L=1536, hop=384, mode=None, detrend=False, B=1, F=20,
         classes=("6 accumulators per lane, a last radix-2 pass",)),
    dict(id="n1600-1x17", setup=0, n_fft=1600, L=1600, hop=400, mode=None, detrend=False, B=1, F=17,
         classes=("7 accumulators per lane",)),
    dict(id="n2000-l1500-1x18", setup=4, n_fft=2000, L=1500, hop=500, mode=None, detrend=False, B=1, F=18,
         classes=("8 accumulators per lane, even n",)),
    dict(id="n2025-detrend-1x35", setup=0, n_fft=2025, L=2025, hop=512, mode=None, detrend=True, B=1, F=35,
         classes=("8 accumulators per lane, odd n, 8 columns per lane",)),
    dict(id="n60-2x600", setup=2, n_fft=60, L=60, hop=16, mode=None, detrend=False, B=2, F=600,
         classes=("three blocks",)),
    dict(id="n18-l16-1x131142", setup=N16, n_fft=18, L=16, hop=2, mode=None, detrend=False, B=1, F=131142,
         classes=("more runs than workgroups (the run loop)", "513 blocks through the join", "L below n_fft")),
    dict(id="n96-2x1", setup=0, n_fft=96, L=96, hop=48, mode=None, detrend=False, B=2, F=1,
         classes=("F below a chunk", "F = 1")),
    dict(id="n400-detrend-2x15", setup=4, n_fft=400, L=400, hop=100, mode=None, detrend=True, B=2, F=15,
         classes=("F below a chunk", "F = 15")),
    dict(id="n300-l200-reflect", setup=2, n_fft=300, L=200, hop=64, mode="reflect", detrend=False, B=2, T=3000,
         classes=("a centred, reflect-padded descriptor",)),
]

# BHW_CFFT_SHIFT: one case of each regime, an odd n in each, and 2025 (the GPU test runs every case shifted as well; these are the ones
# the table names)
SHIFTED = ("n18-2x70", "n45-l40-detrend-1x16", "n75-l60-detrend-2x33", "n400-3x259", "n2025-detrend-1x35")


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
