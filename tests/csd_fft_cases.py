"""The case table of the fused Welch cross spectra (bhw_csd_fft_f32_*), in the manner of tests/welch_fft_cases.py: the call shapes that
between them reach every branch the kernel's text takes (bhw_csd_fft.hip) and every class its planner (bhwp_csd_fft_plan) can emit, and
the classes each shape is there for.

A class is a predicate on the describe line of the call (B.describe_csd_fft): bhw_describe_welch_fft's fields in the same words for the
pair plan -- frames of x and of y side by side, so `fy` rows per workgroup are fy / 2 frame pairs and a run is max(16, fy / 2) frames --
plus the pairs per group, the outputs and the chains.  With 32 pairs per group at n_fft 16 the 70 frames of the first case are three
runs per signal (the fused Welch PSD, 64 frames per group, has two there): the class is "several runs per signal".

tests/test_csd_fft_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds, that a sweep of the planner
over every supported n_fft emits no shape the table lacks, and that the shared fields equal describe_stft_fft's but for the lanes of a
row at n_fft 2048; tests/test_gpu_csd_fft.py runs every case, library and table, word for word against the contract restated on
bhw.stft's rows of x and of y.
"""
import re

from blackman_harris_win_amd import binding as B

import plan_cases as PC
import stft_fft_cases as SF
import welch_fft_cases as WC

SETUPS, params, FORM1, N16 = PC.SETUPS, PC.params, PC.FORM1, PC.N16
CHUNK, BLOCK, MAX_GRID = B.WELCH_FFT_CHUNK, B.WELCH_BLOCK, SF.MAX_GRID
ALL = ("pxy", "pxx", "pyy", "coherence", "h1")
SCHEDULES = {n: s for n, s in SF.SCHEDULES.items() if n <= 2048}

_FIELDS = dict(WC._FIELDS)
_FIELDS.update({"pairs": r"(\d+) frame pairs? per group", "chains": r"(\d+) chains"})


def parse(line):
    d = SF.parse(line)
    for name, pat in _FIELDS.items():
        m = re.search(pat, line)
        if m:
            d[name] = int(m.group(1))
    d["joins"] = 2 if "twice" in line else 1
    d["broadcast"] = "x broadcast" in line
    d["onesided"] = "one-sided" in line
    m = re.search(r"-sided, ([a-z0-9+]+);", line)
    d["outputs"] = tuple(m.group(1).split("+")) if m else ()
    return d


frames_to_samples = WC.frames_to_samples
desc = WC.desc


def line(c, table=None, outputs=ALL):
    s, L, _, det = desc(c)
    return B.describe_csd_fft(params(c["setup"]), L, s, detrend=det, outputs=outputs, broadcast_x=bool(c.get("bcast")), table=table)


def workspace_doubles(nb, F, K):
    """The workspace formula of include/bhw.h: four times the fused Welch PSD's."""
    return 4 * WC.workspace_doubles(nb, F, K)


CLASSES = {f"schedule {s} (n_fft {n})": (lambda c, d, n=n, s=s: d["n_fft"] == n and d["schedule"] == s) for n, s in SCHEDULES.items()}
CLASSES.update({
    "several chunks per group": lambda c, d: d["pairs"] > CHUNK and d["gpr"] == 1 and d["acc"] == 0 and d["run"] == d["pairs"],
    "pair-group = chunk": lambda c, d: d["pairs"] == CHUNK and d["gpr"] == 1 and d["acc"] == 0,
    "first carried regime (two groups per run)": lambda c, d: d["pairs"] == CHUNK // 2 and d["gpr"] == 2 and d["acc"] == 1 and d["n_fft"] == 128,
    "carried regime": lambda c, d: 1 < d["pairs"] < CHUNK and d["gpr"] == CHUNK // d["pairs"] and d["acc"] >= 1,
    "one frame pair per group (sixteen groups per run)": lambda c, d: d["pairs"] == 1 and d["fy"] == 2 and d["gpr"] == CHUNK,
    "1 accumulator per lane and chain": lambda c, d: d["acc"] == 1,
    "2 accumulators per lane and chain (K = 257 on 256 lanes)": lambda c, d: d["acc"] == 2 and d["n_fft"] == 512,
    "3 accumulators per lane and chain": lambda c, d: d["acc"] == 3 and d["n_fft"] == 1024,
    "5 accumulators per lane and chain (the most)": lambda c, d: d["acc"] == 5 and d["n_fft"] == 2048,
    "two butterflies per lane": lambda c, d: d["n_fft"] == 2048 and d["lpf"] == 128 and d["cpl"] == 16,
    "four chains": lambda c, d: d["chains"] == 4,
    "a ragged last chunk": lambda c, d: d["frames"] % CHUNK != 0 and d["frames"] > CHUNK,
    "a whole last chunk": lambda c, d: d["frames"] % CHUNK == 0,
    "exactly one chunk": lambda c, d: d["frames"] == CHUNK and d["chunks"] == 1,
    "F below a chunk": lambda c, d: d["frames"] < CHUNK and d["chunks"] == 1,
    "F = 1": lambda c, d: d["frames"] == 1,
    "F = 15": lambda c, d: d["frames"] == 15,
    "several runs per signal": lambda c, d: d["runs"] > d["signals"] and d["runs"] <= d["grid"],
    "one block (one join launch)": lambda c, d: d["blocks"] == 1 and d["joins"] == 1,
    "several blocks (two join launches)": lambda c, d: d["blocks"] > 1 and d["joins"] == 2,
    "a ragged last block": lambda c, d: d["blocks"] > 1 and d["frames"] % BLOCK != 0,
    "two blocks, the second of 3 frames": lambda c, d: d["blocks"] == 2 and d["frames"] - BLOCK == 3,
    "three blocks": lambda c, d: d["blocks"] == 3,
    "more runs than workgroups (the run loop)": lambda c, d: d["runs"] > d["grid"] == MAX_GRID,
    "513 blocks through the join": lambda c, d: d["blocks"] == 513,
    "one signal": lambda c, d: d["signals"] == 1,
    "several signals": lambda c, d: d["signals"] > 1,
    "a padded output stride": lambda c, d: bool(c.get("padded")),
    "detrend": lambda c, d: d["detrend"],
    "no padding, no detrending": lambda c, d: not d["detrend"] and d["pad"] == 0,
    "L below n_fft": lambda c, d: c["L"] < c["n_fft"],
    "a centred, reflect-padded descriptor": lambda c, d: not d["detrend"] and d["pad"] > 0 and d["reflect"],
    "broadcast x": lambda c, d: d["broadcast"] and d["signals"] > 1,
    "direct form 1": lambda c, d: d["kernels"].get("k_csd_fft_direct") == ("1",),
    "direct form 2": lambda c, d: d["kernels"].get("k_csd_fft_direct") == ("2",),
})

CASES = [
    dict(id="n16-2x70", setup=1, n_fft=16, L=16, hop=4, mode=None, detrend=False, B=2, F=70,
         classes=("schedule 4x2 (n_fft 16)", "several chunks per group", "a ragged last chunk", "several runs per signal",
                  "one block (one join launch)", "several signals", "no padding, no detrending", "four chains")),
    dict(id="n32-l20-detrend-1x16", setup=3, n_fft=32, L=20, hop=8, mode=None, detrend=True, B=1, F=16,
         classes=("schedule 4x4 (n_fft 32)", "exactly one chunk", "a whole last chunk", "one signal", "detrend", "L below n_fft")),
    dict(id="n64-3x17", setup=2, n_fft=64, L=64, hop=8, mode=None, detrend=False, B=3, F=17,
         classes=("schedule 4x4x2 (n_fft 64)", "pair-group = chunk")),
    dict(id="n128-l100-detrend-2x33", setup=0, n_fft=128, L=100, hop=32, mode=None, detrend=True, B=2, F=33,
         classes=("schedule 4x4x4 (n_fft 128)", "first carried regime (two groups per run)", "1 accumulator per lane and chain",
                  "direct form 2")),
    dict(id="n256-l200-detrend-2x40", setup=FORM1, n_fft=256, L=200, hop=64, mode=None, detrend=True, B=2, F=40,
         classes=("schedule 4x4x4x2 (n_fft 256)", "carried regime", "direct form 1")),
    dict(id="n512-l400-3x259", setup=0, n_fft=512, L=400, hop=160, mode=None, detrend=False, B=3, F=259,
         classes=("schedule 4x4x4x4 (n_fft 512)", "2 accumulators per lane and chain (K = 257 on 256 lanes)",
                  "several blocks (two join launches)", "two blocks, the second of 3 frames", "a ragged last block")),
    dict(id="n1024-1x21-padded", setup=4, n_fft=1024, L=1024, hop=256, mode=None, detrend=False, B=1, F=21, padded=True,
         classes=("schedule 4x4x4x4x2 (n_fft 1024)", "one frame pair per group (sixteen groups per run)",
                  "3 accumulators per lane and chain", "a padded output stride")),
    dict(id="n2048-2x18", setup=4, n_fft=2048, L=2048, hop=512, mode=None, detrend=False, B=2, F=18,
         classes=("schedule 4x4x4x4x4 (n_fft 2048)", "two butterflies per lane", "5 accumulators per lane and chain (the most)",
                  "one frame pair per group (sixteen groups per run)")),
    dict(id="n64-2x600", setup=2, n_fft=64, L=64, hop=16, mode=None, detrend=False, B=2, F=600,
         classes=("three blocks", "a ragged last block")),
    dict(id="n16-1x131142", setup=N16, n_fft=16, L=16, hop=2, mode=None, detrend=False, B=1, F=131142,
         classes=("more runs than workgroups (the run loop)", "513 blocks through the join")),
    dict(id="n128-2x1", setup=0, n_fft=128, L=128, hop=64, mode=None, detrend=False, B=2, F=1,
         classes=("F below a chunk", "F = 1")),
    dict(id="n512-detrend-2x15", setup=4, n_fft=512, L=512, hop=100, mode=None, detrend=True, B=2, F=15,
         classes=("F below a chunk", "F = 15")),
    dict(id="n256-l200-reflect", setup=2, n_fft=256, L=200, hop=64, mode="reflect", detrend=False, B=2, T=3000,
         classes=("a centred, reflect-padded descriptor",)),
    dict(id="n256-bcast-3x20", setup=0, n_fft=256, L=256, hop=100, mode=None, detrend=True, B=3, F=20, bcast=True,
         classes=("broadcast x", "carried regime")),
]


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
