"""The case table of the fused Welch PSD for I/Q input (bhw_welch_cfft_f32_*), in the manner of tests/welch_fft_cases.py: the call
shapes that between them reach every branch the kernel's text takes (bhw_welch_cfft.hip) and every class its planner
(bhwp_welch_cfft_plan) can emit, and the classes each shape is there for.

A class is a predicate on the describe line of the call (B.describe_welch_cfft): bhw_describe_stft_cfft's fields in the same words
(without the output form), plus the chunk, the runs, the frames and groups of a run, the accumulators a lane carries, the chunks and
blocks per signal and the workspace bytes.  The complex layout is lpf = min(256, max(4, n / 4)) lanes on a row and fy = 256 / lpf
rows side by side: fy 64, 32, 16 for n_fft 16, 32, 64 (whole chunks per group, nothing carried) and 8, 4, 2, 1, 1 from 128 on
(carried sums, ceil(n_fft / 256) accumulators).

tests/test_welch_cfft_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds, that a sweep of the
planner over every supported n_fft emits no shape the table lacks, and that the shared fields equal describe_stft_cfft's;
tests/test_gpu_welch_cfft.py runs every case, library and table, shifted and not, word for word against the contract restated on
bhw.stft_iq's rows.
"""
import re

from blackman_harris_win_amd import binding as B

import plan_cases as PC
import stft_cfft_cases as SC

SETUPS, params, FORM1, N16 = PC.SETUPS, PC.params, PC.FORM1, PC.N16
CHUNK, BLOCK, MAX_GRID = B.WELCH_FFT_CHUNK, B.WELCH_BLOCK, SC.MAX_GRID

_FIELDS = {
    "chunk": r"chunk (\d+) frames", "runs": r"(\d+) runs of", "run": r"runs of (\d+) frames", "gpr": r"\((\d+) groups? per run\)",
    "acc": r"(\d+) accumulators? per lane", "chunks": r"(\d+) chunks and", "blocks": r"and (\d+) blocks? per signal",
    "workspace": r"workspace (\d+) bytes",
}


def parse(line):
    d = SC.parse(line)
    for name, pat in _FIELDS.items():
        m = re.search(pat, line)
        if m:
            d[name] = int(m.group(1))
    d["joins"] = 2 if "twice" in line else 1
    return d


def frames_to_samples(c):
    """T for exactly c["F"] frames: the Welch extent with detrending ((F - 1) * hop + L), a whole n_fft row otherwise."""
    if "T" in c:
        return c["T"]
    return (c["F"] - 1) * c["hop"] + (c["L"] if c["detrend"] else c["n_fft"])


def desc(c):
    """The bhw_stft of a case as bhw.welch_fft_iq builds it (channels 2): (descriptor, L, frames, detrend).  mode None: no padding
    (center=False); detrend: the Welch segments (col0 0, F = 1 + (T - L) / hop); the y strides are 0."""
    n_fft, L, hop, nb, T = c["n_fft"], c["L"], c["hop"], c["B"], frames_to_samples(c)
    if c["detrend"]:
        pad, col0, mode = 0, 0, B.PAD_CONSTANT
        frames = 1 + (T - L) // hop
    else:
        pad = n_fft // 2 if c["mode"] else 0
        col0 = (n_fft - L) // 2
        mode = B.PAD_REFLECT if c["mode"] == "reflect" else B.PAD_CONSTANT
        frames = 1 + (T + 2 * pad - n_fft) // hop
    s = B.make_stft(nb, T, frames, hop, n_fft, col0=col0, pad=pad, pad_mode=mode, channels=2, shift=SETUPS[c["setup"]][2] - 1)
    return s, L, frames, bool(c["detrend"])


def line(c, table=None, fftshift=False):
    s, L, _, det = desc(c)
    return B.describe_welch_cfft(params(c["setup"]), L, s, detrend=det, fftshift=fftshift, table=table)


def workspace_doubles(nb, F, n_fft):
    """The workspace formula of include/bhw.h."""
    chunks, blocks = -(-F // CHUNK), -(-F // BLOCK)
    return nb * n_fft * (chunks + (blocks if blocks > 1 else 0))


CLASSES = {f"schedule {s} (n_fft {n})": (lambda c, d, n=n, s=s: d["n_fft"] == n and d["schedule"] == s) for n, s in SC.SCHEDULES.items()}
CLASSES.update({
    "fy 64, four chunks per group": lambda c, d: d["fy"] == 4 * CHUNK and d["gpr"] == 1 and d["acc"] == 0,
    "fy 32, two chunks per group": lambda c, d: d["fy"] == 2 * CHUNK and d["gpr"] == 1 and d["acc"] == 0,
    "fy equal to the chunk": lambda c, d: d["fy"] == CHUNK and d["gpr"] == 1 and d["acc"] == 0,
    "fy below the chunk (carried accumulators)": lambda c, d: 1 < d["fy"] < CHUNK and d["gpr"] == CHUNK // d["fy"] and d["acc"] >= 1,
    "fy 8, 128 bins on 256 lanes": lambda c, d: d["fy"] == 8 and d["n_fft"] == 128 and d["acc"] == 1,
    "fy 1 (sixteen groups per run)": lambda c, d: d["fy"] == 1 and d["gpr"] == CHUNK,
    "1 accumulator per lane": lambda c, d: d["acc"] == 1,
    "2 accumulators per lane": lambda c, d: d["acc"] == 2 and d["n_fft"] == 512,
    "4 accumulators per lane": lambda c, d: d["acc"] == 4 and d["n_fft"] == 1024,
    "8 accumulators per lane": lambda c, d: d["acc"] == 8,
    "two butterflies per lane": lambda c, d: d["n_fft"] == 2048 and d["lpf"] == 256,
    "a ragged last chunk": lambda c, d: d["frames"] % CHUNK != 0 and d["frames"] > CHUNK,
    "a whole last chunk": lambda c, d: d["frames"] % CHUNK == 0,
    "exactly one chunk": lambda c, d: d["frames"] == CHUNK and d["chunks"] == 1,
    "F below a chunk": lambda c, d: d["frames"] < CHUNK and d["chunks"] == 1,
    "F = 1": lambda c, d: d["frames"] == 1,
    "F = 15": lambda c, d: d["frames"] == 15,
    "two runs per signal": lambda c, d: d["runs"] == 2 * d["signals"],
    "one block (one join launch)": lambda c, d: d["blocks"] == 1 and d["joins"] == 1,
    "several blocks (two join launches)": lambda c, d: d["blocks"] > 1 and d["joins"] == 2,
    "a ragged last block": lambda c, d: d["blocks"] > 1 and d["frames"] % BLOCK != 0,
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
    "direct form 1": lambda c, d: d["kernels"].get("k_welch_cfft_direct") == ("1",),
    "direct form 2": lambda c, d: d["kernels"].get("k_welch_cfft_direct") == ("2",),
})

CASES = [
    dict(id="n16-2x70", setup=1, n_fft=16, L=16, hop=4, mode=None, detrend=False, B=2, F=70,
         classes=("schedule 4x4 (n_fft 16)", "fy 64, four chunks per group", "a ragged last chunk", "two runs per signal",
                  "one block (one join launch)", "several signals", "no padding, no detrending")),
    dict(id="n32-l20-detrend-1x16", setup=3, n_fft=32, L=20, hop=8, mode=None, detrend=True, B=1, F=16,
         classes=("schedule 4x4x2 (n_fft 32)", "fy 32, two chunks per group", "exactly one chunk", "a whole last chunk", "one signal",
                  "detrend", "L below n_fft")),
    dict(id="n64-3x17", setup=2, n_fft=64, L=64, hop=8, mode=None, detrend=False, B=3, F=17,
         classes=("schedule 4x4x4 (n_fft 64)", "fy equal to the chunk")),
    dict(id="n128-l100-detrend-2x33", setup=0, n_fft=128, L=100, hop=32, mode=None, detrend=True, B=2, F=33,
         classes=("schedule 4x4x4x2 (n_fft 128)", "fy below the chunk (carried accumulators)", "fy 8, 128 bins on 256 lanes",
                  "direct form 2")),
    dict(id="n256-l200-detrend-2x40", setup=FORM1, n_fft=256, L=200, hop=64, mode=None, detrend=True, B=2, F=40,
         classes=("schedule 4x4x4x4 (n_fft 256)", "1 accumulator per lane", "direct form 1")),
    dict(id="n512-l400-3x259", setup=0, n_fft=512, L=400, hop=160, mode=None, detrend=False, B=3, F=259,
         classes=("schedule 4x4x4x4x2 (n_fft 512)", "2 accumulators per lane", "several blocks (two join launches)",
                  "two blocks, the second of 3 frames", "a ragged last block")),
    dict(id="n1024-1x21-padded", setup=4, n_fft=1024, L=1024, hop=256, mode=None, detrend=False, B=1, F=21, padded=True,
         classes=("schedule 4x4x4x4x4 (n_fft 1024)", "fy 1 (sixteen groups per run)", "4 accumulators per lane", "a padded p_stride")),
    dict(id="n2048-detrend-1x35", setup=0, n_fft=2048, L=2048, hop=512, mode=None, detrend=True, B=1, F=35,
         classes=("schedule 4x4x4x4x4x2 (n_fft 2048)", "8 accumulators per lane", "two butterflies per lane")),
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
]

# BHW_CFFT_SHIFT: one case of each regime and 2048 (the GPU test runs every case shifted as well; these are the ones the table names)
SHIFTED = ("n16-2x70", "n256-l200-detrend-2x40", "n2048-detrend-1x35")


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
