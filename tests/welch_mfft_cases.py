"""The case table of the fused Welch PSD at a mixed-radix n_fft (bhw_welch_mfft_f32_*), in the manner of tests/welch_fft_cases.py: the
call shapes that between them reach every branch the accumulate epilogue's text takes (bhw_welch_mfft.hip) and every class its planner
(bhwp_welch_mfft_plan) can emit, and the classes each shape is there for.  The branches of the row function itself (the radix passes,
the lane and column layouts) are tests/stft_mfft_cases.py's: the row function is that kernel's text.

A class is a predicate on the describe line of the call (B.describe_welch_mfft): bhw_describe_stft_mfft's fields in the same words,
plus the chunk, the runs, the frames and groups of a run, the accumulators a lane carries, the chunks and blocks per signal and the
workspace bytes.  95 values of n_fft are supported, so a shape is not a value of n_fft: it is what the epilogue branches on --
shape() below.

The longest case has 131 142 frames of n_fft 18 at hop 2, so T = 131 141 * 2 + 18 = 262 300 samples (the power-of-two table's
262 298 is that count for n_fft 16).

tests/test_welch_mfft_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds, that a sweep of the
planner over every supported n_fft emits no shape the table lacks, and that the shared fields equal describe_stft_mfft's;
tests/test_gpu_welch_mixed.py runs every case, library and table, word for word against the contract restated on bhw.stft_mixed's
rows.
"""
import re

from blackman_harris_win_amd import binding as B

import plan_cases as PC
import stft_mfft_cases as SM

SETUPS, params, FORM1 = PC.SETUPS, PC.params, PC.FORM1
CHUNK, BLOCK, MAX_GRID = B.WELCH_FFT_CHUNK, B.WELCH_BLOCK, SM.MAX_GRID
LANES = 256                                # kFftBlock

_FIELDS = {
    "chunk": r"chunk (\d+) frames", "runs": r"(\d+) runs of", "run": r"runs of (\d+) frames", "gpr": r"\((\d+) groups? per run\)",
    "acc": r"(\d+) accumulators? per lane", "chunks": r"(\d+) chunks and", "blocks": r"and (\d+) blocks? per signal",
    "workspace": r"workspace (\d+) bytes",
}


def parse(line):
    d = SM.parse(line)
    for name, pat in _FIELDS.items():
        m = re.search(pat, line)
        if m:
            d[name] = int(m.group(1))
    d["joins"] = 2 if "twice" in line else 1
    return d


def shape(d):
    """What the text of the accumulate epilogue branches on: the chunks a group holds (fy >= 16: 4, 2 or 1; the (chunk, bin) pairs
    are at most 64 everywhere, one trip), or the groups of a run (fy < 16: 2, 4, 8 or 16) and whether bin M is taken aside.  The
    count of accumulators is the bound of a predicate, not a branch, and the parity of M is none either (the split expression's
    pairs (k, M - k) are the forward kernel's); the classes still hold the edges of both: 1, 2 and 8 accumulators, M odd in each
    regime."""
    M = d["m"]
    if d["fy"] >= CHUNK:
        assert (d["fy"] // CHUNK) * (M + 1) <= 64, d["line"]
        return ("chunks", d["fy"] // CHUNK)
    return ("carried", d["gpr"], M % LANES == 0)


def frames_to_samples(c):
    """T for exactly c["F"] frames: the Welch extent with detrending ((F - 1) * hop + L), a whole n_fft row otherwise."""
    if "T" in c:
        return c["T"]
    return (c["F"] - 1) * c["hop"] + (c["L"] if c["detrend"] else c["n_fft"])


def desc(c):
    """The bhw_stft of a case as bhw.welch_fft_mixed builds it: (descriptor, L, frames, detrend).  mode None: no padding
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
    s = B.make_stft(nb, T, frames, hop, n_fft, col0=col0, pad=pad, pad_mode=mode, shift=SETUPS[c["setup"]][2] - 1)
    return s, L, frames, bool(c["detrend"])


def line(c, table=None):
    s, L, _, det = desc(c)
    return B.describe_welch_mfft(params(c["setup"]), L, s, detrend=det, table=table)


def workspace_doubles(nb, F, K):
    """The workspace formula of include/bhw.h."""
    chunks, blocks = -(-F // CHUNK), -(-F // BLOCK)
    return nb * K * (chunks + (blocks if blocks > 1 else 0))


CLASSES = {
    "fy 64 (four chunks per group)": lambda c, d: d["fy"] == 4 * CHUNK and d["gpr"] == 1 and d["acc"] == 0,
    "fy 32 (two chunks per group)": lambda c, d: d["fy"] == 2 * CHUNK and d["gpr"] == 1 and d["acc"] == 0,
    "fy equal to the chunk": lambda c, d: d["fy"] == CHUNK and d["gpr"] == 1 and d["acc"] == 0,
    "fy 8 (carried sums, two groups per run)": lambda c, d: d["fy"] == 8 and d["gpr"] == 2 and d["acc"] >= 1,
    "fy 4 (four groups per run)": lambda c, d: d["fy"] == 4 and d["gpr"] == 4,
    "fy 2 (eight groups per run)": lambda c, d: d["fy"] == 2 and d["gpr"] == 8,
    "fy 1 (sixteen groups per run)": lambda c, d: d["fy"] == 1 and d["gpr"] == CHUNK,
    "M odd under the chunk regime": lambda c, d: d["m"] % 2 == 1 and d["fy"] >= CHUNK,
    "M odd under carried sums": lambda c, d: d["m"] % 2 == 1 and d["fy"] < CHUNK,
    "the schedule 5x5 of n_fft 50": lambda c, d: d["n_fft"] == 50 and d["schedule"] == "5x5",
    "the (chunk, bin) loop in one trip": lambda c, d: d["fy"] >= CHUNK and (d["fy"] // CHUNK) * (d["m"] + 1) <= LANES,
    "K = 61 on 256 lanes": lambda c, d: d["m"] + 1 == 61 and d["fy"] == CHUNK,
    "1 accumulator per lane, K = 101 on 256 lanes": lambda c, d: d["acc"] == 1 and d["m"] + 1 == 101,
    "2 accumulators per lane": lambda c, d: d["acc"] == 2,
    "bin M aside (M = 3 x 256)": lambda c, d: d["m"] == 3 * LANES and d["acc"] == 4,
    "8 accumulators per lane": lambda c, d: d["acc"] == 8,
    "several trips per pass": lambda c, d: any(s[2] == "several" for s in SM.pass_shapes(d)),
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
    "2 050 runs above the grid cap (the run loop)": lambda c, d: d["runs"] == 2050 > d["grid"] == MAX_GRID,
    "513 blocks through the join": lambda c, d: d["blocks"] == 513,
    "one signal": lambda c, d: d["signals"] == 1,
    "several signals": lambda c, d: d["signals"] > 1,
    "a padded p_stride": lambda c, d: bool(c.get("padded")),
    "detrend": lambda c, d: d["detrend"],
    "no padding, no detrending": lambda c, d: not d["detrend"] and d["pad"] == 0,
    "L below n_fft": lambda c, d: c["L"] < c["n_fft"],
    "a centred, reflect-padded descriptor": lambda c, d: not d["detrend"] and d["pad"] > 0 and d["reflect"],
    "direct form 1": lambda c, d: d["kernels"].get("k_welch_mfft_direct") == ("1",),
    "direct form 2": lambda c, d: d["kernels"].get("k_welch_mfft_direct") == ("2",),
}

CASES = [
    dict(id="n18-l13-detrend-2x70", setup=1, n_fft=18, L=13, hop=5, mode=None, detrend=True, B=2, F=70,
         classes=("fy 64 (four chunks per group)", "M odd under the chunk regime", "a ragged last chunk", "two runs per signal",
                  "one block (one join launch)", "several signals", "detrend", "L below n_fft", "the (chunk, bin) loop in one trip")),
    dict(id="n40-1x16", setup=3, n_fft=40, L=40, hop=8, mode=None, detrend=False, B=1, F=16,
         classes=("fy 32 (two chunks per group)", "exactly one chunk", "a whole last chunk", "one signal", "no padding, no detrending")),
    dict(id="n50-3x17", setup=2, n_fft=50, L=50, hop=10, mode=None, detrend=False, B=3, F=17,
         classes=("fy 32 (two chunks per group)", "M odd under the chunk regime", "the schedule 5x5 of n_fft 50")),
    dict(id="n96-l80-detrend-2x33", setup=0, n_fft=96, L=80, hop=32, mode=None, detrend=True, B=2, F=33,
         classes=("fy equal to the chunk", "direct form 2")),
    dict(id="n120-reflect", setup=2, n_fft=120, L=120, hop=30, mode="reflect", detrend=False, B=2, T=3000,
         classes=("a centred, reflect-padded descriptor", "K = 61 on 256 lanes")),
    dict(id="n200-l160-detrend-2x40", setup=4, n_fft=200, L=160, hop=64, mode=None, detrend=True, B=2, F=40,
         classes=("fy 8 (carried sums, two groups per run)", "1 accumulator per lane, K = 101 on 256 lanes")),
    dict(id="n400-3x259", setup=0, n_fft=400, L=400, hop=160, mode=None, detrend=False, B=3, F=259,
         classes=("fy 4 (four groups per run)", "several blocks (two join launches)", "two blocks, the second of 3 frames",
                  "a ragged last block")),
    dict(id="n1000-1x21-padded", setup=4, n_fft=1000, L=1000, hop=250, mode=None, detrend=False, B=1, F=21, padded=True,
         classes=("fy 2 (eight groups per run)", "2 accumulators per lane", "a padded p_stride")),
    dict(id="n1536-2x18-form1", setup=FORM1, n_fft=1536, L=1536, hop=512, mode=None, detrend=False, B=2, F=18,
         classes=("fy 1 (sixteen groups per run)", "bin M aside (M = 3 x 256)", "direct form 1")),
    dict(id="n4050-detrend-1x35", setup=0, n_fft=4050, L=4050, hop=1024, mode=None, detrend=True, B=1, F=35,
         classes=("M odd under carried sums", "8 accumulators per lane", "several trips per pass")),
    dict(id="n96-2x600", setup=2, n_fft=96, L=96, hop=24, mode=None, detrend=False, B=2, F=600,
         classes=("three blocks", "a ragged last block")),
    dict(id="n18-1x131142", setup=1, n_fft=18, L=18, hop=2, mode=None, detrend=False, B=1, F=131142,
         classes=("2 050 runs above the grid cap (the run loop)", "513 blocks through the join")),
    dict(id="n400-2x1", setup=0, n_fft=400, L=400, hop=160, mode=None, detrend=False, B=2, F=1,
         classes=("F below a chunk", "F = 1")),
    dict(id="n400-detrend-2x15", setup=4, n_fft=400, L=400, hop=100, mode=None, detrend=True, B=2, F=15,
         classes=("F below a chunk", "F = 15")),
]


def case_ids():
    return [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
