"""The case table of the plan-coverage tests: for every front around the window generator (periodogram, cross spectra, STFT frames,
Welch segments, the int32 / any-length / float32 frames kernels, the overlap-add kernels and the ISTFT), the call shapes that between
them reach every branch the planners of bhw_plan.cpp switch on size, and the plan classes each shape is there for.

A plan class is a predicate on the describe line of the call (B.describe_stft, B.describe_welch, B.describe_csd, B.describe_len,
B.describe_f32, B.describe_frames, B.describe_ola), which names the kernel instance, G or Q, the grid and the lanes along the row.
What the line does not print is derived from what it prints: fy = 256 / kx, (step_b, step_f) = divmod(fy, frames), the last frame
block's length from the frames, the row blocks of an overlap-add from count, hop, fy and Q.  A forced plan shape
(bhw_dbg_overlap_add_shape) does not show in a describe line: those classes take (Q, rx) from the case.

tests/test_plan_coverage.py (no GPU) proves that every class has a case and that every case is of the classes it claims;
tests/test_gpu_plan_coverage.py runs every case against the restatements of the fronts' own test files, bit for bit.

Shapes are the smallest that reach their class: the cost of the GPU test is the NumPy reference on the host.

Classes that cannot be reached:
  - direct form 0 (the 32-bit CORDIC state: k_*_direct<0>): direct_form() gives 2 when dat_width + out_shr <= 34 and n_iter >= 7, else 1
    when the state is wide, else 0.  HLS / CPP have out_shr = 2 and n_iter = dat_width >= 8: always 2.  VHDL has out_shr = precision,
    n_iter = dat_width - 1 >= 7 and a wide state exactly when dat_width + precision > 32, which dat_width + precision > 34 implies:
    2 or 1.  No valid bhw_params reaches 0 (test_plan_coverage.test_direct_form_0_is_unreachable sweeps them all).
"""
import re

from blackman_harris_win_amd import binding as B

BLOCK = B.WELCH_BLOCK
MEAN_STRIDE_ROWS = 4 * (1 << 20)          # rows one pass of k_welch_mean takes: kWelchMeanBlock / 64 rows x kWelchMeanMaxGrid workgroups
MAX_GRID_Y = 65535                        # kFramesMaxGridY, kOlaMaxGridY
Q_MAX, Q_MAX_NORM = 16, 8                 # kOlaQMax, kOlaQMaxNorm

# (win, phi_width, dat_width, keywords): the five setups of test_gpu_stft.SETUPS, then a VHDL configuration of direct form 1
SETUPS = [(B.WIN_BH7, 12, 32, {}), (B.WIN_HANN, 10, 16, {}), (B.WIN_BH4, 14, 24, {"model": B.MODEL_VHDL, "combine": B.COMBINE_VHDL}),
          (B.WIN_HAMMING, 9, 24, {"model": B.MODEL_CPP}), (B.WIN_BH5, 16, 32, {}),
          (B.WIN_BH4, 12, 32, {"model": B.MODEL_VHDL, "combine": B.COMBINE_VHDL, "precision": 3}),
          (B.WIN_HANN, 4, 8, {}), (B.WIN_BH4, 6, 32, {"model": B.MODEL_VHDL, "precision": 3})]
FORM1, N16, N64_FORM1 = 5, 6, 7           # indices of the setups the frames / overlap-add cases name


def params(i):
    win, P, W, kw = SETUPS[i]
    return B.make_params(win, P, W, **kw)


# ---- reading a describe line -------------------------------------------------------------------------------------------------------

_FIELDS = {
    "G": r"G = (\d+) ", "Q": r"Q = (\d+) hops", "jmax": r"up to (\d+) frames per output", "kx": r"\((\d+) along (?:k|the row)\)",
    "rx": r"\((\d+) along r,", "qy": r", (\d+) along q\)", "signals": r"(\d+) signals", "frames": r" x (\d+) frames", "rows": r"= (\d+) rows",
    "bins": r" x (\d+) bins", "blocks": r"(\d+) blocks? of", "pass": r"waves of (\d+) frames a pass", "channels": r"(\d+) channels?,",
    "n_fft": r"n_fft (\d+)", "chains": r"(\d+) chains", "mean_grid": r"one wave per row, grid (\d+) x",
}


def parse(line):
    """The numbers of a describe line, by name; kernel: the first k_*<...> instance as (name, template arguments); grid: the
    workgroup counts of the (last) 'grid a x b x 256 lanes' or 'grid a x 256 lanes'."""
    d = {"line": line}
    for name, pat in _FIELDS.items():
        m = re.search(pat, line)
        if m:
            d[name] = int(m.group(1))
    kernels = re.findall(r"(k_\w+)<([\w,]+)>", line)
    d["kernels"] = {k: tuple(a.split(",")) for k, a in kernels}
    m = re.findall(r"grid (\d+) x (\d+) x 256 lanes", line)
    if m:
        d["grid_x"], d["grid_y"] = int(m[-1][0]), int(m[-1][1])
    if "kx" in d:
        d["fy"] = 256 // d["kx"]
    d["table"] = any("_table" in k for k in d["kernels"])
    return d


def _kernel(d, *names):
    for n in names:
        if n in d["kernels"]:
            return d["kernels"][n]
    return None


# ---- periodogram ---------------------------------------------------------------------------------------------------------------------

def _nfft(K):
    return 2 * (K - 1) if K > 1 else 1


def psd_line(c, table=None):
    return B.describe_welch(psd=B.make_psd(c["B"], c["F"], c["K"], _nfft(c["K"]), 1.0, onesided=True))


def _psd_inst(partial, unroll):
    return lambda c, d: _kernel(d, "k_welch_psd") == (str(partial), str(unroll))


def _last_block(d):
    return d["frames"] - (d["blocks"] - 1) * BLOCK


def _psd_tail(unroll, lo, hi):
    """The last block ends r = length mod 64 frames into a pass of 64: the ragged sum of wave 0 (a pass of 32 at unroll 8 ends inside the
    first half, on it, or inside the second half)."""
    return lambda c, d: d["pass"] == unroll and lo <= _last_block(d) % 64 <= hi


PSD_CLASSES = {
    "k_welch_psd<0,16>": _psd_inst(0, 16), "k_welch_psd<1,16>": _psd_inst(1, 16),
    "k_welch_psd<0,8>": _psd_inst(0, 8), "k_welch_psd<1,8>": _psd_inst(1, 8),
    "unroll 16, last block 0 < r < 32": _psd_tail(16, 1, 31), "unroll 16, last block r = 32": _psd_tail(16, 32, 32),
    "unroll 16, last block 32 < r < 64": _psd_tail(16, 33, 63),
    "unroll 8, last block 0 < r < 32": _psd_tail(8, 1, 31), "unroll 8, last block r = 32": _psd_tail(8, 32, 32),
    "unroll 8, last block 32 < r < 64": _psd_tail(8, 33, 63),
    "a whole last block": lambda c, d: _last_block(d) == BLOCK,
    "join, one trip": lambda c, d: 2 <= d["blocks"] <= 16,
    "join, two trips, the last ragged": lambda c, d: d["blocks"] in (17, 18),
    "join<1,8>, two trips": lambda c, d: d["blocks"] in (17, 18) and _kernel(d, "k_welch_psd") == ("1", "8"),
    "the benchmarked spectrum (64, 998, 257)": lambda c, d: (d["signals"], d["frames"], d["bins"]) == (64, 998, 257),
    "strided rows and output": lambda c, d: bool(c.get("strided")),
}
PSD_CASES = [
    dict(id="b2-f71-k33", B=2, F=71, K=33, classes=("k_welch_psd<0,16>", "unroll 16, last block 0 < r < 32")),
    dict(id="b2-f96-k65", B=2, F=96, K=65, strided=True, classes=("unroll 16, last block r = 32", "strided rows and output")),
    dict(id="b3-f110-k1", B=3, F=110, K=1, classes=("unroll 16, last block 32 < r < 64",)),
    dict(id="b2-f552-k129", B=2, F=552, K=129, classes=("k_welch_psd<1,16>", "join, one trip")),
    dict(id="b2-f4116-k65", B=2, F=16 * BLOCK + 20, K=65, strided=True, classes=("join, two trips, the last ragged",)),
    dict(id="b1-f4608-k33", B=1, F=18 * BLOCK, K=33, classes=("a whole last block",)),
    dict(id="b1030-f71-k1", B=1030, F=71, K=1, classes=("k_welch_psd<0,8>", "unroll 8, last block 0 < r < 32")),
    dict(id="b1030-f96-k3", B=1030, F=96, K=3, strided=True, classes=("unroll 8, last block r = 32",)),
    dict(id="b515-f110-k65", B=515, F=110, K=65, classes=("unroll 8, last block 32 < r < 64",)),
    dict(id="b180-f1312-k1", B=180, F=5 * BLOCK + 32, K=1, classes=("k_welch_psd<1,8>",)),
    dict(id="b70-f4103-k1", B=70, F=16 * BLOCK + 7, K=1, strided=True, classes=("join<1,8>, two trips",)),
    dict(id="bench-64-998-257", B=64, F=998, K=257, classes=("the benchmarked spectrum (64, 998, 257)",)),
]

# ---- cross spectra -------------------------------------------------------------------------------------------------------------------

ALL = ("pxy", "pxx", "pyy", "coherence", "h1")


def csd_line(c, table=None):
    return B.describe_csd(B.make_csd(c["B"], c["F"], c["K"], _nfft(c["K"]), 1.0, outputs=c["outputs"], onesided=True,
                                     broadcast_x=bool(c.get("broadcast"))))


def _csd_inst(chains, partial):
    return lambda c, d: _kernel(d, "k_welch_csd") == (str(chains), str(partial))


def _csd_join(chains, blocks):
    return lambda c, d: _kernel(d, "k_welch_csd_join") == (str(chains),) and d["blocks"] == blocks


CSD_CLASSES = {
    "k_welch_csd<2,0>": _csd_inst(2, 0), "k_welch_csd<2,1>": _csd_inst(2, 1), "k_welch_csd<4,0>": _csd_inst(4, 0),
    "k_welch_csd<4,1>": _csd_inst(4, 1),
    "join<2>, 5 blocks (second trip, ragged)": _csd_join(2, 5), "join<4>, 5 blocks (second trip, ragged)": _csd_join(4, 5),
    "join<2>, 9 blocks (third trip, ragged)": _csd_join(2, 9), "join<4>, 9 blocks (third trip, ragged)": _csd_join(4, 9),
    "X broadcast at 5 blocks or more": lambda c, d: "X broadcast" in d["line"] and d["blocks"] >= 5,
    "a single real output of the four-chain form": lambda c, d: d["chains"] == 4 and len(c["outputs"]) == 1,
}
CSD_CASES = [
    dict(id="pxy-b2-f100-k33", B=2, F=100, K=33, outputs=("pxy",), classes=("k_welch_csd<2,0>",)),
    dict(id="all-b2-f77-k65", B=2, F=77, K=65, outputs=ALL, classes=("k_welch_csd<4,0>",)),
    dict(id="pxy-b2-f1044-k65", B=2, F=4 * BLOCK + 20, K=65, outputs=("pxy",),
         classes=("k_welch_csd<2,1>", "join<2>, 5 blocks (second trip, ragged)")),
    dict(id="all-b2-f1044-k33", B=2, F=4 * BLOCK + 20, K=33, outputs=ALL,
         classes=("k_welch_csd<4,1>", "join<4>, 5 blocks (second trip, ragged)")),
    dict(id="pxy-b1-f2057-k17", B=1, F=8 * BLOCK + 9, K=17, outputs=("pxy",), classes=("join<2>, 9 blocks (third trip, ragged)",)),
    dict(id="all-b1-f2057-k33", B=1, F=8 * BLOCK + 9, K=33, outputs=ALL, classes=("join<4>, 9 blocks (third trip, ragged)",)),
    dict(id="all-bcast-b3-f1281-k33", B=3, F=5 * BLOCK + 1, K=33, outputs=ALL, broadcast=True, classes=("X broadcast at 5 blocks or more",)),
    dict(id="coh-b2-f1300-k9", B=2, F=5 * BLOCK + 20, K=9, outputs=("coherence",), classes=("a single real output of the four-chain form",)),
]

# ---- STFT frames and Welch segments: one plan (bhwp_stft_plan) -----------------------------------------------------------------------

def stft_desc(c):
    """The bhw_stft of a frames case: (descriptor, L, frames, col0, pad).  odd: x_stride and y_batch_stride odd, so two channels move as
    4-byte halves; padded: gaps behind every row and every signal of y (sentinels in the GPU test) and behind every signal of x."""
    n_fft, L, hop, C, nb, T = c["n_fft"], c["L"], c["hop"], c["C"], c["B"], c["T"]
    pad = n_fft // 2 if c["center"] else 0
    frames = 1 + (T + 2 * pad - n_fft) // hop
    col0 = (n_fft - L) // 2
    xs, ys, ybs = T * C, n_fft * C, frames * n_fft * C
    if c.get("padded"):
        xs, ys = xs + 4, ys + 6
        ybs = frames * ys + 10
    if c.get("odd"):
        xs, ybs = xs + 1, ybs + 1
    s = B.make_stft(nb, T, frames, hop, n_fft, col0=col0, pad=pad, pad_mode=B.PAD_REFLECT if c["mode"] == "reflect" else B.PAD_CONSTANT,
                    channels=C, shift=SETUPS[c["setup"]][2] - 1, x_stride=xs, y_stride=ys, y_batch_stride=ybs)
    return s, L, frames, col0, pad


def stft_line(c, table=None):
    s, L = stft_desc(c)[:2]
    return B.describe_stft(params(c["setup"]), L, s, table=table)


def welch_desc(c):
    """The bhw_stft of a Welch segments case (pad 0, col0 0, F = 1 + (T - L) / hop) and L, F; padded / odd as stft_desc."""
    nfft, L, hop, C, nb, T = c["n_fft"], c["L"], c["hop"], c["C"], c["B"], c["T"]
    F = 1 + (T - L) // hop
    xs, ys, ybs = T * C, nfft * C, F * nfft * C
    if c.get("padded"):
        xs, ys = xs + 4, ys + 6
        ybs = F * ys + 10
    if c.get("odd"):
        xs, ybs = xs + 1, ybs + 1
    s = B.make_stft(nb, T, F, hop, nfft, channels=C, shift=SETUPS[c["setup"]][2] - 1, x_stride=xs, y_stride=ys, y_batch_stride=ybs)
    return s, L, F


def welch_line(c, table=None):
    s, L, _ = welch_desc(c)
    return B.describe_welch(params(c["setup"]), L, stft=s, detrend=True, table=table)


def _steps(d):
    return divmod(d["fy"], d["frames"])                                # (step_b, step_f): fy = step_b * frames + step_f


def _rows_plan(G_many, fy_many):
    return lambda c, d: (d["G"] > 1) == G_many and (d["fy"] > 1) == fy_many


def _step_class(b_nonzero, f_nonzero):
    return lambda c, d: d["G"] > 1 and (_steps(d)[0] != 0) == b_nonzero and (_steps(d)[1] != 0) == f_nonzero


_ROWS_CLASSES = {
    "G = 1, fy = 1": _rows_plan(False, False), "G = 1, fy > 1": _rows_plan(False, True),
    "G > 1, fy = 1": _rows_plan(True, False), "G > 1, fy > 1": _rows_plan(True, True),
    "G > 1, step (0, f)": _step_class(False, True), "G > 1, step (b, 0)": _step_class(True, False), "G > 1, step (b, f)": _step_class(True, True),
    "G > 4 and not a multiple of 4 (a ragged last trip of the four-row loop)": lambda c, d: d["G"] > 4 and d["G"] % 4 != 0,
    "G > 1, kx above n_fft (idle lanes)": lambda c, d: d["G"] > 1 and d["kx"] > d["n_fft"],
    "G > 1, one channel": lambda c, d: d["G"] > 1 and d["channels"] == 1,
    "G > 1, two channels, 8-byte pairs": lambda c, d: d["G"] > 1 and d["channels"] == 2 and not c.get("odd"),
    "G > 1, two channels, 4-byte halves": lambda c, d: d["G"] > 1 and d["channels"] == 2 and bool(c.get("odd")),
    "G > 1, padded strides": lambda c, d: d["G"] > 1 and bool(c.get("padded")),
}
STFT_CLASSES = dict(_ROWS_CLASSES)
STFT_CLASSES.update({
    "G > 1, reflect padding": lambda c, d: d["G"] > 1 and c["center"] and c["mode"] == "reflect",
    "G > 1, constant padding": lambda c, d: d["G"] > 1 and c["center"] and c["mode"] == "constant",
    "G > 1, center=False": lambda c, d: d["G"] > 1 and not c["center"],
    "G > 1, L below n_fft (zero columns)": lambda c, d: d["G"] > 1 and c["L"] < c["n_fft"],
    "the benchmarked batch (64 x 160000, 400 / 512 / 160)": lambda c, d: (d["signals"], d["frames"], d["n_fft"], d["G"]) == (64, 1001, 512, 32),
})
STFT_CASES = [
    dict(id="n512-b2", setup=0, n_fft=512, L=400, hop=160, center=True, mode="reflect", C=1, B=2, T=4000, classes=("G = 1, fy = 1",)),
    dict(id="n64-b3", setup=1, n_fft=64, L=49, hop=13, center=True, mode="constant", C=2, B=3, T=150, classes=("G = 1, fy > 1",)),
    dict(id="n256-hop4-b5", setup=2, n_fft=256, L=256, hop=4, center=False, mode="reflect", C=2, B=5, T=20000, padded=True,
         classes=("G > 1, fy = 1", "G > 1, center=False", "G > 1, two channels, 8-byte pairs", "G > 1, padded strides",
                  "G > 4 and not a multiple of 4 (a ragged last trip of the four-row loop)")),
    dict(id="n64-hop4-b14", setup=3, n_fft=64, L=49, hop=4, center=True, mode="reflect", C=2, B=14, T=20000, odd=True,
         classes=("G > 1, fy > 1", "G > 1, step (0, f)", "G > 1, two channels, 4-byte halves", "G > 1, reflect padding",
                  "G > 1, L below n_fft (zero columns)")),
    dict(id="n32-f4-b40000", setup=0, n_fft=32, L=32, hop=16, center=True, mode="reflect", C=1, B=40000, T=50,
         classes=("G > 1, step (b, 0)", "G > 1, one channel")),
    dict(id="n32-f3-b50000", setup=4, n_fft=32, L=30, hop=16, center=True, mode="constant", C=1, B=50000, T=40,
         classes=("G > 1, step (b, f)", "G > 1, constant padding")),
    dict(id="n100-hop7-b300", setup=1, n_fft=100, L=77, hop=7, center=True, mode="reflect", C=1, B=300, T=2000,
         classes=("G > 1, kx above n_fft (idle lanes)",)),
    dict(id="bench-64x160000", setup=0, n_fft=512, L=400, hop=160, center=True, mode="reflect", C=1, B=64, T=160000,
         classes=("the benchmarked batch (64 x 160000, 400 / 512 / 160)",)),
]

WELCH_CLASSES = dict(_ROWS_CLASSES)
WELCH_CLASSES.update({
    "mean pass inside its stride loop, one channel": lambda c, d: d["rows"] > MEAN_STRIDE_ROWS and d["channels"] == 1,
    "mean pass k_welch_mean<2> at G > 1": lambda c, d: d["G"] > 1 and d["channels"] == 2 and not c.get("odd"),
    "mean pass k_welch_mean<1> at G > 1": lambda c, d: d["G"] > 1 and d["channels"] == 2 and bool(c.get("odd")),
    "G > 1, L below n_fft (zero columns)": lambda c, d: d["G"] > 1 and c["L"] < c["n_fft"],
})
WELCH_CASES = [
    dict(id="l400-b2", setup=0, n_fft=512, L=400, hop=160, C=1, B=2, T=4000, classes=("G = 1, fy = 1",)),
    dict(id="l13-b3", setup=1, n_fft=16, L=13, hop=5, C=2, B=3, T=100, classes=("G = 1, fy > 1",)),
    dict(id="l200-hop8-b10", setup=2, n_fft=256, L=200, hop=8, C=2, B=10, T=20000, padded=True,
         classes=("G > 1, fy = 1", "G > 1, two channels, 8-byte pairs", "G > 1, padded strides", "mean pass k_welch_mean<2> at G > 1",
                  "G > 4 and not a multiple of 4 (a ragged last trip of the four-row loop)")),
    dict(id="l50-hop4-b14", setup=3, n_fft=64, L=50, hop=4, C=2, B=14, T=20000, odd=True,
         classes=("G > 1, fy > 1", "G > 1, step (0, f)", "G > 1, two channels, 4-byte halves", "mean pass k_welch_mean<1> at G > 1",
                  "G > 1, L below n_fft (zero columns)")),
    dict(id="l30-f4-b40000", setup=0, n_fft=32, L=30, hop=16, C=1, B=40000, T=80, classes=("G > 1, step (b, 0)", "G > 1, one channel")),
    dict(id="l30-f3-b50000", setup=4, n_fft=32, L=30, hop=16, C=1, B=50000, T=70, classes=("G > 1, step (b, f)",)),
    dict(id="l77-hop7-b300", setup=1, n_fft=100, L=77, hop=7, C=1, B=300, T=2000, classes=("G > 1, kx above n_fft (idle lanes)",)),
    # 4 194 498 rows of one signal: 17 MB of x, 67 MB of y; the reference runs in chunks of rows
    dict(id="l3-rows-4194498", setup=0, n_fft=4, L=3, hop=1, C=1, B=1, T=MEAN_STRIDE_ROWS + 196,
         classes=("mean pass inside its stride loop, one channel",)),
]

# ---- frames kernels: int32 power of two, int32 any length, float32 ---------------------------------------------------------------------

def frames_desc(c):
    return B.make_frames(c["frames"], c["hop"], channels=c["C"], shift=SETUPS[c["setup"]][2] - 1,
                         y_stride=c["L"] * c["C"] + 6 if c.get("padded") else 0)


def frames_line(c, table=None):
    p, f = params(c["setup"]), frames_desc(c)
    if c["kind"] == "pow2":
        assert c["L"] == 1 << p.phi_width
        return B.describe_frames(p, c["frames"], c["hop"], channels=c["C"], y_stride=f.y_stride, table=table)
    if c["kind"] == "len":
        return B.describe_len(p, c["L"], frames=f, table=table)
    return B.describe_f32(p, c["L"], frames=f, table=table)


FRAMES_KERNELS = {"pow2": ("k_frames_direct", "k_frames_table"), "len": ("k_frames_direct_len", "k_frames_table_len"),
                  "f32": ("k_frames_f32_direct_len", "k_frames_f32_table_len")}


def _frames_class(kind, pred):
    return lambda c, d: c["kind"] == kind and _kernel(d, *FRAMES_KERNELS[kind]) is not None and pred(c, d)


def _idle(c, d):
    return d["kx"] < 256 and c["L"] < d["kx"]


FRAMES_CLASSES = {}
for _kind in ("len", "f32"):
    for _kx in (1, 4, 128, 256):
        FRAMES_CLASSES[f"{_kind}: kx = {_kx}"] = _frames_class(_kind, lambda c, d, kx=_kx: d["kx"] == kx)
    FRAMES_CLASSES[f"{_kind}: idle lanes below 256 columns"] = _frames_class(_kind, _idle)
    FRAMES_CLASSES[f"{_kind}: idle lanes in the last of several column blocks"] = _frames_class(
        _kind, lambda c, d: d["kx"] == 256 and c["L"] % 256 != 0 and d["grid_x"] > 1)
for _kind in ("pow2", "len", "f32"):
    FRAMES_CLASSES[f"{_kind}: G > 1, fy > 1"] = _frames_class(_kind, lambda c, d: d["G"] > 1 and d["fy"] > 1)
    FRAMES_CLASSES[f"{_kind}: G > 1, fy > 1, two channels"] = _frames_class(_kind, lambda c, d: d["G"] > 1 and d["fy"] > 1 and c["C"] == 2)
    FRAMES_CLASSES[f"{_kind}: G > 1, fy > 1, padded stride"] = _frames_class(_kind, lambda c, d: d["G"] > 1 and d["fy"] > 1 and bool(c.get("padded")))
    FRAMES_CLASSES[f"{_kind}: direct form 1"] = _frames_class(_kind, lambda c, d: _kernel(d, FRAMES_KERNELS[c["kind"]][0]) == ("1",))
    FRAMES_CLASSES[f"{_kind}: direct form 2"] = _frames_class(_kind, lambda c, d: _kernel(d, FRAMES_KERNELS[c["kind"]][0]) == ("2",))
FRAMES_CLASSES["len: G > 4 and not a multiple of 4, fy > 1"] = _frames_class("len", lambda c, d: d["G"] > 4 and d["G"] % 4 and d["fy"] > 1)
FRAMES_CLASSES["f32: G > 4 and not a multiple of 4, fy > 1"] = _frames_class("f32", lambda c, d: d["G"] > 4 and d["G"] % 4 and d["fy"] > 1)


def _frames_cases():
    out = []
    # (L, frames, hop, setup, C, padded): kx 1, 4, 8, 128, 256 and 256 with a ragged second column block
    shapes = [(1, 1200000, 1, 0, 1, False), (3, 600000, 2, 1, 2, False), (5, 200000, 3, 3, 1, True), (100, 40000, 7, FORM1, 2, True),
              (100, 9000, 7, 2, 1, False), (255, 9, 100, 4, 2, False), (400, 12, 160, 0, 1, False)]
    for kind in ("len", "f32"):
        for L, frames, hop, setup, C, padded in shapes:
            cl = []
            kx = 1
            while kx < 256 and kx < L:
                kx *= 2
            if kx in (1, 4, 128, 256) and not (L == 400):
                cl.append(f"{kind}: kx = {kx}")
            if (L, frames) == (3, 600000):
                cl += [f"{kind}: idle lanes below 256 columns", f"{kind}: G > 1, fy > 1, two channels"]
            if (L, frames) == (5, 200000):
                cl += [f"{kind}: G > 1, fy > 1", f"{kind}: G > 1, fy > 1, padded stride"]
            if (L, frames) == (100, 40000):
                cl += [f"{kind}: direct form 1", f"{kind}: G > 4 and not a multiple of 4, fy > 1"]
            if (L, frames) == (100, 9000):
                cl += [f"{kind}: direct form 2"]
            if L == 400:
                cl += [f"{kind}: idle lanes in the last of several column blocks"]
            out.append(dict(id=f"{kind}-l{L}-f{frames}", kind=kind, L=L, frames=frames, hop=hop, setup=setup, C=C, padded=padded,
                            classes=tuple(cl)))
    out.append(dict(id="pow2-n16-f300000", kind="pow2", L=16, frames=300000, hop=3, setup=N16, C=1, padded=True,
                    classes=("pow2: G > 1, fy > 1", "pow2: G > 1, fy > 1, padded stride", "pow2: direct form 2")))
    out.append(dict(id="pow2-n64-f20000", kind="pow2", L=64, frames=20000, hop=5, setup=N64_FORM1, C=2, padded=False,
                    classes=("pow2: G > 1, fy > 1, two channels", "pow2: direct form 1")))
    return out


FRAMES_CASES = _frames_cases()

# ---- overlap-add kernels: int32 power of two, int32 any length, float32, ISTFT ---------------------------------------------------------

def ola_desc(c):
    """The bhw_ola of a one-signal overlap-add case: every output of the extent."""
    count = (c["frames"] - 1) * c["hop"] + c["L"]
    return B.make_ola(c["frames"], c["hop"], count, channels=c["C"], shift=SETUPS[c["setup"]][2] - 1,
                      y_stride=c["L"] * c["C"] + 6 if c.get("padded") else 0)


def istft_desc(c):
    """The bhw_stft of an ISTFT case (center=True, length = the default of torch.istft): (descriptor, L, frames, col0, pad, T)."""
    n_fft, L, hop, C, nb, frames = c["n_fft"], c["L"], c["hop"], c["C"], c["B"], c["frames"]
    pad, col0 = n_fft // 2, (n_fft - L) // 2
    T = n_fft + hop * (frames - 1) - 2 * pad
    return B.make_stft(nb, T, frames, hop, n_fft, col0=col0, pad=pad, channels=C, shift=SETUPS[c["setup"]][2] - 1), L, frames, col0, pad, T


def ola_line(c, table=None):
    p = params(c["setup"])
    if c["kind"] == "istft":
        s, L = istft_desc(c)[:2]
        return B.describe_stft(p, L, s, inverse=True, normalize=bool(c.get("normalize")), table=table)
    o = ola_desc(c)
    if c["kind"] == "pow2":
        assert c["L"] == 1 << p.phi_width
        return B.describe_ola(p, c["frames"], c["hop"], o.count, channels=c["C"], y_stride=o.y_stride, table=table)
    if c["kind"] == "len":
        return B.describe_len(p, c["L"], ola=o, table=table)
    return B.describe_f32(p, c["L"], ola=o, normalize=bool(c.get("normalize")), table=table)


def ola_shape(c, d):
    """(rows, fy, Q, row blocks) of the launch: the forced shape of the case (bhw_dbg_overlap_add_shape), else the line's."""
    count = (c["frames"] - 1) * c["hop"] + c["L"] if c["kind"] != "istft" else istft_desc(c)[5]
    rows = -(-count // c["hop"])
    q, rx = c.get("force", (d["Q"], d["rx"]))
    fy = 256 // rx
    return rows, fy, q, -(-rows // (fy * q))


def _q_max(c):
    return Q_MAX_NORM if c.get("normalize") else Q_MAX


def _ola_class(kind, normalize, pred):
    return lambda c, d: c["kind"] == kind and bool(c.get("normalize")) == normalize and pred(c, d)


def _narrow(c, d):
    return c["L"] < 256 and d["rx"] < 256 and d["qy"] > 1


OLA_CLASSES = {}
for _kind, _norms in (("len", (False,)), ("f32", (False, True)), ("istft", (False, True))):
    for _n in _norms:
        _tag = f"{_kind}{', normalize' if _n else ''}"
        OLA_CLASSES[f"{_tag}: rx < 256 with fy > 1 at L < 256"] = _ola_class(_kind, _n, _narrow)
        OLA_CLASSES[f"{_tag}: Q = 1"] = _ola_class(_kind, _n, lambda c, d: _narrow(c, d) and d["Q"] == 1)
        OLA_CLASSES[f"{_tag}: 1 < Q < q_max"] = _ola_class(_kind, _n, lambda c, d: _narrow(c, d) and 1 < d["Q"] < _q_max(c))
        OLA_CLASSES[f"{_tag}: Q = q_max"] = _ola_class(_kind, _n, lambda c, d: _narrow(c, d) and d["Q"] == _q_max(c))
OLA_CLASSES["len: rx = 1 (hop 1)"] = _ola_class("len", False, lambda c, d: d["rx"] == 1)
OLA_CLASSES["f32: rx = 1 (hop 1)"] = _ola_class("f32", False, lambda c, d: d["rx"] == 1)
OLA_CLASSES["pow2: rx < 256 with fy > 1"] = _ola_class("pow2", False, lambda c, d: "force" not in c and d["rx"] < 256 and d["qy"] > 1)
OLA_CLASSES["pow2: row blocks above 65 535 (forced Q = 1, rx = 256)"] = _ola_class(
    "pow2", False, lambda c, d: c.get("force") == (1, 256) and ola_shape(c, d)[3] > MAX_GRID_Y)
OLA_CLASSES["f32: row blocks above 65 535"] = _ola_class(
    "f32", False, lambda c, d: ola_shape(c, d)[3] > MAX_GRID_Y and d["grid_y"] == MAX_GRID_Y and d["Q"] == Q_MAX)
OLA_CLASSES["f32, normalize: row blocks above 65 535"] = _ola_class(
    "f32", True, lambda c, d: ola_shape(c, d)[3] > MAX_GRID_Y and d["grid_y"] == MAX_GRID_Y and d["Q"] == Q_MAX_NORM)


def _ola_cases():
    out = []
    # (L, frames, hop, setup, C, padded, what): L = 100 at hop = L (Q = 1), hop 25 (Q = 4), hop 5 (Q = q_max); L = 3 at hop 1
    shapes = [(100, 50, 100, 0, 1, False, "Q = 1"), (100, 500, 25, FORM1, 2, True, "1 < Q < q_max"), (100, 500, 5, 2, 1, False, "Q = q_max"),
              (3, 5000, 1, 1, 2, False, "rx = 1 (hop 1)")]
    for kind, norms in (("len", (False,)), ("f32", (False, True))):
        for n in norms:
            tag = f"{kind}{', normalize' if n else ''}"
            for L, frames, hop, setup, C, padded, what in shapes:
                if what.startswith("rx = 1"):
                    cl = (f"{kind}: {what}",) if not n else ()
                else:
                    cl = (f"{tag}: {what}",) + ((f"{tag}: rx < 256 with fy > 1 at L < 256",) if what == "Q = 1" else ())
                out.append(dict(id=f"{kind}{'-norm' if n else ''}-l{L}-hop{hop}", kind=kind, L=L, frames=frames, hop=hop, setup=setup, C=C,
                                padded=padded, normalize=n, classes=cl))
    # ISTFT: the batch shares the workgroup target; n_fft 64, L 49
    for n in (False, True):
        tag = f"istft{', normalize' if n else ''}"
        for frames, hop, nb, C, what in ((40, 64, 3, 1, "Q = 1"), (300, 13, 2, 2, "1 < Q < q_max"), (1100, 3, 3, 1, "Q = q_max")):
            cl = (f"{tag}: {what}",) + ((f"{tag}: rx < 256 with fy > 1 at L < 256",) if what == "Q = 1" else ())
            out.append(dict(id=f"istft{'-norm' if n else ''}-hop{hop}", kind="istft", n_fft=64, L=49, frames=frames, hop=hop, B=nb, C=C,
                            setup=1, normalize=n, classes=cl))
    out.append(dict(id="pow2-n16-hop4", kind="pow2", L=16, frames=10000, hop=4, setup=N16, C=2, padded=True,
                    classes=("pow2: rx < 256 with fy > 1",)))
    # one row block per output: 70 000 row blocks against a grid of 65 535
    out.append(dict(id="pow2-n16-hop1-forced", kind="pow2", L=16, frames=70000 - 15, hop=1, setup=N16, C=1, force=(1, 256),
                    classes=("pow2: row blocks above 65 535 (forced Q = 1, rx = 256)",)))
    # hop = L = 256: fy = 1, Q = q_max, one term per output; 65 535 q_max + 100 frames: 0.5 GiB each of y and x normalised, 1 GiB each not
    for n in (True, False):
        q = Q_MAX_NORM if n else Q_MAX
        out.append(dict(id=f"f32{'-norm' if n else ''}-l256-rowblocks", kind="f32", L=256, frames=MAX_GRID_Y * q + 100, hop=256, setup=0, C=1,
                        normalize=n, device_reference=True,
                        classes=(f"f32{', normalize' if n else ''}: row blocks above 65 535",)))
    return out


OLA_CASES = _ola_cases()

# ---- the fronts ------------------------------------------------------------------------------------------------------------------------

FRONTS = {
    "psd": (PSD_CASES, PSD_CLASSES, psd_line), "csd": (CSD_CASES, CSD_CLASSES, csd_line), "stft": (STFT_CASES, STFT_CLASSES, stft_line),
    "welch": (WELCH_CASES, WELCH_CLASSES, welch_line), "frames": (FRAMES_CASES, FRAMES_CLASSES, frames_line),
    "ola": (OLA_CASES, OLA_CLASSES, ola_line),
}


def case_ids(front):
    return [c["id"] for c in FRONTS[front][0]]


def case(front, cid):
    return next(c for c in FRONTS[front][0] if c["id"] == cid)
