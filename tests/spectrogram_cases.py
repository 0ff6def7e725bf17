"""The case table of the fused spectrogram (bhw_spectrogram_f32_*), in the manner of tests/stft_fft_cases.py.

Power mode: every case of stft_fft_cases.CASES, imported and not edited -- the kernel is the forward kernel with another epilogue, so
the plan classes are the forward's and its table reaches them.  Bank mode: the cases below, which between them reach every class of
the filter-bank epilogue (how the filters fall on the lanes of a row, what a band may look like, the workgroup shapes, the strides).

A class is a predicate on the case, on the describe line of its call (B.describe_spectrogram), and on the case's dense bank.
tests/test_spectrogram_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds and that the describe
line's plan fields are those of describe_stft_fft for the same call; tests/test_gpu_spectrogram.py runs every case, library and table,
bit for bit against values computed from bhw.stft.
"""
import re

import numpy as np

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from blackman_harris_win_amd.selector import fbank_bands

import stft_fft_cases as FC

SETUPS, params = FC.SETUPS, FC.params
PLAN_FIELDS = ("signals", "frames", "rows", "n_fft", "m", "lpf", "fy", "cpl", "groups", "grid", "lds", "L", "col0", "pad", "schedule",
               "detrend", "reflect", "table")


def parse(line):
    """FC.parse plus the spectrogram's own fields: mode ('power' or 'bank'), W, and for a bank filters, weights, fpl."""
    d = FC.parse(line)
    m = re.search(r"(power|bank) mode, W = (\d+)", line)
    d["mode"], d["W"] = (m.group(1), int(m.group(2))) if m else (None, None)
    m = re.search(r"\((\d+) filters, (\d+) weights, (\d+) filters per lane\)", line)
    if m:
        d["filters"], d["weights"], d["fpl"] = (int(g) for g in m.groups())
    return d


def random_bank(K, filters, seed):
    """A dense (K, filters) float32 bank with the shapes a band may take: filter 0 over all K bins, filter 1 bin 0 alone, filter 2 bin
    M alone, filter 3 empty, filter 4 two weights around interior zeros, the rest random bands; about a third of the weights negative."""
    rng = np.random.default_rng(seed)
    w = np.zeros((K, filters), dtype=np.float32)
    for m in range(filters):
        k0 = int(rng.integers(0, K))
        c = int(rng.integers(1, K - k0 + 1))
        w[k0:k0 + c, m] = (rng.random(c) - 0.33).astype(np.float32) + np.float32(1e-3)
    w[:, 0] = (rng.random(K) + 0.5).astype(np.float32)
    if filters > 1:
        w[:, 1] = 0
        w[0, 1] = 0.75
    if filters > 2:
        w[:, 2] = 0
        w[K - 1, 2] = -1.5
    if filters > 3:
        w[:, 3] = 0
    if filters > 4:
        w[:, 4] = 0
        w[1, 4], w[K - 2, 4] = 2.0, 0.5
    return w


_BANKS = {}


def bank(c):
    """The dense (K, filters) float32 array of a bank case (cached), or None for a power case."""
    spec = c.get("bank")
    if spec is None:
        return None
    key = (c["n_fft"], spec)
    if key not in _BANKS:
        K = c["n_fft"] // 2 + 1
        kind, n = spec
        if kind == "mel":
            w = bhw.mel_weights(c["n_fft"], n, 16000)
        elif kind == "identity":
            w = np.eye(K, dtype=np.float32)
        else:
            w = random_bank(K, n, 100 + c["n_fft"] + n)
        w.setflags(write=False)
        _BANKS[key] = w
    return _BANKS[key]


def width(c):
    w = bank(c)
    return c["n_fft"] // 2 + 1 if w is None else w.shape[1]


def desc(c, forward=False):
    """The bhw_stft of a case: (descriptor, L, frames, col0, pad, detrend).  padded: gaps of 3 floats behind every output row (an odd
    stride: no evenness rule here) and of 7 behind every signal, and of 5 behind every signal of x.  forward: the same call for
    bhw_describe_stft_fft (packed spectrum rows)."""
    n_fft, L, hop, nb, T = c["n_fft"], c["L"], c["hop"], c["B"], c["T"]
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
        xs = T + 5
        if not forward:
            ys = width(c) + 3
            ybs = frames * ys + 7
    s = B.make_stft(nb, T, frames, hop, n_fft, col0=col0, pad=pad, pad_mode=mode, shift=SETUPS[c["setup"]][2] - 1, x_stride=xs, y_stride=ys,
                    y_batch_stride=ybs)
    return s, L, frames, col0, pad, bool(c["detrend"])


def fbank_desc(c):
    """A bhw_fbank for the describe call (host arithmetic: the pointers are not looked at), or None."""
    w = bank(c)
    if w is None:
        return None
    _, offset, _ = fbank_bands(w)
    return B.make_fbank(w.shape[1], w.shape[0], int(offset[-1]), None, None, None)


def line(c, table=None):
    s, L, _, _, _, det = desc(c)
    return B.describe_spectrogram(params(c["setup"]), L, s, detrend=det, fbank=fbank_desc(c), table=table)


def forward_line(c, table=None):
    s, L, _, _, _, det = desc(c, forward=True)
    return B.describe_stft_fft(params(c["setup"]), L, s, detrend=det, table=table)


def _bands(w):
    first, offset, _ = fbank_bands(w)
    return first.astype(np.int64), np.diff(offset.astype(np.int64))


CLASSES = {
    "power mode": lambda c, d, w: d["mode"] == "power" and d["W"] == c["n_fft"] // 2 + 1 and w is None,
    "bank mode": lambda c, d, w: d["mode"] == "bank" and d["W"] == w.shape[1] == d["filters"],
    "fewer filters than lanes per row": lambda c, d, w: d["mode"] == "bank" and d["filters"] < d["lpf"] and d["fpl"] == 1,
    "several filters per lane (n_fft 16, 4 lanes, 10 filters)": lambda c, d, w: d["mode"] == "bank" and (d["n_fft"], d["lpf"], d["filters"], d["fpl"]) == (16, 4, 10, 3),
    "more filters than bins": lambda c, d, w: d["mode"] == "bank" and d["filters"] > c["n_fft"] // 2 + 1,
    "an empty filter": lambda c, d, w: w is not None and bool((_bands(w)[1] == 0).any()),
    "a filter over all K bins": lambda c, d, w: w is not None and bool((_bands(w)[1] == w.shape[0]).any()),
    "filters that take bin 0 and bin M": lambda c, d, w: w is not None and bool((_bands(w)[0][_bands(w)[1] > 0] == 0).any())
    and bool((sum(_bands(w)) == w.shape[0])[_bands(w)[1] > 0].any()),
    "a band with interior zeros": lambda c, d, w: w is not None and d["weights"] > int((w != 0).sum()),
    "the identity bank": lambda c, d, w: w is not None and w.shape[0] == w.shape[1] and np.array_equal(w, np.eye(w.shape[0], dtype=np.float32)),
    "negative weights": lambda c, d, w: w is not None and bool((w < 0).any()),
    "one row per workgroup": lambda c, d, w: d["mode"] == "bank" and d["fy"] == 1,
    "64 rows per workgroup": lambda c, d, w: d["mode"] == "bank" and d["fy"] == 64,
    "a ragged last group": lambda c, d, w: d["mode"] == "bank" and d["fy"] > 1 and d["rows"] % d["fy"] != 0,
    "padded output strides": lambda c, d, w: d["mode"] == "bank" and bool(c.get("padded")),
    "padded output strides, power mode": lambda c, d, w: d["mode"] == "power" and bool(c.get("padded")),
    "detrended segments through a bank": lambda c, d, w: d["mode"] == "bank" and d["detrend"],
    "the group loop through a bank": lambda c, d, w: d["mode"] == "bank" and d["groups"] > d["grid"],
    "the mel bank 80 / 512 / 16000 on the benchmarked batch": lambda c, d, w: (d["mode"], d.get("filters"), d["n_fft"], d["signals"], c["T"], c["L"], c["hop"])
    == ("bank", 80, 512, 64, 160000, 400, 160) and np.array_equal(w, bhw.mel_weights(512, 80, 16000)),
}

POWER_CASES = [dict(c, id="power-" + c["id"], bank=None,
                    classes=("power mode",) + (("padded output strides, power mode",) if c.get("padded") else ())) for c in FC.CASES]

BANK_CASES = [
    dict(id="bank-n16-f10-detrend", setup=1, n_fft=16, L=13, hop=5, mode=None, detrend=True, B=3, T=100, bank=("random", 10),
         classes=("bank mode", "several filters per lane (n_fft 16, 4 lanes, 10 filters)", "more filters than bins", "an empty filter",
                  "a filter over all K bins", "filters that take bin 0 and bin M", "a band with interior zeros", "negative weights",
                  "64 rows per workgroup", "a ragged last group", "detrended segments through a bank")),
    dict(id="bank-n64-identity", setup=3, n_fft=64, L=49, hop=13, mode="constant", detrend=False, B=3, T=150, bank=("identity", 33),
         classes=("the identity bank",)),
    dict(id="bank-n256-mel80", setup=2, n_fft=256, L=256, hop=64, mode="reflect", detrend=False, B=2, T=3000, bank=("mel", 80),
         classes=("an empty filter",)),
    dict(id="bank-n512-f10-padded", setup=0, n_fft=512, L=400, hop=160, mode="reflect", detrend=False, B=2, T=4000, padded=True,
         bank=("random", 10), classes=("fewer filters than lanes per row", "padded output strides")),
    dict(id="bank-n2048-mel128-loop", setup=4, n_fft=2048, L=2048, hop=16, mode="reflect", detrend=False, B=1, T=34000, bank=("mel", 128),
         classes=("one row per workgroup", "the group loop through a bank")),
    dict(id="bank-n4096-f40-padded", setup=0, n_fft=4096, L=4096, hop=5000, mode=None, detrend=True, B=2, T=20000, padded=True,
         bank=("random", 40), classes=("one row per workgroup", "padded output strides")),
    dict(id="bank-bench-mel80", setup=0, n_fft=512, L=400, hop=160, mode="reflect", detrend=False, B=64, T=160000, bank=("mel", 80),
         classes=("the mel bank 80 / 512 / 16000 on the benchmarked batch",)),
]

CASES = POWER_CASES + BANK_CASES


def case_ids(cases=None):
    return [c["id"] for c in (CASES if cases is None else cases)]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
