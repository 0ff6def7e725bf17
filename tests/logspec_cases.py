"""The case table of the fused log spectrogram, log-mel spectrogram and MFCC (bhw_logspec_f32_*, bhw_logspec_mfft_f32_*), in the manner
of tests/spectrogram_cases.py, and the numpy restatement of their contract.

Derived cases: every case of spectrogram_cases.CASES (power and bank) and every power or bank case of stft_mfft_cases.CASES, imported
and not edited, with the log stage; every bank case among them once more with a DCT (all have filters <= n_fft).  New cases: the
classes of the DCT epilogue -- how the coefficients fall on the lanes of a row, the limit filters = n_fft, the workgroup shapes, the
log modes and multipliers.

A class is a predicate on the case and on the describe line of its call (B.describe_logspec / B.describe_logspec_mfft).
tests/test_logspec_host.py (no GPU) proves that every class has a case, that every claim holds and that the describe line's plan
fields are the parent's for the same call; tests/test_gpu_logspec.py runs every case, library and table.
"""
import math
import re

import numpy as np

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from blackman_harris_win_amd.selector import fbank_bands, log_multiplier

import spectrogram_cases as SC
import stft_mfft_cases as MC

params = SC.params
ROW_GAP, SIGNAL_GAP = 3, 7                # floats behind every output row and every signal of a padded case

# name -> (log, floor, add): the three named logs, a negative multiplier, both modes
LOGS = {
    "db": ("db", 1e-10, False),
    "ln-add": ("ln", 1e-6, True),
    "log10": ("log10", 1e-3, False),
    "neg": (-2.5, 0.5, False),
    "db-add": ("db", 1.0, True),
}


# ---- the numpy restatement of the contract -------------------------------------------------------------------------------------------

def log_ref(q, mult, floor, add):
    """g = fl32(mult * log(t)) of the float32 words q: t = q + floor (add) or max(q, floor) with a NaN passed through (clamp), in
    float64."""
    q = np.asarray(q, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = q + floor if add else np.where(q < floor, floor, q)
        return (mult * np.log(t)).astype(np.float32)


def dct_ref(g, dense):
    """c_j = fl32(sum over m of (double) g_m * (double) D[m, j]) in ascending m from +0.0: plain float64 `acc + a * b`, which equals the
    fma chain because a product of two float32 values is exact in float64.  g (R, filters) float32, dense (filters, coeffs) float32."""
    g64, d64 = np.asarray(g, dtype=np.float32).astype(np.float64), np.asarray(dense, dtype=np.float32).astype(np.float64)
    acc = np.zeros((g64.shape[0], d64.shape[1]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(d64.shape[0]):
            acc = acc + g64[:, m:m + 1] * d64[m:m + 1, :]
        return acc.astype(np.float32)


def ulps_apart(a, b):
    """The distance of two float32 arrays in units in the last place (0 where both are NaN, a huge number where one is)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.abs(ia - ib)
    na, nb = np.isnan(a), np.isnan(b)
    d[na & nb] = 0
    d[na ^ nb] = 1 << 40
    return d


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

def _bank_spec(family, base):
    if family == "pow2":
        return base.get("bank")
    return ("mel", MC.BANK_FILTERS) if base.get("form") == "bank" else None


def _derived():
    out = []
    clamp_logs, any_logs = ("db", "log10", "neg"), ("db", "ln-add", "log10", "neg", "db-add")
    for family, bases in (("pow2", SC.CASES), ("mixed", [c for c in MC.CASES if c.get("form") in ("power", "bank")])):
        for i, base in enumerate(bases):
            spec = _bank_spec(family, base)
            # a random bank has negative weights: its values may be negative, and log(q + floor) of those is a NaN -- clamp them
            pool = clamp_logs if spec and spec[0] == "random" else any_logs
            stem = ("p2-" if family == "pow2" else "mx-") + base["id"]
            out.append(dict(id=stem + "-log", family=family, base=base, bank=spec, log=pool[i % len(pool)], coeffs=0,
                            classes=("derived: log of a parent case",)))
            if spec:
                out.append(dict(id=stem + "-dct", family=family, base=base, bank=spec, log=pool[(i + 1) % len(pool)],
                                coeffs=min(13, spec[1]), dct="ortho", classes=("derived: DCT of a parent bank case",)))
    return out


def _base(n_fft, L, hop, mode, detrend, nb, T, setup=0, padded=False):
    return dict(setup=setup, n_fft=n_fft, L=L, hop=hop, mode=mode, detrend=detrend, B=nb, T=T, padded=padded)


NEW_CASES = [
    dict(id="dct-n16-f16-c10", family="pow2", base=_base(16, 13, 5, None, True, 3, 100, setup=1), bank=("random", 16), log="db", coeffs=10,
         dct="random", classes=("several coefficients per lane", "filters = n_fft (n_fft 16)", "64 rows per workgroup", "clamp mode",
                                "log db", "a ragged last group")),
    dict(id="dct-n64-square-identity", family="pow2", base=_base(64, 49, 13, "constant", False, 3, 150, setup=3), bank=("random", 12),
         log="log10", coeffs=12, dct="identity", classes=("a square matrix", "the identity matrix", "log log10")),
    dict(id="dct-n128-c1-padded", family="pow2", base=_base(128, 100, 37, "reflect", False, 4, 2000, setup=2, padded=True), bank=("mel", 20),
         log="ln-add", coeffs=1, dct="ortho", classes=("one coefficient", "add mode", "log ln", "padded output strides")),
    dict(id="dct-n2048-mel128-c40", family="pow2", base=_base(2048, 2048, 512, "reflect", False, 1, 12000, setup=4), bank=("mel", 128),
         log="neg", coeffs=40, dct="ortho", classes=("one row per workgroup", "a negative multiplier")),
    dict(id="dct-m18-f18-c18", family="mixed", base=_base(18, 13, 5, None, True, 3, 100, setup=1), bank=("random", 18), log="neg", coeffs=18,
         dct="random", classes=("filters = n_fft (the smallest mixed size)", "several coefficients per lane", "64 rows per workgroup",
                                "a square matrix", "a negative multiplier")),
    dict(id="dct-m400-mel80-c13", family="mixed", base=_base(400, 400, 160, "reflect", False, 2, 4000), bank=("mel", 80), log="ln-add",
         coeffs=13, dct="ortho", classes=("the MFCC front end 400 / 160 / 80 mel / 13", "add mode", "log ln")),
    dict(id="dct-m1200-mel64-c20-padded", family="mixed", base=_base(1200, 1200, 300, "reflect", False, 2, 6000, setup=4, padded=True),
         bank=("mel", 64), log="db-add", coeffs=20, dct="ortho", classes=("one row per workgroup", "padded output strides", "log db")),
    dict(id="log-m30-power-log10", family="mixed", base=_base(30, 24, 7, "constant", False, 3, 150, setup=3), bank=None, log="log10", coeffs=0,
         classes=("power rows, mixed", "log log10")),
]

CASES = _derived() + NEW_CASES


def case_ids(cases=None):
    return [c["id"] for c in (CASES if cases is None else cases)]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)


_BANKS, _DCTS = {}, {}


def bank(c):
    """The dense (K, filters) float32 array of the case's bank (cached), or None."""
    spec = c["bank"]
    if spec is None:
        return None
    n_fft = c["base"]["n_fft"]
    key = (n_fft, spec)
    if key not in _BANKS:
        K, (kind, n) = n_fft // 2 + 1, spec
        if kind == "mel":
            w = bhw.mel_weights(n_fft, n, 16000)
        elif kind == "identity":
            w = np.eye(K, dtype=np.float32)
        else:
            w = SC.random_bank(K, n, 100 + n_fft + n)
        w.setflags(write=False)
        _BANKS[key] = w
    return _BANKS[key]


def dct(c):
    """The dense (filters, coeffs) float32 matrix of a DCT case (cached), or None."""
    if not c["coeffs"]:
        return None
    filters, key = bank(c).shape[1], (bank(c).shape[1], c["coeffs"], c["dct"])
    if key not in _DCTS:
        if c["dct"] == "ortho":
            d = bhw.dct_weights(c["coeffs"], filters)
        elif c["dct"] == "identity":
            d = np.eye(filters, c["coeffs"], dtype=np.float32)
        else:
            d = (np.random.default_rng(filters * 4099 + c["coeffs"]).random((filters, c["coeffs"])) - 0.4).astype(np.float32)
        d.setflags(write=False)
        _DCTS[key] = d
    return _DCTS[key]


def parent_width(c):
    w = bank(c)
    return c["base"]["n_fft"] // 2 + 1 if w is None else w.shape[1]


def width(c):
    return c["coeffs"] or parent_width(c)


def log_args(c):
    """(mult, floor, add) of the case."""
    log, floor, add = LOGS[c["log"]]
    return log_multiplier(log), floor, add


def call_kw(c):
    """The keyword arguments of bhw.log_spectrogram(_mixed) / bhw.spectrogram(_mixed) that frame the case."""
    b = c["base"]
    if b["detrend"]:
        return dict(win_length=b["L"], center=False, detrend=True)
    return dict(win_length=b["L"], center=bool(b["mode"]), pad_mode=b["mode"] or "reflect")


def desc(c, parent=False):
    """The bhw_stft of a case: (descriptor, L, frames, detrend); a padded case has gaps of ROW_GAP floats behind every output row and
    SIGNAL_GAP behind every signal (of the parent's rows under parent=True) and of 5 samples behind every signal of x."""
    b = c["base"]
    n_fft, L, hop, nb, T = b["n_fft"], b["L"], b["hop"], b["B"], b["T"]
    if b["detrend"]:
        pad, col0, mode = 0, 0, B.PAD_CONSTANT
        frames = 1 + (T - L) // hop
    else:
        pad = n_fft // 2 if b["mode"] else 0
        col0 = (n_fft - L) // 2
        mode = B.PAD_REFLECT if b["mode"] == "reflect" else B.PAD_CONSTANT
        frames = 1 + (T + 2 * pad - n_fft) // hop
    xs, ys, ybs = 0, 0, 0
    if b.get("padded"):
        xs = T + 5
        ys = (parent_width(c) if parent else width(c)) + ROW_GAP
        ybs = frames * ys + SIGNAL_GAP
    s = B.make_stft(nb, T, frames, hop, n_fft, col0=col0, pad=pad, pad_mode=mode, shift=SC.SETUPS[b["setup"]][2] - 1, x_stride=xs,
                    y_stride=ys, y_batch_stride=ybs)
    return s, L, frames, bool(b["detrend"])


def fbank_desc(c):
    """A bhw_fbank for the describe calls (host arithmetic: the pointers are not looked at), or None."""
    w = bank(c)
    if w is None:
        return None
    _, offset, _ = fbank_bands(w)
    return B.make_fbank(w.shape[1], w.shape[0], int(offset[-1]), None, None, None)


def logspec_desc(c):
    mult, floor, add = log_args(c)
    return B.make_logspec(floor, mult, add=add, coeffs=c["coeffs"], dct_rows=parent_width(c) if c["coeffs"] else 0)


def line(c, table=None):
    s, L, _, det = desc(c)
    fn = B.describe_logspec if c["family"] == "pow2" else B.describe_logspec_mfft
    return fn(params(c["base"]["setup"]), L, s, logspec_desc(c), detrend=det, fbank=fbank_desc(c), table=table)


def parent_line(c, table=None):
    s, L, _, det = desc(c, parent=True)
    p = params(c["base"]["setup"])
    if c["family"] == "pow2":
        return B.describe_spectrogram(p, L, s, detrend=det, fbank=fbank_desc(c), table=table)
    return B.describe_stft_mfft(p, L, s, detrend=det, power=True, fbank=fbank_desc(c), table=table)


def plan_text(text):
    """The plan fields of a describe line: everything from the signals on."""
    return re.search(r"\d+ signals x .*$", text).group(0)


def parse(text):
    d = MC.parse(text)
    m = re.search(r"log (clamp|add) floor (\S+), mult (\S+?)(?:,|$)", text)
    d["mode"], d["floor"], d["mult"] = (m.group(1), float(m.group(2)), float(m.group(3))) if m else (None, None, None)
    m = re.search(r"DCT (\d+) x (\d+)", text)
    d["dct"] = (int(m.group(1)), int(m.group(2))) if m else None
    m = re.search(r"W = (\d+):", text)
    d["W"] = int(m.group(1)) if m else None
    d["rows_form"] = "bank" if "bank rows" in text else "power" if "power rows" in text else None
    return d


def _mult(name):
    return lambda c, d: math.isclose(d["mult"], log_multiplier(name), rel_tol=1e-15) and LOGS[c["log"]][0] == name


CLASSES = {
    "derived: log of a parent case": lambda c, d: d["dct"] is None and d["W"] == parent_width(c),
    "derived: DCT of a parent bank case": lambda c, d: d["dct"] == (parent_width(c), c["coeffs"]) and d["W"] == c["coeffs"],
    "one coefficient": lambda c, d: d["dct"] is not None and d["dct"][1] == 1 and d["W"] == 1,
    "several coefficients per lane": lambda c, d: d["dct"] is not None and d["dct"][1] > d["lpf"],
    "a square matrix": lambda c, d: d["dct"] is not None and d["dct"][0] == d["dct"][1],
    "the identity matrix": lambda c, d: d["dct"] is not None and np.array_equal(dct(c), np.eye(*d["dct"], dtype=np.float32)),
    "filters = n_fft (n_fft 16)": lambda c, d: c["family"] == "pow2" and d["dct"] is not None and d["dct"][0] == d["n_fft"] == 16,
    "filters = n_fft (the smallest mixed size)": lambda c, d: c["family"] == "mixed" and d["dct"] is not None and d["dct"][0] == d["n_fft"] == 18,
    "one row per workgroup": lambda c, d: d["dct"] is not None and d["fy"] == 1,
    "64 rows per workgroup": lambda c, d: d["dct"] is not None and d["fy"] == 64,
    "a ragged last group": lambda c, d: d["dct"] is not None and d["fy"] > 1 and d["rows"] % d["fy"] != 0,
    "padded output strides": lambda c, d: d["dct"] is not None and bool(c["base"].get("padded")),
    "clamp mode": lambda c, d: d["dct"] is not None and d["mode"] == "clamp",
    "add mode": lambda c, d: d["dct"] is not None and d["mode"] == "add",
    "log db": _mult("db"),
    "log ln": _mult("ln"),
    "log log10": _mult("log10"),
    "a negative multiplier": lambda c, d: d["mult"] < 0,
    "power rows, mixed": lambda c, d: c["family"] == "mixed" and d["rows_form"] == "power" and d["dct"] is None,
    "the MFCC front end 400 / 160 / 80 mel / 13": lambda c, d: (c["family"], d["n_fft"], c["base"]["hop"], d["dct"], d["mode"]) ==
    ("mixed", 400, 160, (80, 13), "add") and np.array_equal(bank(c), bhw.mel_weights(400, 80, 16000)),
}

# what the derived cases must carry over from the parents' tables (checked by the coverage test on the parent's own class names)
PARENT_CLASSES_POW2 = ("several filters per lane (n_fft 16, 4 lanes, 10 filters)", "an empty filter", "a filter over all K bins", "the identity bank",
                       "negative weights", "a ragged last group", "the group loop through a bank", "padded output strides",
                       "padded output strides, power mode", "power mode")
PARENT_CLASSES_MIXED = ("bank output", "power output", "padded strides")
