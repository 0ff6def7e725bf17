"""The case table of the fused max-hold / min-hold traces for I/Q input, both families (bhw_hold_cfft_f32_*, bhw_hold_cmfft_f32_*).

The plan of a hold call IS the plan of its Welch sibling (BhwHoldCfftPlan wraps BhwWelchCfftPlan, BhwHoldCmfftPlan wraps
BhwWelchCmfftPlan), and the epilogue of bhw_hold.h branches where the Welch epilogues do: whole chunks per group from fy 16 on, carried
per-lane values below, the live-slot count, the run's last group, the column turn.  So the shapes are not restated: the cases are
welch_cfft_cases.CASES and welch_cmfft_cases.CASES, with the classes they claim there, read on the hold call's own describe line
(B.describe_hold_cfft / B.describe_hold_cmfft: the sibling's fields in the same words, plus the traces that are stored).  They reach
both regimes, every accumulator count 1..8, odd n, ragged and whole last chunks, F = 1 and 15, two and three blocks, 513 blocks, the run
loop, a padded p_stride, detrend and reflect.  What this table adds is the classes of the traces: "max only", "min only", "both".

tests/test_hold_iq_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds on the hold line, that a sweep
of the planner over all 8 + 91 sizes emits no regime the table lacks and that the shared fields equal the Welch sibling's line;
tests/test_gpu_hold_iq.py runs every case, library and table, shifted and not, the traces each way, bit for bit against amax / amin of
bhw.spectrogram_iq(_mixed)'s rows.
"""
import re

from blackman_harris_win_amd import binding as B

import welch_cfft_cases as WC
import welch_cmfft_cases as WM

CHUNK, BLOCK = B.WELCH_FFT_CHUNK, B.WELCH_BLOCK
FAMILIES = ("cfft", "cmfft")
_MOD = {"cfft": WC, "cmfft": WM}
_DESCRIBE = {"cfft": B.describe_hold_cfft, "cmfft": B.describe_hold_cmfft}
_WELCH = {"cfft": B.describe_welch_cfft, "cmfft": B.describe_welch_cmfft}
SIZES = {"cfft": [1 << e for e in range(4, 12)], "cmfft": list(WM.SIZES)}
TRACES = ("both", "max", "min")
params, desc = WC.params, WC.desc


def parse(family, line):
    """The sibling's fields (its parser reads the hold line: the words are the same) and the traces."""
    d = _MOD[family].parse(line)
    m = re.search(r"; traces: (max, min|max|min)$", line)
    d["traces"] = {"max, min": "both", "max": "max", "min": "min"}[m.group(1)] if m else None
    return d


def line(family, c, table=None, fftshift=False, traces="both"):
    s, L, _, det = desc(c)
    return _DESCRIBE[family](params(c["setup"]), L, s, detrend=det, fftshift=fftshift, traces=traces, table=table)


def welch_line(family, c, table=None, fftshift=False):
    s, L, _, det = desc(c)
    return _WELCH[family](params(c["setup"]), L, s, detrend=det, fftshift=fftshift, table=table)


def to_welch(family, text):
    """A hold line in the Welch sibling's names: the call, the kernels and the join, without the traces."""
    text = re.sub(r"; traces: (max, min|max|min)$", "", text)
    return text.replace(f"hold {family} ", f"welch {family} ").replace(f"k_hold_{family}_", f"k_welch_{family}_").replace("k_hold_join", "k_welch_fft_join")


def regime(d):
    """What the epilogue branches on, a function of n_fft alone (welch_cmfft_cases.regime)."""
    return (d["fy"], d["gpr"], d["acc"])


def _renamed(family, pred):
    """A sibling's class on a hold line: its predicates name the sibling's kernels."""
    def f(c, d):
        d = dict(d)
        d["kernels"] = {k.replace(f"k_hold_{family}_", f"k_welch_{family}_"): v for k, v in d["kernels"].items()}
        return pred(c, d)
    return f


TRACE_CLASSES = {
    "both traces": lambda c, d: d["traces"] == "both",
    "max only": lambda c, d: d["traces"] == "max",
    "min only": lambda c, d: d["traces"] == "min",
}
# per family: the sibling's classes, then the traces
CLASSES = {fam: {**{n: _renamed(fam, p) for n, p in _MOD[fam].CLASSES.items()}, **TRACE_CLASSES} for fam in FAMILIES}

# The traces a case is described (and, on the GPU, first run) with: they rotate over the table, so that each selection meets both
# regimes in both families; the GPU test runs every case with all three.
CASES = []
for _fam in FAMILIES:
    for _i, _c in enumerate(_MOD[_fam].CASES):
        _t = TRACES[_i % 3]
        CASES.append(dict(_c, family=_fam, id=f"{_fam}-{_c['id']}", traces=_t,
                          classes=tuple(_c["classes"]) + ({"both": "both traces", "max": "max only", "min": "min only"}[_t],)))

SHIFTED = tuple(f"cfft-{i}" for i in WC.SHIFTED) + tuple(f"cmfft-{i}" for i in WM.SHIFTED)


def case_ids(family=None):
    return [c["id"] for c in CASES if family in (None, c["family"])]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
