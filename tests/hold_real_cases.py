"""The case table of the fused max-hold / min-hold traces for real input, both families (bhw_hold_fft_f32_*, bhw_hold_mfft_f32_*).

The plan of a hold call IS the plan of its Welch sibling (BhwHoldFftPlan wraps BhwWelchFftPlan, BhwHoldMfftPlan wraps
BhwWelchMfftPlan), and the epilogue of bhw_hold_real.h branches where the Welch epilogues do: whole chunks per group from fy 16 on,
carried per-lane pairs below, the live-slot count, the run's last group, bin M aside.  So the shapes are not restated: the cases are
welch_fft_cases.CASES and welch_mfft_cases.CASES, with the classes they claim there, read on the hold call's own describe line
(B.describe_hold_fft / B.describe_hold_mfft: the sibling's fields in the same words, plus the traces that are stored).  What this table
adds is the classes of the traces: "max only", "min only", "both".

tests/test_hold_real_plan_coverage.py (no GPU) proves that every class has a case, that every claim holds on the hold line, that a sweep
of the planner over all 9 + 95 sizes emits no regime the table lacks and that the shared fields equal the Welch sibling's line;
tests/test_gpu_hold_real.py runs every case, library and table, the traces each way and the doubling both ways, bit for bit against
amax / amin of bhw.spectrogram(_mixed)'s rows.
"""
import re

from blackman_harris_win_amd import binding as B

import welch_fft_cases as WF
import welch_mfft_cases as WM

CHUNK, BLOCK = B.WELCH_FFT_CHUNK, B.WELCH_BLOCK
FAMILIES = ("fft", "mfft")
_MOD = {"fft": WF, "mfft": WM}
_DESCRIBE = {"fft": B.describe_hold_fft, "mfft": B.describe_hold_mfft}
_WELCH = {"fft": B.describe_welch_fft, "mfft": B.describe_welch_mfft}
HOLD_WS = {"fft": B.hold_fft_workspace_bytes, "mfft": B.hold_mfft_workspace_bytes}
WELCH_WS = {"fft": B.welch_fft_workspace_bytes, "mfft": B.welch_mfft_workspace_bytes}
SIZES = {"fft": [1 << e for e in range(4, 13)],
         "mfft": [n for n in range(B.MFFT_MIN_N, B.MFFT_MAX_N + 1) if B.mfft_supported(n)]}
TRACES = ("both", "max", "min")
params = WF.params


def desc(family, c):
    return _MOD[family].desc(c)


def parse(family, line):
    """The sibling's fields (its parser reads the hold line: the words are the same) and the traces."""
    d = _MOD[family].parse(line)
    m = re.search(r"; traces: (max, min|max|min)$", line)
    d["traces"] = {"max, min": "both", "max": "max", "min": "min"}[m.group(1)] if m else None
    return d


def line(family, c, table=None, traces="both"):
    s, L, _, det = desc(family, c)
    return _DESCRIBE[family](params(c["setup"]), L, s, detrend=det, traces=traces, table=table)


def welch_line(family, c, table=None):
    s, L, _, det = desc(family, c)
    return _WELCH[family](params(c["setup"]), L, s, detrend=det, table=table)


def to_welch(family, text):
    """A hold line in the Welch sibling's names: the call, the kernels and the join, without the traces."""
    text = re.sub(r"; traces: (max, min|max|min)$", "", text)
    return text.replace(f"hold {family} ", f"welch {family} ").replace(f"k_hold_{family}_", f"k_welch_{family}_").replace("k_hold_join", "k_welch_fft_join")


def aside(family, m):
    """Whether bin M = n_fft / 2 is reduced aside on lane 0 (bhw_hold_real.h, as the Welch siblings)."""
    return m >= 256 if family == "fft" else m % 256 == 0


def regime(family, d):
    """What the epilogue branches on, a function of n_fft alone: the rows side by side, the groups of a run, the pairs a lane carries
    and whether bin M is aside."""
    return (d["fy"], d["gpr"], d["acc"], d["fy"] < CHUNK and aside(family, d["n_fft"] // 2))


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


def case_ids(family=None):
    return [c["id"] for c in CASES if family in (None, c["family"])]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)
