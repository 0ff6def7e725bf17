"""The inputs, geometries, references and bounds of the epilogue size sweep: every n_fft of the four fused forward FFT families under
every epilogue that is not the stored spectrum -- the power rows (spectrogram*), the filter bank, the frame average (welch_fft*) and
the max- / min-hold traces (hold_fft*).  Pure NumPy (no GPU, no torch), so tests/test_epilogue_sweep_rows.py (a float32 CPU library
pushed through the same epilogues, no GPU), tests/test_gpu_epilogue_size_sweep.py (the kernels) and tools/sweep_fft_sizes.py
--epilogues (the record) share them.

Why: the size sweeps (fft_sweep_rows.py, iq_mixed_sweep_rows.py) run every size under the store epilogue only.  The accumulating
epilogues read other lanes' points out of LDS behind the last pass, map lanes to bins by fy, K and M, mask frames by fy against F and
compile the row function again; their class tables name 10 to 16 sizes each.

Families and sizes (the lists of the sweeps, none left out): "mixed" fft_sweep_rows.SIZES (95), "iq_mixed" iq_mixed_sweep_rows.SIZES
(91), "real" POW2_REAL (9), "iq" POW2_IQ (8).  The index i of a size is its position in its own list.

Signals: the forward rows of the sweeps at this geometry's length -- noise, impulse, exact-bin tones, DC + Nyquist -- so that one
wrong bin is not diluted.

Geometry of size n, index i: hop n // 4 + 1.
  even i: L = n, centred, reflect padding, F = 35 frames per signal, T the smallest length that gives 35.  35 is two whole chunks of
          16 and a ragged one of 3; with fy = 32 a full group, then a group of a live chunk of 3 and a chunk of pure padding that
          must not be stored; with fy < 16 three runs, and at fy = 2 groups with 2, 1 and 0 live slots.
  odd i:  L = n - 3, center=False, detrend=True, F = 19, T = (F - 1) * hop + L: one whole chunk and a ragged one under detrending.
          Detrending forms Welch segments, so the window stands at column 0 (the library's rule), not at (n - L) // 2.
Parameter set: fft_sweep_rows.setup_for(i, L).

Filter bank of size n (bank): a dense (K, 6) float64 array of float32 values, K = n // 2 + 1: a filter on bin 0 alone, one on bin M
alone, a triangle over the lowest quarter, a ramp ending at M, a flat band over all K bins, and a band straddling bins 255 / 256
where K > 256, else K // 2.

Float64 references, independent of the library's stft*: rows() restates the float32 rows the transform must see (fft_sweep_rows.frames;
under detrending the segment mean m = fl32(binary64 sum / L), y = fl32(fl32(x - m) * v), as welch_frames defines them);
spectrum64() is numpy.fft.rfft / fft of them in float64; P64 = |Y64|^2; welch64 = s_k * sum over frames (the library's scale carries
the 1 / F of the mean), hold64 = s_k * max / min over frames, bank64 = P64 @ W.

Bounds, derived and not measured.  Let g = gate(n, row): the relative l2 error of a row the stored spectrum is already held to, so
Y = Y64 + e with |e|_2 <= g |Y64|_2 in every frame.  Then | |Y_k|^2 - |Y64_k|^2 | <= 2 |Y64_k| |e_k| + |e_k|^2, and by
Cauchy-Schwarz over k the sum is at most (2 g + g^2) sum_k P64_k.  P_k = fl32(|Y_k|^2) adds at most 2^-24 |Y_k|^2, in sum
2^-24 (1 + g)^2 sum_k P64_k <= 2^-23 sum_k P64_k.  So for one frame

    sum_k |P_k - P64_k| <= (2 g + g^2 + 2^-23) sum_k P64_k                                            power_bound(n, row)

  Welch: the kernel sums q = |Y_k|^2 in binary64 (no fl32 of a power, so the 2^-23 term is slack), and the frame sum of the left
         sides is bounded by the frame sum of the right sides; the one rounding of A * s_k adds 2^-24.     welch_bound = power + 2^-24
         The factor s_k (scale, doubled for the one-sided bins) is divided out of the result in float64 before the sum over k, so
         that the Cauchy-Schwarz step above stands unweighted.
  Hold:  |max_f a_f - max_f b_f| <= max_f |a_f - b_f| per bin (and the same for min); the trace is held to the power bound of the
         loudest frame's sum_k P64_k, per signal.  Summed over the bins this takes the worst frames of different bins not to
         conspire: the rigorous constant is F times larger.  tests/test_epilogue_sweep_rows.py shows that a float32 library stays
         inside it at every size.  The sweep calls hold_fft* with a power-of-two scale, so s_k multiplies exactly and the trace
         carries no rounding beyond the power's own.                                                        hold_bound = power
  Bank:  |sum_k W_km (P_k - P64_k)| <= max |W| sum_k |P_k - P64_k|, against sum_k P64_k of the frame.   bank_bound = power * max |W|
         The band sum's own rounding (2^-24 of at most max |W| sum_k P_k) is covered by the slack of the 2^-23 term to first order.
"""
import numpy as np

import fft_sweep_rows as R
import iq_mixed_sweep_rows as Q
import welch_cfft_cases as WC
import welch_cmfft_cases as WX
import welch_fft_cases as WF
import welch_mfft_cases as WM

FAMILIES = {"mixed": R.SIZES, "iq_mixed": Q.SIZES, "real": R.POW2_REAL, "iq": R.POW2_IQ}
assert [len(FAMILIES[f]) for f in ("mixed", "iq_mixed", "real", "iq")] == [95, 91, 9, 8]
IQ = {"mixed": False, "iq_mixed": True, "real": False, "iq": True}
WELCH_CASES = {"mixed": WM, "iq_mixed": WX, "real": WF, "iq": WC}           # the Welch sibling's describe line and its parser
F_EVEN, F_ODD = 35, 19
CHUNK = 16
LANES = 256
ASIDE = (1536, 2560, 3072)                                                 # the mixed-radix sizes with M % 256 == 0
FILTERS = 6
WELCH_SCALE_C, HOLD_SCALE = 1.0 / 3.7, 2.0 ** -6                          # welch_fft* takes WELCH_SCALE_C / F; hold_fft* a power of two

gate = R.gate


def row_types(fam):
    return R.ROW_TYPES_IQ if IQ[fam] else R.ROW_TYPES


def bins(fam, n):
    return n if IQ[fam] else n // 2 + 1


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------

def case(fam, n):
    """The call of size n of family fam as a case of the Welch siblings' tables (the keys their desc() and line() read), plus frames,
    col0, pad and T."""
    i = FAMILIES[fam].index(n)
    hop = n // 4 + 1
    nb = R.NB_IQ if IQ[fam] else R.NB
    if i % 2 == 0:
        L, pad, F = n, n // 2, F_EVEN
        T = (F - 1) * hop + n - 2 * pad                                    # the smallest T with 1 + (T + 2 pad - n) // hop == F
        assert 1 + (T + 2 * pad - n) // hop == F and 1 + (T - 1 + 2 * pad - n) // hop == F - 1 and pad < T
        return dict(id=f"{fam}-n{n}", setup=R.setup_for(i, L), n_fft=n, L=L, hop=hop, mode="reflect", detrend=False, B=nb, T=T, col0=0,
                    pad=pad, frames=F)
    L, F = n - 3, F_ODD
    return dict(id=f"{fam}-n{n}", setup=R.setup_for(i, L), n_fft=n, L=L, hop=hop, mode=None, detrend=True, B=nb, T=(F - 1) * hop + L,
                col0=0, pad=0, frames=F)


def call_kw(c):
    """The keyword arguments of every front for the case (welch_fft* and hold_fft* default to center=False: all are named)."""
    if c["detrend"]:
        return dict(win_length=c["L"], center=False, detrend=True)
    return dict(win_length=c["L"], center=True, pad_mode="reflect", detrend=False)


def signals(fam, n):
    """(B, T) float32 or complex64: the sweeps' forward rows at the case's length."""
    T = case(fam, n)["T"]
    if fam == "iq_mixed":
        return Q.forward_signals_iq(n, T)
    return R.forward_signals_iq(n, T) if IQ[fam] else R.forward_signals(n, T)


def plan(fam, n):
    """The parsed describe line of the Welch sibling of the case (as the class tables parse it)."""
    mod = WELCH_CASES[fam]
    return mod.parse(mod.line(case(fam, n)))


# ---- the filter bank ---------------------------------------------------------------------------------------------------------------------

def bank_edges(n):
    """[(first bin, last bin)] of the six filters of size n."""
    M = n // 2
    K = M + 1
    q = max(2, K // 4)
    mid = (250, min(M, 261)) if K > LANES else (max(0, K // 2 - 2), min(M, K // 2 + 1))
    return [(0, 0), (M, M), (0, q), (M - q, M), (0, M), mid]


def bank(n):
    """(K, 6) float64 holding float32 values: every weight inside a band is positive, so the bands of the sparse form are bank_edges."""
    K = n // 2 + 1
    e = bank_edges(n)
    W = np.zeros((K, FILTERS))
    W[0, 0] = 1.0
    W[K - 1, 1] = 0.5
    lo, hi = e[2]
    k = np.arange(lo, hi + 1)
    W[lo:hi + 1, 2] = 1.0 - np.abs(k - hi / 2.0) / (hi / 2.0 + 1.0)         # a triangle, positive at both ends
    lo, hi = e[3]
    W[lo:hi + 1, 3] = (np.arange(lo, hi + 1) - lo + 1.0) / (hi - lo + 1.0)  # a ramp ending at M with weight 1
    W[:, 4] = 1.0
    lo, hi = e[5]
    W[lo:hi + 1, 5] = 0.75
    return W.astype(np.float32).astype(np.float64)


# ---- float64 references -------------------------------------------------------------------------------------------------------------------

def rows(x, v, c):
    """x (B, T) float32 or complex64, v (L,) float32 -> the float32 rows (B, frames, n_fft) the transform must see."""
    if not c["detrend"]:
        return R.frames(x, v, c)
    L, n = c["L"], c["n_fft"]
    assert len(v) == L
    idx = np.arange(c["frames"])[:, None] * c["hop"] + np.arange(L)[None, :]
    seg = x[:, idx]                                                        # (B, F, L)
    s = seg.astype(np.complex128 if np.iscomplexobj(x) else np.float64).sum(axis=-1) / np.float64(L)
    m = s.astype(x.dtype)                                                  # each part rounded once to float32
    y = np.zeros((x.shape[0], c["frames"], n), dtype=x.dtype)
    y[:, :, :L] = (seg - m[:, :, None]).astype(x.dtype) * v[None, None, :]
    return y


def spectrum64(r):
    """numpy.fft.rfft (real rows) or fft (complex rows) of the rows in float64."""
    if np.iscomplexobj(r):
        return np.fft.fft(r.astype(np.complex128), axis=-1)
    return np.fft.rfft(r.astype(np.float64), axis=-1)


def power64(Y):
    return Y.real ** 2 + Y.imag ** 2


def sk(fam, n, scale, doubled):
    """(K,) float64: the factor of bin k -- scale, times 2 for the one-sided bins of real input (every bin but 0 and n / 2) where
    doubled."""
    s = np.full(bins(fam, n), float(scale))
    if doubled and not IQ[fam]:
        s[1:-1] *= 2.0
    return s


def welch64(P64, s):
    """P64 (B, F, K), s (K,) -> (B, K): s_k times the sum over the frames (s carries the 1 / F of the mean)."""
    return P64.sum(axis=1) * s


def hold64(P64, s):
    return P64.max(axis=1) * s, P64.min(axis=1) * s


def bank64(P64, W):
    return P64 @ W


# ---- bounds -------------------------------------------------------------------------------------------------------------------------------

def power_bound(n, row):
    """(2 g + g^2 + 2^-23): Cauchy-Schwarz on 2 |Y| |e| + |e|^2 with |e|_2 <= g |Y64|_2, and one float32 rounding of the power."""
    g = gate(n, row)
    return 2.0 * g + g * g + 2.0 ** -23


def welch_bound(n, row):
    """The power bound, both sides summed over the frames, plus 2^-24 for the one rounding of A * s_k."""
    return power_bound(n, row) + 2.0 ** -24


def hold_bound(n, row):
    """The power bound, against the loudest frame: |max a - max b| <= max |a - b| (a power-of-two scale adds no rounding)."""
    return power_bound(n, row)


def bank_bound(n, row, W):
    """The power bound times max |W|, against sum_k P64_k of the frame."""
    return power_bound(n, row) * float(np.abs(W).max())


# ---- the metrics: each the ratio of an error to its bound, per signal; at most 1 passes ----------------------------------------------------

def _ratio(err, allowed):
    """max err / allowed over the entries; an entry whose allowance is zero must have no error."""
    err, allowed = np.asarray(err, dtype=np.float64), np.asarray(allowed, dtype=np.float64)
    assert np.isfinite(err).all(), "a result is not finite"
    zero = allowed == 0
    assert not (err[zero] != 0).any(), "a row of zero power must give zeros"
    return float((err[~zero] / allowed[~zero]).max()) if (~zero).any() else 0.0


def power_ratios(fam, n, P, P64):
    """P (B, F, K) against P64: per signal, the largest sum_k |P - P64| / (bound * sum_k P64) over the frames."""
    P = np.asarray(P, dtype=np.float64)
    err, tot = np.abs(P - P64).sum(axis=-1), P64.sum(axis=-1)
    return [_ratio(err[b], power_bound(n, b) * tot[b]) for b in range(P.shape[0])]


def bank_ratios(fam, n, S, P64, W):
    """S (B, F, 6) against P64 @ W: per signal, the largest |S - ref| / (bound * sum_k P64 of the frame) over frames and filters."""
    S = np.asarray(S, dtype=np.float64)
    err, tot = np.abs(S - bank64(P64, W)).max(axis=-1), P64.sum(axis=-1)
    return [_ratio(err[b], bank_bound(n, b, W) * tot[b]) for b in range(S.shape[0])]


def welch_ratios(fam, n, got, P64, s):
    """got (B, K) = welch_fft*(..., scale) against welch64(P64, s), s_k divided out of both in float64."""
    got = np.asarray(got, dtype=np.float64) / s
    err, tot = np.abs(got - P64.sum(axis=1)).sum(axis=-1), P64.sum(axis=(1, 2))
    return [_ratio(err[b], welch_bound(n, b) * tot[b]) for b in range(got.shape[0])]


def hold_ratios(fam, n, got, P64, s, which):
    """got (B, K) = a hold trace against hold64(P64, s)[which], s_k divided out, the allowance that of the loudest frame."""
    got = np.asarray(got, dtype=np.float64) / s
    ref = P64.max(axis=1) if which == "max" else P64.min(axis=1)
    err, loud = np.abs(got - ref).sum(axis=-1), P64.sum(axis=-1).max(axis=-1)
    return [_ratio(err[b], hold_bound(n, b) * loud[b]) for b in range(got.shape[0])]


def sentinel_sizes(fam):
    """The sizes whose calls also run into sentinel-filled outputs: the smallest and the largest of the list and, for "mixed", the
    three with bin M aside."""
    sizes = FAMILIES[fam]
    extra = [n for n in ASIDE if n in sizes] if fam == "mixed" else []
    return sorted({sizes[0], sizes[-1], *extra})
