"""The grid, inputs, references and metrics of the differential suite that holds every SciPy-shaped spectral front (welch*, hold_fused*,
cross_spectra*, csd*, coherence*, transfer_function*, library and ResidentTable forms) to SciPy, bin by bin.  Pure NumPy (no GPU, no
torch, no SciPy), so tests/test_spectral_front_cases.py (the restatements against SciPy itself and a float32 CPU stand-in, no GPU) and
tests/test_gpu_spectral_fronts.py (the fronts) share them.

Why: the kernels are held word for word to the library's own rows, the fronts to the *_fft calls, detrending to the header's order.
Whatever the front and the header agree on -- the doubling rule at bins 0 and n/2, welch_scale, F = (T - noverlap) // hop, the default
overlap, zero-padding at the END of a segment, fs, the conjugation of Pxy -- is asked of nobody else, and the few end-to-end tests take
max |dP| / max P on a tone 80 dB above the noise, where a factor of two in one bin lies three orders of magnitude below the gate.  Here
the spectra are flat and the metrics are per bin, so no bin can hide behind a peak.

Families and sizes (nfft): SIZES.  The real and mixed sizes are one per regime of hold_real_cases.regime / welch_*_cases.shape plus both
ends of each range; 75 and 2025 are odd.  welch(fft="torch") additionally takes the odd nfft 513 with L = 401 (ODD_TORCH_CASE).

Geometries (GEOMETRIES; geometry() builds them), four per size by the table PLAN, every one in every family:
  defaults  L = nfft, noverlap=None, nfft=None, 9 segments (the real family: 40, as in padded, nov0 and partial; see Cross spectra)
  padded    L < nfft, L odd (nfft - 3, or nfft - 4 for an odd nfft), noverlap L // 3, 12 segments and one sample over: the zeros go at
            the END of the segment, as SciPy does, not around it as stft does
  nov0      noverlap=0, 8 segments
  hop1      noverlap = L - 1, 40 segments (nfft <= 64)
  partial   L = nfft - nfft // 4, noverlap L // 4, 10 segments and hop - 1 samples over: the partial segment is dropped
  one       T = L: one segment (nfft <= 96: one periodogram of noise has exponentially distributed bins, and among thousands of them
            one is always nearly empty)
  f17       17 segments: one chunk of 16 and one more
  f259      259 segments at hop nfft // 8: one block of 256 and three more (nfft <= 512, so that T stays small)

Arguments: the four pairs PAIRS of (detrend, scaling) meet every size (one geometry each, rotated by the size's position); fs, the
layout of x (1-D, (3, T) contiguous, (3, T) as a row-strided view of a wider buffer), fftshift and traces rotate with the case's
position in its family, each on a period of its own.  Parameter sets: plan_cases.SETUPS by fft_sweep_rows.setup_for.

Inputs: seeded white noise of amplitude 1000 and NO tone; with detrend="constant" an offset of 250 (with detrend=False none: the window
would carry it into the low bins and the per-bin metric would measure leakage).  I/Q: independent real and imaginary parts (offset
250 - 90j).  Cross spectra: y[t] = 0.7 x[t-3] - 0.2 x[t-1] + 0.3 w[t], w independent: the true coherence is at least 0.73 in every bin
and |H| lies in [0.5, 0.9].  That is the coherence of the process; the ESTIMATE of F segments scatters around it by about
(1 - C) sqrt(2 C / F), so among the thousands of bins of nfft 4096 some bin of 17 segments falls below 0.5 at every seed, and a window
of 16 or 64 coefficients whose weight sits on a few samples loses y's three-sample delay altogether (a coherence near 0).  The real
family therefore has 40 segments where the geometry leaves the number free, and the six cases of INCOHERENT, where no seed can meet the
condition, are not `coherent`: their Pxx, Pyy and coherence (an absolute metric) are still gated, their Pxy and H1 -- relative to a
reference near zero -- are not.

References, float64 / complex128, the window passed in as an array: spectrogram_ref (scipy.signal.spectrogram(mode="psd"), and its
mean = scipy.signal.welch, max, min over the segments), cross_ref (scipy.signal.csd, coherence, H1 = Pxy / Pxx), freqs_ref.

Metrics (maximum and RMS over all bins and signals): rel |got - ref| / |ref| (mean PSD, Pxx, Pyy, Pxy, H1); hold_rel |got - ref| / mean
(the traces: a min-hold bin can be legitimately tiny, and a float32 FFT's error scales with the row, not the bin); absolute (coherence).

Conditions, asserted by references() on whatever window it is given so that no case is silently weak: every bin enters every metric
(shapes are compared, figures must be finite); min ref >= 0.02 median ref over the bins of every signal's mean PSD; the reference
coherence is at least 0.5 in every bin of every coherent case.  A case that misses one gets another seed (RESEED), never another condition.
"""
import functools

import numpy as np

import fft_sweep_rows as R

NB = 3
FAMILIES = ("real", "mixed", "iq", "iq_mixed")
SIZES = {"real": (16, 64, 512, 4096), "mixed": (18, 96, 400, 1536, 4050), "iq": (16, 64, 512, 2048), "iq_mixed": (18, 75, 400, 2025)}
GEOMETRIES = ("defaults", "padded", "nov0", "hop1", "partial", "one", "f17", "f259")
PLAN = {
    "real": {16: ("defaults", "hop1", "f259", "one"), 64: ("padded", "hop1", "f17", "partial"),
             512: ("nov0", "f259", "defaults", "padded"), 4096: ("partial", "f17", "nov0", "defaults")},
    "mixed": {18: ("hop1", "f259", "padded", "one"), 96: ("defaults", "f17", "nov0", "one"), 400: ("f259", "padded", "partial", "defaults"),
              1536: ("nov0", "partial", "f17", "defaults"), 4050: ("padded", "partial", "f17", "nov0")},
    "iq": {16: ("hop1", "defaults", "f259", "partial"), 64: ("hop1", "padded", "one", "f17"),
           512: ("f259", "nov0", "defaults", "padded"), 2048: ("partial", "f17", "nov0", "defaults")},
    "iq_mixed": {18: ("hop1", "f259", "defaults", "one"), 75: ("padded", "f17", "nov0", "partial"),
                 400: ("f259", "partial", "padded", "defaults"), 2025: ("nov0", "partial", "f17", "padded")},
}
# the fronts each family's cases call, by their names in blackman_harris_win_amd.__all__ (and on ResidentTable); the fused cross spectra
# take nfft up to CSD_FUSED_MAX_N, and welch / cross_spectra / csd / coherence / transfer_function run as fft="torch" and fft="fused"
FRONTS = {
    "real": ("welch", "welch_fused", "hold_fused", "cross_spectra", "csd", "coherence", "transfer_function", "cross_spectra_fused",
             "csd_fused", "coherence_fused", "transfer_function_fused"),
    "mixed": ("welch_fused_mixed", "hold_fused_mixed"),
    "iq": ("welch", "welch_fused_iq", "hold_fused_iq"),
    "iq_mixed": ("welch_fused_iq_mixed", "hold_fused_iq_mixed"),
}
CSD_FUSED_MAX_N = 2048
PAIRS = (("constant", "density"), (False, "spectrum"), ("constant", "spectrum"), (False, "density"))
FS = (1.0, 48000.0)
LAYOUTS = ("1d", "rows", "strided")
TRACES = ("both", "max", "min")
STRIDE_GAP = 5                            # the strided layout: rows of a (3, T + 5) buffer
MIN_OVER_MEDIAN, MIN_COHERENCE = 0.02, 0.5
# the real cases whose reference coherence no seed lifts to MIN_COHERENCE in every bin (see "Cross spectra" in the module docstring)
INCOHERENT = {(16, "defaults"), (16, "hop1"), (16, "f259"), (64, "hop1"), (64, "partial"), (4096, "f17")}
# case id -> the seed's offset, where offset 0 missed a condition (found with the stand-in window and the library's own float32 window
# of the case's parameter set, at 0.03 of the median and a coherence of 0.53)
RESEED = {'real-n16-one': 1, 'real-n64-f17': 5, 'real-n512-nov0': 1, 'real-n4096-partial': 2, 'real-n4096-nov0': 1, 'real-n4096-defaults': 1,
          'mixed-n18-one': 13, 'mixed-n96-one': 220, 'iq-n64-one': 1647, 'iq_mixed-n18-one': 50}


def geometry(name, n, many=False):
    """(L, noverlap or None, nfft argument or None, T, F) of geometry `name` at nfft n; many: 40 segments where the geometry leaves the
    number free (the real family: the coherence of few segments dips below MIN_COHERENCE in some bin of thousands)."""
    over = 0
    if name == "defaults":
        L, nov, arg, F = n, None, None, 40 if many else 9
    elif name == "padded":
        L = n - 3 if n % 2 == 0 else n - 4
        nov, arg, F, over = L // 3, n, 40 if many else 12, 1
    elif name == "nov0":
        L, nov, arg, F = n, 0, n, 40 if many else 8
    elif name == "hop1":
        L, nov, arg, F = n, n - 1, None, 40
    elif name == "partial":
        L = n - n // 4
        nov, arg, F = L // 4, n, 40 if many else 10
        over = L - nov - 1
    elif name == "one":
        L, nov, arg, F = n, None, None, 1
    elif name == "f17":
        L, nov, arg, F = n, n // 2, n, 17
    elif name == "f259":
        L, nov, arg, F = n, n - max(1, n // 8), n, 259
    else:
        raise ValueError(name)
    hop = L - (L // 2 if nov is None else nov)
    T = L + (F - 1) * hop + over
    assert over < hop and F == (T - (L - hop)) // hop
    return L, nov, arg, T, F


def _cases():
    out = []
    for family in FAMILIES:
        pos = 0
        for j, n in enumerate(SIZES[family]):
            for g, name in enumerate(PLAN[family][n]):
                L, nov, arg, T, F = geometry(name, n, family == "real")
                detrend, scaling = PAIRS[(g + j) % 4]
                out.append(dict(id=f"{family}-n{n}-{name}", family=family, nfft=n, geometry=name, L=L, noverlap=nov, nfft_arg=arg, T=T, F=F,
                                hop=L - (L // 2 if nov is None else nov), detrend=detrend, scaling=scaling, fs=FS[pos % 2],
                                layout=LAYOUTS[pos % 3], fftshift=bool((pos // 2) % 2), traces=TRACES[(pos + pos // 4) % 3],
                                setup=R.setup_for(pos + j, L), iq=family.startswith("iq"), pos=pos, torch_only=False,
                                coherent=family == "real" and (n, name) not in INCOHERENT))
                pos += 1
    # the odd nfft that only the torch.fft route of welch / cross_spectra takes
    out.append(dict(id="real-n513-padded-torch", family="real", nfft=513, geometry="padded", L=401, noverlap=100, nfft_arg=513,
                    T=401 + 39 * 301 + 1, F=40, hop=301, detrend="constant", scaling="spectrum", fs=48000.0, layout="rows", fftshift=False,
                    traces="both", setup=0, iq=False, pos=16, torch_only=True, coherent=True))
    for k, c in enumerate(out):
        c["seed"] = 7000 + 10000 * k + RESEED.get(c["id"], 0)
    return out


CASES = _cases()
ODD_TORCH_CASE = "real-n513-padded-torch"


def case_ids(family=None, fused_only=False):
    return [c["id"] for c in CASES if family in (None, c["family"]) and not (fused_only and c["torch_only"])]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)


def kwargs(c):
    """The keyword arguments of the fronts for case c: noverlap and nfft only where the geometry passes them."""
    kw = dict(length=c["L"], detrend=c["detrend"], scaling=c["scaling"])
    if c["noverlap"] is not None:
        kw["noverlap"] = c["noverlap"]
    if c["nfft_arg"] is not None:
        kw["nfft"] = c["nfft_arg"]
    return kw


def standin_window(L):
    """SciPy's periodic 4-term Blackman-Harris window in float32: the stand-in of the CPU tests for bhw.window(p, L, dtype=float32)."""
    t = 2.0 * np.pi * np.arange(L) / L
    return (0.35875 - 0.48829 * np.cos(t) + 0.14128 * np.cos(2 * t) - 0.01168 * np.cos(3 * t)).astype(np.float32)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------

def signals(c):
    """(x, y): x (3, T) float32 or complex64; y (3, T) float32 for the real family (the cross spectra's response), else None."""
    rng = np.random.default_rng(c["seed"])
    T = c["T"]
    if c["iq"]:
        x = (rng.standard_normal((NB, T)) + 1j * rng.standard_normal((NB, T))) * 1000.0
        if c["detrend"]:
            x = x + (250.0 - 90.0j)
        return x.astype(np.complex64), None
    e = rng.standard_normal((NB, T + 3)) * 1000.0
    offset = 250.0 if c["detrend"] else 0.0
    x = (e[:, 3:] + offset).astype(np.float32)
    if c["family"] != "real":
        return x, None
    w = rng.standard_normal((NB, T)) * 1000.0
    y = 0.7 * e[:, :T] - 0.2 * e[:, 2:T + 2] + 0.3 * w + offset
    return x, y.astype(np.float32)


def strided(x):
    """x (3, T) as rows of a wider (3, T + STRIDE_GAP) buffer whose gaps hold a value no sum should meet."""
    buf = np.full((x.shape[0], x.shape[1] + STRIDE_GAP), 1e30, dtype=x.dtype)
    buf[:, :x.shape[1]] = x
    return buf


# ---- the restatements of SciPy, float64 / complex128 ---------------------------------------------------------------------------------------

def freqs_ref(c):
    """scipy's frequency axis: rfftfreq(nfft, 1 / fs) for real input, fftfreq for I/Q (fftshift of it where the case shifts)."""
    n, d = c["nfft"], 1.0 / c["fs"]
    if not c["iq"]:
        return np.arange(n // 2 + 1) / (n * d)
    k = np.arange(n)
    k[(n + 1) // 2:] -= n                                                 # 0 .. ceil(n / 2) - 1, then -floor(n / 2) .. -1
    f = k / (n * d)
    return np.fft.fftshift(f) if c["fftshift"] else f


def _segments(x, c):
    """(B, F, L) float64 / complex128: scipy's segments, the partial one dropped, each with its mean removed where the case detrends."""
    x = np.asarray(x, dtype=np.complex128 if np.iscomplexobj(x) else np.float64)
    L, hop = c["L"], c["hop"]
    F = (x.shape[-1] - (L - hop)) // hop
    assert F == c["F"]
    seg = x[..., np.arange(F)[:, None] * hop + np.arange(L)[None, :]]
    if c["detrend"]:
        seg = seg - seg.mean(axis=-1, keepdims=True)
    return seg


def _scale(v, c):
    v = np.asarray(v, dtype=np.float64)
    return 1.0 / (c["fs"] * (v * v).sum()) if c["scaling"] == "density" else 1.0 / v.sum() ** 2


def _double(P, n):
    """The one-sided rule: every bin doubled but 0 and, for an even nfft, n / 2."""
    P[..., 1:] *= 2.0
    if n % 2 == 0:
        P[..., -1] /= 2.0
    return P


def _spectra(x, v, c):
    seg = _segments(x, c) * np.asarray(v, dtype=np.float64)
    n = c["nfft"]
    return np.fft.fft(seg, n=n, axis=-1) if np.iscomplexobj(seg) else np.fft.rfft(seg, n=n, axis=-1)     # n > L: zeros at the end


def spectrogram_ref(x, v, c):
    """scipy.signal.spectrogram(x, fs, window=v, noverlap=.., nfft=.., detrend=.., scaling=.., mode="psd") with the time axis last but
    one: (B, F, K) float64, one-sided for real x, two-sided for I/Q (bins shifted where the case shifts)."""
    Y = _spectra(x, v, c)
    S = (Y.real ** 2 + Y.imag ** 2) * _scale(v, c)
    if not np.iscomplexobj(x):
        return _double(S, c["nfft"])
    return np.fft.fftshift(S, axes=-1) if c["fftshift"] else S


def cross_ref(x, y, v, c):
    """scipy.signal.csd(x, y) = mean conj(X) Y, welch of x and of y, scipy.signal.coherence and H1 = Pxy / Pxx: a dict by output name."""
    X, Y = _spectra(x, v, c), _spectra(y, v, c)
    s, n = _scale(v, c), c["nfft"]
    pxy = _double((np.conj(X) * Y).mean(axis=-2) * s, n)
    pxx = _double((X.real ** 2 + X.imag ** 2).mean(axis=-2) * s, n)
    pyy = _double((Y.real ** 2 + Y.imag ** 2).mean(axis=-2) * s, n)
    return {"pxy": pxy, "pxx": pxx, "pyy": pyy, "coherence": np.abs(pxy) ** 2 / (pxx * pyy), "h1": pxy / pxx}


def references(c, v, x=None, y=None):
    """Every reference of case c for the window v (float32 array of L): a dict with freqs, mean, max, min (B, K) and, for the real
    family, cross (cross_ref's dict).  Asserts the conditions of the module docstring."""
    if x is None:
        x, y = signals(c)
    assert len(v) == c["L"] and x.shape == (NB, c["T"])
    S = spectrogram_ref(x, v, c)
    ref = {"freqs": freqs_ref(c), "mean": S.mean(axis=-2), "max": S.max(axis=-2), "min": S.min(axis=-2)}
    K = c["nfft"] if c["iq"] else c["nfft"] // 2 + 1
    assert S.shape == (NB, c["F"], K) and ref["freqs"].shape == (K,)
    ratio = float((ref["mean"].min(axis=-1) / np.median(ref["mean"], axis=-1)).min())
    assert ratio >= MIN_OVER_MEDIAN, f"{c['id']}: min / median of the reference mean PSD is {ratio:.4f}: give the case another seed (RESEED)"
    ref["min_over_median"] = ratio
    if y is not None:
        ref["cross"] = cross_ref(x, y, v, c)
        coh = float(ref["cross"]["coherence"].min())
        assert not c["coherent"] or coh >= MIN_COHERENCE, f"{c['id']}: the reference coherence falls to {coh:.3f}: give the case another seed (RESEED)"
        assert np.abs(ref["cross"]["pxx"] - ref["mean"]).max() <= 1e-12 * ref["mean"].max()
    return ref


# ---- a float32 route in NumPy: float32 segments, float32 window, the library FFT in single precision, binary64 sums ---------------------------

def float32_route(c, v, fft, x=None, y=None):
    """The figures' other side on the CPU: references()'s keys from float32 segments (the mean a binary64 sum rounded to float32, then a
    float32 subtraction), times the float32 window, through `fft` (a module with rfft / fft that keep single precision: scipy.fft or
    numpy.fft), |Y|^2 and every sum over the segments in binary64."""
    if x is None:
        x, y = signals(c)
    v = np.asarray(v, dtype=np.float32)
    L, hop, n, F = c["L"], c["hop"], c["nfft"], c["F"]
    idx = np.arange(F)[:, None] * hop + np.arange(L)[None, :]

    def spectra(t):
        seg = t[..., idx]
        if c["detrend"]:
            seg = seg - seg.mean(axis=-1, keepdims=True, dtype=np.complex128 if c["iq"] else np.float64).astype(seg.dtype)
        seg = seg * v
        assert seg.dtype == t.dtype
        Y = (fft.fft if c["iq"] else fft.rfft)(seg, n=n, axis=-1)
        assert Y.dtype == np.complex64, "the library keeps single precision"
        return Y.astype(np.complex128)

    s = _scale(v, c)
    X = spectra(x)
    S = (X.real ** 2 + X.imag ** 2) * s
    S = (np.fft.fftshift(S, axes=-1) if c["fftshift"] else S) if c["iq"] else _double(S, n)
    out = {"mean": S.mean(axis=-2), "max": S.max(axis=-2), "min": S.min(axis=-2)}
    if y is not None:
        Y = spectra(y)
        pxy = _double((np.conj(X) * Y).mean(axis=-2) * s, n)
        pyy = _double((Y.real ** 2 + Y.imag ** 2).mean(axis=-2) * s, n)
        out["cross"] = {"pxy": pxy, "pxx": out["mean"], "pyy": pyy, "coherence": np.abs(pxy) ** 2 / (out["mean"] * pyy), "h1": pxy / out["mean"]}
    return out


# ---- metrics: (maximum, RMS) over every bin of every signal -----------------------------------------------------------------------------------

def _figures(e, ref):
    assert e.shape == ref.shape and e.ndim == 2 and e.shape[0] == NB, (e.shape, ref.shape)     # no bin and no signal is left out
    assert np.isfinite(e).all()
    return float(e.max()), float(np.sqrt((e * e).mean()))


def _as(got, ref):
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return got.astype(ref.dtype)


def rel(got, ref):
    """e = |got - ref| / |ref| per bin: the mean PSD, Pxx, Pyy, and (complex) Pxy and H1."""
    return _figures(np.abs(_as(got, ref) - ref) / np.abs(ref), ref)


def hold_rel(got, ref, mean):
    """e = |got - ref| / mean per bin, mean the reference MEAN PSD of that bin: the max-hold and min-hold traces."""
    return _figures(np.abs(_as(got, ref) - ref) / mean, ref)


def absolute(got, ref):
    """e = |got - ref| per bin: the coherence."""
    return _figures(np.abs(_as(got, ref) - ref), ref)


CROSS_METRICS = {"pxy": rel, "pxx": rel, "pyy": rel, "h1": rel, "coherence": absolute}


def edge_bins(c):
    """The bins of a one-sided spectrum that are not doubled: 0 and, for an even nfft, nfft / 2."""
    return [0, c["nfft"] // 2] if c["nfft"] % 2 == 0 else [0]


def cap(c):
    return R.cap(c["nfft"])


@functools.lru_cache(maxsize=None)
def standin_references(cid):
    """references() of case `cid` for the stand-in window: what the CPU tests share."""
    c = case(cid)
    return references(c, standin_window(c["L"]))
