"""The grid, references and inputs of tests/spectral_front_cases.py without a GPU.

Restatements: every float64 restatement the GPU suite measures the fronts against is held to SciPy itself -- scipy.signal.welch,
spectrogram(mode="psd"), csd and coherence -- within 1e-12 of the largest value, on every case of the grid (odd nfft, both scalings,
both detrends, the default overlap and nfft, two-sided spectra of complex input); skipped where SciPy is absent.

Stand-in: a float32 CPU library FFT (scipy.fft where SciPy imports, else numpy.fft; both keep single precision) runs every case as a
float32 route does -- float32 segments, float32 window, binary64 sums -- and its figures are printed in units of
fft_sweep_rows.cap(nfft).  It must stay under the 64 caps the GPU suite allows its yardstick: that is what shows that these inputs keep
an honest float32 route inside the gates.  The window is SciPy's 4-term Blackman-Harris (spectral_front_cases.standin_window).

Coverage: every argument value meets every family, every (detrend, scaling) pair every size, every geometry every family; every front
of blackman_harris_win_amd.__all__ matching welch*, hold_fused*, cross_spectra*, csd*, coherence*, transfer_function* is called by some
family's cases and has its ResidentTable method (the descriptor-level calls welch_fft*, hold_fft*, csd_fft, welch_frames / welch_psd /
welch_csd have files of their own)."""
import fnmatch

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
import fft_sweep_rows as R
import spectral_front_cases as C

try:
    import scipy.fft as _fft
    LIBRARY = "scipy.fft"
except ImportError:                                                       # pragma: no cover
    _fft = np.fft
    LIBRARY = "numpy.fft"

YARDSTICK_CAPS = 64.0


def _close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (what, float(np.abs(got - want).max() / np.abs(want).max()))


@pytest.mark.parametrize("cid", C.case_ids())
def test_restatements_equal_scipy(cid):
    signal = pytest.importorskip("scipy.signal")
    c = C.case(cid)
    x, y = C.signals(c)
    v = C.standin_window(c["L"])
    ref = C.standin_references(cid)
    x64, v64 = x.astype(np.complex128 if c["iq"] else np.float64), v.astype(np.float64)
    kw = dict(window=v64, nfft=c["nfft_arg"], detrend=c["detrend"], scaling=c["scaling"], return_onesided=not c["iq"])
    shift = (lambda a, axis=-1: np.fft.fftshift(a, axes=axis)) if c["iq"] and c["fftshift"] else (lambda a, axis=-1: a)
    f, P = signal.welch(x64, c["fs"], noverlap=c["noverlap"], **kw)
    atol = 1e-15 * c["fs"] * c["nfft"]
    assert np.allclose(shift(f), ref["freqs"], rtol=0, atol=atol)
    _close(shift(P), ref["mean"], "welch")
    # spectrogram's own default overlap is nperseg // 8: welch's default is passed to it
    f, t, S = signal.spectrogram(x64, c["fs"], noverlap=c["L"] // 2 if c["noverlap"] is None else c["noverlap"], mode="psd", **kw)
    assert S.shape[-1] == c["F"] and np.allclose(shift(f), ref["freqs"], rtol=0, atol=atol)
    S = shift(S, axis=-2)
    _close(S.max(axis=-1), ref["max"], "max-hold")
    _close(S.min(axis=-1), ref["min"], "min-hold")
    _close(S.mean(axis=-1), ref["mean"], "mean of the spectrogram")
    worst = float(np.abs(P - S.mean(axis=-1) if not (c["iq"] and c["fftshift"]) else shift(P) - S.mean(axis=-1)).max() / P.max())
    if y is None:
        print(f"{cid}: welch, spectrogram max / min / mean equal scipy.signal's within 1e-12 (welch against spectrogram {worst:.1e})")
        return
    y64 = y.astype(np.float64)
    f, Pxy = signal.csd(x64, y64, c["fs"], noverlap=c["noverlap"], **kw)
    assert np.allclose(f, ref["freqs"], rtol=0, atol=atol)
    _close(Pxy, ref["cross"]["pxy"], "csd")
    _close(signal.welch(y64, c["fs"], noverlap=c["noverlap"], **kw)[1], ref["cross"]["pyy"], "welch of y")
    kw.pop("scaling"), kw.pop("return_onesided")
    _close(signal.coherence(x64, y64, c["fs"], noverlap=c["noverlap"], **kw)[1], ref["cross"]["coherence"], "coherence")
    _close(Pxy / P, ref["cross"]["h1"], "H1")
    print(f"{cid}: welch, spectrogram max / min / mean, csd, coherence, H1 equal scipy.signal's within 1e-12; least coherence "
          f"{float(ref['cross']['coherence'].min()):.3f}")


def standin_figures(c):
    """{quantity: (max, rms)} of the float32 CPU route of case c against the float64 references, as the GPU suite measures the fronts."""
    ref = C.standin_references(c["id"])
    got = C.float32_route(c, C.standin_window(c["L"]), _fft)
    fig = {"mean": C.rel(got["mean"], ref["mean"]), "max": C.hold_rel(got["max"], ref["max"], ref["mean"]),
           "min": C.hold_rel(got["min"], ref["min"], ref["mean"])}
    if "cross" in ref:
        for name, metric in C.CROSS_METRICS.items():
            if c["coherent"] or name not in ("pxy", "h1"):
                fig[name] = metric(got["cross"][name], ref["cross"][name])
    return fig


def test_float32_stand_in_stays_inside_the_yardsticks_allowance():
    worst = {}
    print(f"{LIBRARY} in float32 through every case, figures in units of 2^-24 log2 nfft (max, rms); window: 4-term Blackman-Harris")
    for c in C.CASES:
        fig = standin_figures(c)
        cap = C.cap(c)
        print(f"stand-in {c['id']}: " + ", ".join(f"{q} {m / cap:.2f} {r / cap:.2f}" for q, (m, r) in fig.items())
              + f"; min / median {C.standin_references(c['id'])['min_over_median']:.3f}")
        for q, (m, r) in fig.items():
            assert m <= YARDSTICK_CAPS * cap, (c["id"], q, m / cap)
            group = "hold" if q in ("max", "min") else q
            w = worst.setdefault(group, [0.0, 0.0, None])
            w[1] = max(w[1], r / cap)
            if m / cap > w[0]:
                w[0], w[2] = m / cap, c["id"]
    for group, (m, r, cid) in worst.items():
        print(f"stand-in worst {group}: max {m:.2f} caps (at {cid}), rms {r:.2f} caps")


def test_every_argument_value_meets_every_family_and_every_pair_every_size():
    for family in C.FAMILIES:
        cases = [c for c in C.CASES if c["family"] == family and not c["torch_only"]]
        assert {c["nfft"] for c in cases} == set(C.SIZES[family])
        assert {c["geometry"] for c in cases} == set(C.GEOMETRIES), family
        for key, values in (("scaling", ("density", "spectrum")), ("fs", C.FS), ("detrend", ("constant", False)), ("layout", C.LAYOUTS),
                            ("traces", C.TRACES), ("fftshift", (False, True))):
            assert {c[key] for c in cases} == set(values), (family, key)
        for n in C.SIZES[family]:
            mine = [c for c in cases if c["nfft"] == n]
            assert len(mine) >= 3 and {(c["detrend"], c["scaling"]) for c in mine} == set(C.PAIRS), (family, n)
            assert {c["traces"] for c in mine} == set(C.TRACES), (family, n)
        assert len({c["setup"] for c in cases}) >= 4, family
    by_geometry = {g: [c for c in C.CASES if c["geometry"] == g] for g in C.GEOMETRIES}
    assert all(c["nfft"] <= 64 for c in by_geometry["hop1"]) and all(c["nfft"] <= 512 for c in by_geometry["f259"])
    assert all(c["noverlap"] is None and c["nfft_arg"] is None for c in by_geometry["defaults"] + by_geometry["one"])
    assert all(c["L"] < c["nfft"] and c["L"] % 2 == 1 for c in by_geometry["padded"])
    assert all((c["T"] - c["L"]) % c["hop"] == c["hop"] - 1 for c in by_geometry["partial"])
    assert all(c["T"] == c["L"] and c["F"] == 1 for c in by_geometry["one"])
    assert all(c["F"] == 17 for c in by_geometry["f17"]) and all(c["F"] == 259 for c in by_geometry["f259"])
    assert all(c["F"] <= 40 for c in C.CASES if c["geometry"] != "f259")
    assert {c["setup"] for c in C.CASES} == {0, 1, 2, 3, 4}
    odd = C.case(C.ODD_TORCH_CASE)
    assert (odd["nfft"], odd["L"]) == (513, 401) and odd["torch_only"]
    real = [c for c in C.CASES if c["family"] == "real"]
    assert {(c["nfft"], c["geometry"]) for c in real if not c["coherent"]} == C.INCOHERENT
    assert {c["nfft"] for c in real if c["coherent"]} >= set(C.SIZES["real"])
    assert len({c["seed"] for c in C.CASES}) == len(C.CASES)


def test_every_scipy_shaped_front_is_called_and_has_its_table_method():
    patterns = ("welch*", "hold_fused*", "cross_spectra*", "csd*", "coherence*", "transfer_function*")
    descriptor_level = ("welch_fft*", "hold_fft*", "csd_fft*", "welch_frames", "welch_psd", "welch_csd", "welch_*_workspace_bytes")
    fronts = sorted(n for n in bhw.__all__ if any(fnmatch.fnmatch(n, p) for p in patterns)
                    and not any(fnmatch.fnmatch(n, p) for p in descriptor_level))
    called = {n for names in C.FRONTS.values() for n in names}
    assert set(fronts) == called, (sorted(set(fronts) - called), sorted(called - set(fronts)))
    for n in fronts:
        assert callable(getattr(bhw, n)) and callable(getattr(bhw.ResidentTable, n, None)), n
    assert set(C.FRONTS) == set(C.FAMILIES) and len(fronts) == 17
    print("fronts held to SciPy:", ", ".join(fronts))


def test_one_wrong_bin_is_far_outside_the_gates():
    """What the suite is after -- a doubling, a scale, a bin, a conjugate -- is at least 0.5 in these metrics and an overlap one sample
    off at least 0.1, against a float32 route's 1e-6: each on the reference of one case, through the suite's own metric.  Zero-padding
    around the segment instead of behind it is a linear phase: it cancels in |X|^2 and in conj(X) Y, so no output of these fronts can
    show it (the segments' own tests, bit for bit, are what holds it)."""
    c = C.case("real-n512-defaults")
    ref = C.standin_references(c["id"])
    x, y = C.signals(c)
    v = C.standin_window(c["L"])
    bad = ref["mean"].copy()
    bad[:, -1] *= 2.0                                                     # the Nyquist exception of the doubling dropped
    assert C.rel(bad, ref["mean"])[0] >= 0.99
    v64 = v.astype(np.float64)
    ratio = v64.sum() ** 2 / (v64 * v64).sum()                             # S1^2 and S2 swapped in welch_scale, either scaling
    assert C.rel(ref["mean"] * ratio, ref["mean"])[0] >= 0.5 and C.rel(ref["mean"] / ratio, ref["mean"])[0] >= 0.5
    other = dict(c, noverlap=c["L"] // 2 + 1, hop=c["L"] - c["L"] // 2 - 1, F=(c["T"] - c["L"] // 2 - 1) // (c["L"] - c["L"] // 2 - 1))
    assert C.rel(C.spectrogram_ref(x, v, other).mean(axis=-2), ref["mean"])[0] >= 0.1           # L // 2 + 1 as the default overlap
    assert C.rel(np.conj(ref["cross"]["pxy"]), ref["cross"]["pxy"])[0] >= 0.5                   # the other factor conjugated
    neighbour = np.roll(ref["mean"], 1, axis=-1)                                                # every bin read from its neighbour
    assert C.rel(neighbour, ref["mean"])[0] >= 0.5
    c = C.case("real-n64-padded")
    ref = C.standin_references(c["id"])
    x, y = C.signals(c)
    seg = x.astype(np.float64)[..., np.arange(c["F"])[:, None] * c["hop"] + np.arange(c["L"])[None, :]] * C.standin_window(c["L"])
    col0 = (c["nfft"] - c["L"]) // 2
    centred = np.zeros(seg.shape[:-1] + (c["nfft"],))
    centred[..., col0:col0 + c["L"]] = seg                                # the zero-padding centred, as stft does it
    X, Y = np.fft.rfft(centred, axis=-1), np.fft.rfft(seg, n=c["nfft"], axis=-1)
    assert np.abs(np.abs(X) - np.abs(Y)).max() <= 1e-9 * np.abs(Y).max()   # the POWER does not see it ...
    yc = np.zeros_like(centred)
    yseg = y.astype(np.float64)[..., np.arange(c["F"])[:, None] * c["hop"] + np.arange(c["L"])[None, :]] * C.standin_window(c["L"])
    yc[..., col0:col0 + c["L"]] = yseg
    pxy_c = (np.conj(X) * np.fft.rfft(yc, axis=-1)).mean(axis=-2)
    pxy = (np.conj(Y) * np.fft.rfft(yseg, n=c["nfft"], axis=-1)).mean(axis=-2)
    assert np.abs(pxy_c - pxy).max() <= 1e-9 * np.abs(pxy).max()           # ... nor do the cross spectra: the shift cancels in conj(X) Y
    assert R.cap(512) * YARDSTICK_CAPS < 1e-4
