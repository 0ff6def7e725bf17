"""Every n_fft of bhw.istft_iq_mixed -- all 91 sizes 2^a 3^b 5^c in 16..2047 that are no power of two, 18 of them odd -- in one small
call each, on noise, an impulse, single bins at +1, -1, n / 2 - 1 and -(n / 4) (tones), and DC plus bin n // 2 (inverse_spectra
below).  In the mixed-radix kernel a size is not a shape: each n_fft has its own radix schedule, twiddle stride, (i, Ns) pairs of the
float-multiply `i mod Ns`, folded or full twiddle table, `cols` mask, bin turn and ring step.

The tones are the spectra of STATIONARY tones: bin k0 of frame f carries the phase 2 pi k0 f hop / n_fft the tone has at the frame's
start, so the overlapping frames add in phase, as the frames of a real signal do.  fft_sweep_rows.inverse_spectra_iq gives every
frame an arbitrary phase (0.3 + f radians); at hop n // 4 four such frames can cancel under the window, the reference shrinks and
the relative error measures that cancellation and not the transform: at n_fft 25 its tone at bin 11 put torch.fft.ifft +
istft_overlap_add at 2.28 of the cap, and the fused call at 2.31, next to 0.16 - 0.49 for the same bin at 27.  The no-GPU half holds
the conditioning of every structured signal (test_the_structured_signals_are_well_conditioned).

The impulse rows are not the all-ones spectrum: its impulse sits at column 0, where a Blackman-Harris window is about 1e-5 of its
middle, and the relative error of the output would measure the window and not the kernel.  They are fft_sweep_rows' impulses, whose
column moves from frame to frame inside the window's middle half (all bins of equal modulus, every twiddle with equal weight), for
the reason impulse_columns() gives.

Geometry of size n at position i of SIZES: 7 signals x 12 frames, hop n // 4, L = n, centred, torch.istft's default length; even i:
normalize=True, odd i: normalize=False.

Gates, the forward sweep's (tests/test_gpu_iq_mixed_size_sweep.py, fft_sweep_rows): the noise signal within the cap 2^-24 log2 n and
twice the error of bhw.istft_overlap_add(torch.fft.ifft(Y)) on the same GPU; structured signals within twice the cap.  The reference
is a float64 restatement: numpy.fft.ifft in complex128, the float32 window, the overlap-add and the division in float64.  Word for
word: library against table, the shifted call on shifted bins against the call on bins in order.

The no-GPU half (the tests without the gpu mark) holds the yardsticks themselves: a float32 inverse FFT of a CPU library in front of
the float64 overlap-add stays inside the structured gate at every size and row type, and 1e-5 of the peak added to one output of the
impulse signal fails that signal's gate at every size (a tone spreads over all T outputs and the per-signal metric dilutes one
output by sqrt(T): the smallest error caught there is printed and bounded)."""
import numpy as np
import pytest

import blackman_harris_win_amd as bhw

import fft_sweep_rows as R
import iq_mixed_sweep_rows as Q
import istft_cmfft_cases as XC
import plan_cases as PC

try:
    import scipy.fft as _fft
    LIBRARY = "scipy.fft"
except ImportError:                                                       # pragma: no cover
    _fft = np.fft
    LIBRARY = "numpy.fft"

F = R.F_INV


def inverse_case(n):
    """The inverse call of size n as a case of tests/istft_cmfft_cases.py (the keys its geometry(), desc() and line() read), plus col0,
    pad, t0 and T, the keys fft_sweep_rows.overlap_add64 and reached read."""
    i = Q.SIZES.index(n)
    hop, pad = n // 4, n // 2
    return dict(id=f"n{n}", setup=R.setup_for(i, n), n_fft=n, L=n, hop=hop, center=True, normalize=i % 2 == 0, B=R.NB_IQ, F=F, col0=0, pad=pad,
                t0=pad, T=n + hop * (F - 1) - 2 * pad)


def inverse_spectra(n):
    """(7, 12, n) complex64, bins in order: ROW_TYPES_IQ in order.  Noise and the impulses are fft_sweep_rows.inverse_spectra_iq's; the
    single bins (amplitude 100 + 3 f) and the DC + bin n // 2 row carry the phase of a stationary tone at hop n // 4."""
    hop = n // 4
    f = np.arange(F)
    Y = R.inverse_spectra_iq(n).astype(np.complex128)
    Y[2:] = 0.0

    def tone(k0):
        return np.exp(1j * (0.3 + 2.0 * np.pi * ((k0 * f * hop) % n) / n))

    for b, k0 in zip((2, 3, 4, 5), (1, n - 1, n // 2 - 1, n - n // 4)):
        Y[b, :, k0] = (100.0 + 3 * f) * tone(k0)
    Y[6, :, 0] = (50.0 + f) * (1 - 0.4j)
    Y[6, :, n // 2] = -(70.0 + f) * (1 + 0.3j) * tone(n // 2)
    return Y.astype(np.complex64)


def _ref64(Yh, v, c):
    return R.overlap_add64(np.fft.ifft(Yh.astype(np.complex128), axis=-1), v, c)


# ---- no GPU ------------------------------------------------------------------------------------------------------------------------

def _library_figures(n):
    """Per signal: the error of a float32 library ifft in front of the float64 overlap-add, in units of the cap; and the reference."""
    c = inverse_case(n)
    Yh = inverse_spectra(n)
    v = np.blackman(n).astype(np.float32)
    rows = _fft.ifft(Yh, axis=-1)
    rows = rows.astype(np.complex64) if LIBRARY == "numpy.fft" else rows      # numpy.fft may widen
    assert rows.dtype == np.complex64, "the library keeps single precision"
    ref = _ref64(Yh, v, c)
    got = R.overlap_add64(rows.astype(np.complex128), v, c).astype(np.complex64)
    return [R.signal_error(got[b], ref[b]) / R.cap(n) for b in range(c["B"])], ref


def test_geometry():
    assert len(Q.SIZES) == 91 and sum(n % 2 for n in Q.SIZES) == 18
    for i, n in enumerate(Q.SIZES):
        c = inverse_case(n)
        assert (c["B"], c["F"], c["hop"], c["L"], c["pad"], c["col0"]) == (7, 12, n // 4, n, n // 2, 0) and c["T"] == 11 * (n // 4) + n % 2
        assert XC.geometry(c)[4] == c["T"] and c["normalize"] == (i % 2 == 0)
        Y = inverse_spectra(n)
        assert Y.dtype == np.complex64 and Y.shape == (7, 12, n)
        assert np.allclose(np.abs(Y[1]), np.abs(Y[1][:, :1]), rtol=1e-6), "the impulse rows: every bin of equal modulus"
        for b, k0 in zip((2, 3, 4), (1, n - 1, n // 2 - 1)):
            assert set(np.flatnonzero(np.abs(Y[b]).sum(axis=0)).tolist()) == {k0}
    assert {n % 2 for i, n in enumerate(Q.SIZES) if i % 2 == 0} == {0, 1} and {n % 2 for i, n in enumerate(Q.SIZES) if i % 2} == {0, 1}


def test_the_float32_library_is_within_the_structured_gate_on_every_size_and_row_type():
    fig = {n: _library_figures(n)[0] for n in Q.SIZES}
    for b, name in enumerate(Q.ROW_TYPES_IQ):
        n = max(fig, key=lambda m: fig[m][b])
        print(f"{LIBRARY} inverse + float64 overlap-add, I/Q mixed radix, {name}: worst {fig[n][b]:.3f} of 2^-24 log2 n at n_fft {n}")
    for n, per_signal in fig.items():
        for b, e in enumerate(per_signal):
            assert e <= R.GATE_STRUCTURED, (n, Q.ROW_TYPES_IQ[b], e)
        assert per_signal[0] <= R.GATE_NOISE, (n, per_signal[0])


def test_the_structured_signals_are_well_conditioned():
    """The relative error of an overlap-added signal is the rows' relative error times kappa = sqrt(sum over f of |r_f v|^2) / |S|, S
    the (unnormalised) sum: frames that add in phase give kappa below 1, frames that cancel give any number.  Held below 1 for every
    tone and the DC row at every size; the impulses do not overlap their own peaks and sit at kappa 1."""
    worst = {}
    for n in Q.SIZES:
        c = dict(inverse_case(n), normalize=False)
        Yh = inverse_spectra(n)
        v = np.blackman(n).astype(np.float32)
        rows = np.fft.ifft(Yh.astype(np.complex128), axis=-1)
        S = R.overlap_add64(rows, v, c)
        for b in range(1, 7):
            # only the frames' parts that land inside the outputs count
            parts = 0.0
            for fr in range(F):
                lo, hi = max(fr * c["hop"], c["t0"]), min(fr * c["hop"] + n, c["t0"] + c["T"])
                if hi > lo:
                    seg = rows[b, fr, lo - fr * c["hop"]:hi - fr * c["hop"]] * v[lo - fr * c["hop"]:hi - fr * c["hop"]]
                    parts += float((np.abs(seg) ** 2).sum())
            kappa = np.sqrt(parts) / np.sqrt(float((np.abs(S[b]) ** 2).sum()))
            assert kappa <= 1.001, (n, Q.ROW_TYPES_IQ[b], kappa)
            worst[b] = max(worst.get(b, 0.0), kappa)
    for b in range(1, 7):
        print(f"I/Q mixed radix inverse, {Q.ROW_TYPES_IQ[b]}: kappa at most {worst[b]:.3f}")


def test_one_output_off_by_1e_5_of_the_peak_fails_the_impulse_signal_at_every_size():
    """The impulse signal keeps its energy in a dozen outputs, as an exact-bin tone keeps it in one bin of the forward sweep: 1e-5 of
    its peak added to one output (off the peak) fails the signal's gate at every size.  A tone or the DC row spreads its energy over
    all T = 11 (n // 4) outputs, so the per-signal l2 metric dilutes one output by sqrt(T): there the smallest single-output error the
    gate catches is printed as a share of the peak and held below 2e-4 (2 x 2^-24 log2 n x sqrt(T) < 1.4e-6 x 75)."""
    least, share = np.inf, {}
    for n in Q.SIZES:
        ref = _library_figures(n)[1]
        sig = ref[1]
        peak = np.abs(sig).max()
        bad = sig.copy()
        bad[(int(np.argmax(np.abs(sig))) + 2) % len(sig)] += 1e-5 * peak
        e = R.signal_error(bad, sig)
        assert e > R.gate(n, 1), (n, e, R.gate(n, 1))
        least = min(least, e / R.gate(n, 1))
        for b in range(2, 7):
            caught = R.gate(n, b) * np.sqrt((np.abs(ref[b]) ** 2).sum()) / np.abs(ref[b]).max()
            assert caught < 2e-4, (n, b, caught)
            share[b] = max(share.get(b, 0.0), caught)
    print(f"I/Q mixed radix inverse, impulse: one output off by 1e-5 of the peak is at least {least:.1f} times the gate")
    for b in range(2, 7):
        print(f"I/Q mixed radix inverse, {Q.ROW_TYPES_IQ[b]}: the gate catches one output off by {share[b]:.1e} of the peak at every size")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def tables(torch):
    held = {}

    def get(setup):
        if setup not in held:
            held[setup] = bhw.ResidentTable(PC.params(setup))
        return held[setup]

    yield get
    torch.cuda.synchronize()
    for t in held.values():
        t.close()


@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    for b, name in enumerate(Q.ROW_TYPES_IQ):
        if b in w:
            print(f"istft_iq_mixed over {w['sizes']} sizes, {name}: worst fused / cap {w[b][0]:.3f} at n_fft {w[b][1]}")
    if "noise ratio" in w:
        print(f"istft_iq_mixed over {w['sizes']} sizes, noise: worst fused / (ifft + istft_overlap_add) {w['noise ratio'][0]:.3f} at n_fft "
              f"{w['noise ratio'][1]}")


def _words(torch, t):
    return torch.view_as_real(t.contiguous()).cpu().numpy().view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("n", Q.SIZES)
def test_inverse_iq_mixed_every_size(torch, tables, worst, n):
    c = inverse_case(n)
    p, tab = PC.params(c["setup"]), tables(c["setup"])
    hop, T = c["hop"], c["T"]
    Yh = inverse_spectra(n)
    w = bhw.window(p, n).cpu().numpy()
    v = np.ldexp(w.astype(np.float32), -(p.dat_width - 1)).astype(np.float32)
    kw = dict(win_length=n, center=True, length=T, normalize=c["normalize"])
    ref = _ref64(Yh, v, c)
    Y = torch.from_numpy(Yh).cuda()
    two = bhw.istft_overlap_add(p, torch.fft.ifft(Y, dim=-1), n, hop, **kw).cpu().numpy()
    got = bhw.istft_iq_mixed(p, Y, n, hop, **kw)
    assert got.dtype == torch.complex64 and tuple(got.shape) == (c["B"], T)
    d = XC.parse(XC.line(c, table=tab._live()))
    assert d["table"] and "k_istft_cmfft_table" in d["kernels"] and d["rows"] == c["B"] * F, d["line"]
    assert np.array_equal(_words(torch, got), _words(torch, tab.istft_iq_mixed(p, Y, n, hop, **kw))), "library against table"
    Ys = torch.fft.fftshift(Y, dim=-1)
    for src in (bhw, tab):
        assert np.array_equal(_words(torch, src.istft_iq_mixed(p, Ys, n, hop, fftshift=True, **kw)), _words(torch, got)), "the shifted bins"
    assert not _words(torch, got)[:, ~R.reached(c)].any(), "outputs no frame reaches are +0.0"
    gh = got.cpu().numpy()
    figures = [(R.signal_error(gh[b], ref[b]), R.signal_error(two[b], ref[b])) for b in range(c["B"])]
    cap = R.cap(n)
    for b, (err, yd) in enumerate(figures):
        print(f"istft_iq_mixed n_fft {n}, {Q.ROW_TYPES_IQ[b]}: fused {err:.3e}, yardstick {yd:.3e}, ratio {err / yd if yd else float('nan'):.3f}, "
              f"cap {cap:.3e}, fused / cap {err / cap:.3f}")
        if err / cap > worst.get(b, (0.0, 0))[0]:
            worst[b] = (err / cap, n)
    worst["sizes"] = worst.get("sizes", 0) + 1
    if figures[0][0] / figures[0][1] > worst.get("noise ratio", (0.0, 0))[0]:
        worst["noise ratio"] = (figures[0][0] / figures[0][1], n)
    for b, (err, yd) in enumerate(figures):
        if b == 0:
            assert err <= 2.0 * yd, (n, Q.ROW_TYPES_IQ[b], err, yd)
        assert err <= Q.gate(n, b), (n, Q.ROW_TYPES_IQ[b], err, Q.gate(n, b))
