"""The rows and gates of tests/fft_sweep_rows.py without a GPU: for every size and every row type the reference alone must stay inside
the gates the GPU sweep holds the kernels to, or a kernel failure there would say nothing.

A float32 CPU library FFT (scipy.fft where SciPy imports, else numpy.fft; both keep single precision) stands in for the kernel, a NumPy
Blackman window rounded to float32 for v.  Forward: the windowed frames of the geometry, float32 rfft / fft against float64.  Inverse:
irfft / ifft in float32, then window, overlap-add and envelope division in float64, against the same steps fed by a float64 transform.
Every (size, row type) must be within the cap 2^-24 log2 n -- half the structured rows' gate -- and the worst figure per row type is
printed.

Sensitivity: 1e-5 of a row's largest bin added to one bin of a structured row (an exact-bin tone or the DC-plus-Nyquist row) must fail
that row's gate at every size.  On a flat spectrum the same error is diluted by sqrt(K): it is the error noise rows let through at
large n_fft."""
import numpy as np
import pytest

import fft_sweep_rows as R

try:
    import scipy.fft as _fft
    LIBRARY = "scipy.fft"
except ImportError:                                                       # pragma: no cover
    _fft = np.fft
    LIBRARY = "numpy.fft"


def _window(L):
    return np.blackman(L).astype(np.float32)


def _forward_figures(n, iq):
    c = R.forward_case(n, iq)
    x = R.forward_signals_iq(n) if iq else R.forward_signals(n)
    rows = R.frames(x, _window(c["L"]), c)
    assert rows.dtype == (np.complex64 if iq else np.float32)
    if iq:
        got, ref = _fft.fft(rows, axis=-1), np.fft.fft(rows.astype(np.complex128), axis=-1)
    else:
        got, ref = _fft.rfft(rows, axis=-1), np.fft.rfft(rows.astype(np.float64), axis=-1)
    assert got.dtype == np.complex64, "the library keeps single precision"
    return [R.row_error(got[b], ref[b]) / R.cap(n) for b in range(x.shape[0])], ref


def _inverse_figures(n, iq):
    c = R.inverse_case(n, iq)
    Y = R.inverse_spectra_iq(n) if iq else R.inverse_spectra(n)
    v = _window(c["L"])
    if iq:
        got, ref = _fft.ifft(Y, axis=-1), np.fft.ifft(Y.astype(np.complex128), axis=-1)
        assert got.dtype == np.complex64, "the library keeps single precision"
    else:
        got, ref = _fft.irfft(Y, n=n, axis=-1), np.fft.irfft(Y.astype(np.complex128), n=n, axis=-1)
        assert got.dtype == np.float32, "the library keeps single precision"
    a = R.overlap_add64(got.astype(ref.dtype), v, c)
    b = R.overlap_add64(ref, v, c)
    return [R.signal_error(a[s], b[s]) / R.cap(n) for s in range(Y.shape[0])]


def _report(title, names, figures):
    """figures: {n: [figure per row type]} in units of the cap; prints the worst per row type and returns them."""
    worst = []
    for b, name in enumerate(names):
        n = max(figures, key=lambda m: figures[m][b])
        worst.append(figures[n][b])
        print(f"{LIBRARY} {title}, {name}: worst {figures[n][b]:.3f} of 2^-24 log2 n at n_fft {n}")
    return worst


@pytest.mark.parametrize("family,sizes,iq", [("mixed radix", R.SIZES, False), ("power of two, real", R.POW2_REAL, False),
                                             ("power of two, I/Q", R.POW2_IQ, True)], ids=["mixed", "pow2", "iq"])
def test_the_float32_library_is_within_the_cap_on_every_size_and_row_type(family, sizes, iq):
    names = R.ROW_TYPES_IQ if iq else R.ROW_TYPES
    fwd = {n: _forward_figures(n, iq)[0] for n in sizes}
    inv = {n: _inverse_figures(n, iq) for n in sizes}
    wf = _report(f"forward, {family}", names, fwd)
    wi = _report(f"inverse, {family}", names, inv)
    for fig in (fwd, inv):
        for n, per_row in fig.items():
            for b, e in enumerate(per_row):
                assert e <= 1.0, (family, n, names[b], e)
    assert max(wf + wi) <= 1.0


def test_geometry():
    assert R.SIZES[0] == 18 and R.SIZES[-1] == 4050 and 960 in R.SIZES and 1920 in R.SIZES
    assert R.POW2_REAL == [16, 32, 64, 128, 256, 512, 1024, 2048, 4096] and R.POW2_IQ == R.POW2_REAL[:-1]
    setups = set()
    for n in R.SIZES + R.POW2_REAL:
        c, ci = R.forward_case(n), R.inverse_case(n)
        even = R.index(n) % 2 == 0
        assert c["B"] * c["frames"] >= 72 and c["frames"] in ((15, 16) if even else (12, 13)), (n, c["frames"])
        assert (c["L"], c["mode"], c["col0"]) == ((n, "reflect", 0) if even else (n - 3, None, 1))
        assert (ci["L"], ci["normalize"], ci["F"], ci["B"]) == ((n, True, 12, 6) if even else (n - 3, False, 12, 6))
        assert c["hop"] == ci["hop"] == n // 4 + 1 and c["T"] == 4 * n + 7
        assert R.reached(ci).all()
        setups.add(c["setup"])
        Y = R.inverse_spectra(n)
        assert Y.dtype == np.complex64 and Y.shape == (6, 12, n // 2 + 1) and not Y.imag[..., 0].any() and not Y.imag[..., -1].any()
        x = R.forward_signals(n)
        assert x.dtype == np.float32 and x.shape == (6, c["T"])
        rows = R.frames(x[1:2], np.ones(c["L"], dtype=np.float32), c)[0]
        count = np.count_nonzero(rows, axis=-1)                          # one impulse a frame (and its mirror image in the padding)
        assert (count <= 2).all() and (count[2:-2] <= 1).all()
        cols = [int(np.flatnonzero(r)[0]) for r in rows if np.count_nonzero(r) == 1]
        assert len(set(cols)) >= 4 and all(a != b for a, b in zip(cols, cols[1:])), (n, cols)     # and its column moves
    assert setups == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("family,sizes,iq", [("mixed radix", R.SIZES, False), ("power of two, real", R.POW2_REAL, False),
                                             ("power of two, I/Q", R.POW2_IQ, True)], ids=["mixed", "pow2", "iq"])
def test_one_bin_off_by_1e_5_of_the_peak_fails_a_structured_row_at_every_size(family, sizes, iq):
    """The exact-bin tones and the DC-plus-Nyquist row: the reference of the row with the most energy, one bin (off the peak) moved by
    1e-5 of the largest bin, through the GPU sweep's own metric and gate."""
    structured = range(2, 7 if iq else 6)
    least = {}
    for n in sizes:
        ref = _forward_figures(n, iq)[1]
        for b in structured:
            row = ref[b][np.argmax((np.abs(ref[b]) ** 2).sum(axis=-1))]
            peak = np.abs(row).max()
            bad = row.copy()
            bad[(int(np.argmax(np.abs(row))) + 2) % row.shape[0]] += 1e-5 * peak
            e = R.row_error(bad[None, :], row[None, :])
            assert e > R.gate(n, b), (family, n, b, e, R.gate(n, b))
            least[b] = min(least.get(b, np.inf), e / R.gate(n, b))
    names = R.ROW_TYPES_IQ if iq else R.ROW_TYPES
    for b in structured:
        print(f"{family}, {names[b]}: one bin off by 1e-5 of the peak is at least {least[b]:.1f} times the gate")
