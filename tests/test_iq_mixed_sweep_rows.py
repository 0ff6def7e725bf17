"""The rows and gates of tests/iq_mixed_sweep_rows.py without a GPU: for every one of the 91 sizes and every row type the reference
alone must stay inside the gates the GPU sweep holds the kernel to, or a kernel failure there would say nothing.

A float32 CPU library FFT (scipy.fft where SciPy imports, else numpy.fft) stands in for the kernel, a NumPy Blackman window rounded to
float32 for v: the windowed frames of the geometry, float32 fft against float64.  Every (size, row type) must be within the cap
2^-24 log2 n -- half the structured rows' gate -- and the worst figure per row type is printed.

Sensitivity: 1e-5 of a row's largest bin added to one bin of a structured row (an exact-bin tone or the last row) must fail that
row's gate at every size."""
import numpy as np

import iq_mixed_sweep_rows as Q

try:
    import scipy.fft as _fft
    LIBRARY = "scipy.fft"
except ImportError:                                                       # pragma: no cover
    _fft = np.fft
    LIBRARY = "numpy.fft"


def _figures(n):
    c = Q.forward_case(n)
    x = Q.forward_signals_iq(n)
    rows = Q.frames(x, np.blackman(c["L"]).astype(np.float32), c)
    assert rows.dtype == np.complex64 and rows.shape == (7, c["frames"], n)
    got, ref = _fft.fft(rows, axis=-1), np.fft.fft(rows.astype(np.complex128), axis=-1)
    got = got.astype(np.complex64) if LIBRARY == "numpy.fft" else got     # numpy.fft may widen
    assert got.dtype == np.complex64, "the library keeps single precision"
    return [Q.row_error(got[b], ref[b]) / Q.cap(n) for b in range(7)], ref


def test_geometry():
    assert len(Q.SIZES) == 91 and Q.SIZES[0] == 18 and Q.SIZES[-1] == 2025 and sum(n % 2 for n in Q.SIZES) == 18
    setups = set()
    for i, n in enumerate(Q.SIZES):
        c = Q.forward_case(n)
        even = i % 2 == 0
        assert c["B"] == 7 and c["B"] * c["frames"] >= 72 and c["hop"] == n // 4 + 1 and c["T"] == 4 * n + 7
        assert (c["L"], c["mode"], c["pad"]) == ((n, "reflect", n // 2) if even else (n - 3, None, 0))
        assert c["col0"] == (n - c["L"]) // 2 == (0 if even else 1)
        setups.add(c["setup"])
        x = Q.forward_signals_iq(n)
        assert x.dtype == np.complex64 and x.shape == (7, c["T"])
        if n % 2:                                                        # DC and bin (n - 1) / 2, nothing else, in a whole row of n samples
            spec = np.abs(np.fft.fft(x[6, :n].astype(np.complex128)))
            big = set(np.flatnonzero(spec > 1e-3 * spec.max()).tolist())
            assert big == {0, (n - 1) // 2}, (n, sorted(big))
    assert setups == {0, 1, 2, 3, 4}
    assert {n % 2 for i, n in enumerate(Q.SIZES) if i % 2 == 0} == {0, 1} and {n % 2 for i, n in enumerate(Q.SIZES) if i % 2} == {0, 1}


def test_the_float32_library_is_within_the_cap_on_every_size_and_row_type():
    fig = {n: _figures(n)[0] for n in Q.SIZES}
    worst = []
    for b, name in enumerate(Q.ROW_TYPES_IQ):
        n = max(fig, key=lambda m: fig[m][b])
        worst.append(fig[n][b])
        print(f"{LIBRARY} forward, I/Q mixed radix, {name}: worst {fig[n][b]:.3f} of 2^-24 log2 n at n_fft {n}")
    for n, per_row in fig.items():
        for b, e in enumerate(per_row):
            assert e <= 1.0, (n, Q.ROW_TYPES_IQ[b], e)
    assert max(worst) <= 1.0


def test_one_bin_off_by_1e_5_of_the_peak_fails_a_structured_row_at_every_size():
    """The exact-bin tones and the last row: the reference of the row with the most energy, one bin (off the peak) moved by 1e-5 of
    the largest bin, through the GPU sweep's own metric and gate."""
    least = {}
    for n in Q.SIZES:
        ref = _figures(n)[1]
        for b in range(2, 7):
            row = ref[b][np.argmax((np.abs(ref[b]) ** 2).sum(axis=-1))]
            peak = np.abs(row).max()
            bad = row.copy()
            bad[(int(np.argmax(np.abs(row))) + 2) % n] += 1e-5 * peak
            e = Q.row_error(bad[None, :], row[None, :])
            assert e > Q.gate(n, b), (n, b, e, Q.gate(n, b))
            least[b] = min(least.get(b, np.inf), e / Q.gate(n, b))
    for b in range(2, 7):
        print(f"I/Q mixed radix, {Q.ROW_TYPES_IQ[b]}: one bin off by 1e-5 of the peak is at least {least[b]:.1f} times the gate")
