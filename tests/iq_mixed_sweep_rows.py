"""The inputs and geometries of the I/Q mixed-radix size sweep: every n_fft bhw.stft_iq_mixed takes -- the 91 sizes 2^a 3^b 5^c in
16..2047 that are no power of two, 18 of them odd -- on the I/Q rows of tests/fft_sweep_rows.py: noise, impulses, exact-bin tones in
both halves of the spectrum and a DC-plus-Nyquist row.  Pure NumPy (no GPU, no torch), so tests/test_iq_mixed_sweep_rows.py (the
float32 CPU library against float64, no GPU) and tests/test_gpu_iq_mixed_size_sweep.py (the kernel) share them.  cap, frames,
row_error, forward_signals_iq and the gates are that file's, imported and not restated.

Geometry of size n at position i of SIZES: that file's forward geometry -- seven signals, hop n // 4 + 1, T = 4 n + 7; even i: L = n,
centred, reflect padding; odd i: L = n - 3, center=False, no detrending.  At least 72 rows everywhere.

An odd n has no Nyquist bin: there the last row is DC plus an exact-bin tone at (n - 1) / 2, the bin next to where it would be."""
import numpy as np

from blackman_harris_win_amd import binding as B

import fft_sweep_rows as R

SIZES = [n for n in range(B.CMFFT_MIN_N, B.CMFFT_MAX_N + 1) if B.cmfft_supported(n)]
assert len(SIZES) == 91, len(SIZES)
ROW_TYPES_IQ, NB_IQ = R.ROW_TYPES_IQ, R.NB_IQ
cap, gate, frames, row_error = R.cap, R.gate, R.frames, R.row_error


def forward_case(n):
    """The forward call of size n as a case of tests/stft_cmfft_cases.py (the keys its desc() and line() read), plus frames, col0, pad."""
    i = SIZES.index(n)
    even = i % 2 == 0
    L = n if even else n - 3
    hop, T = n // 4 + 1, 4 * n + 7
    pad = n // 2 if even else 0
    c = dict(id=f"n{n}", setup=R.setup_for(i, L), n_fft=n, L=L, hop=hop, mode="reflect" if even else None, detrend=False, B=NB_IQ, T=T,
             col0=(n - L) // 2, pad=pad, frames=1 + (T + 2 * pad - n) // hop)
    assert c["B"] * c["frames"] >= 72
    return c


def forward_signals_iq(n, T=None):
    """(7, T) complex64, T = 4 n + 7 unless given: ROW_TYPES_IQ in order (fft_sweep_rows.forward_signals_iq); at an odd n the last
    row is DC plus the exact-bin tone at (n - 1) / 2."""
    x = R.forward_signals_iq(n, T)
    if n % 2:
        ti = np.arange(x.shape[1])
        k0 = (n - 1) // 2
        x[6] = ((500.0 - 200.0j) + (1000.0 + 300.0j) * np.exp(2j * np.pi * ((k0 * ti) % n) / n)).astype(np.complex64)
    return x
