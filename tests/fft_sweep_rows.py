"""The inputs and geometries of the FFT size sweep: every n_fft the fused FFT kernels take, on noise, impulses, exact-bin tones and a
DC-plus-Nyquist row.  Pure NumPy (no GPU, no torch), so tests/test_fft_sweep_rows.py (the float32 CPU library against float64, no GPU),
tests/test_gpu_fft_size_sweep.py (the kernels) and tools/sweep_fft_sizes.py (the record) share them.

Why these rows: the accuracy gates of the FFT families run on white noise plus two tones and an offset and take the relative l2 error of a
row.  On a flat spectrum one wrong bin is diluted by sqrt(K).  On an impulse every twiddle carries equal weight, on an exact-bin tone and
on the DC-plus-Nyquist row the energy sits in one or two bins (a few more under the window's main lobe), so the same metric sees a single
wrong bin near 1e-7 of the peak.

Why every size: in the mixed-radix kernels a size is not a shape -- each n_fft has its own radix schedule, twiddle stride, (i, Ns) pairs
of the float-multiply `i mod Ns`, odd or even M, `cols` mask and ring step.

Sizes.  SIZES: the 95 n_fft of bhw.stft_mixed / istft_mixed (binding.mfft_supported); the index of a size is its position in the sorted
list.  POW2_REAL (bhw.stft / istft) and POW2_IQ (bhw.stft_iq / istft_iq) likewise, indexed by their own position.

Forward geometry of size n, index i: hop n // 4 + 1, T = 4 n + 7, six signals (seven for I/Q); even i: L = n, centred, reflect padding
(15 or 16 frames); odd i: L = n - 3 (odd, col0 = 1), center=False, no detrending (12 or 13 frames).  At least 72 rows everywhere: more
than the 64 rows a workgroup holds at the smallest sizes, so a second, ragged group exists at every size.

Inverse geometry: hop n // 4 + 1, F = 12, centred, torch.istft's default length; even i: L = n, normalize=True; odd i: L = n - 3,
normalize=False.

Parameter sets: plan_cases.SETUPS[i mod 5]; where that set's phase width does not hold L (a window has at most 2^phi_width
coefficients), the next of the five that does.

The gates (GATE_NOISE, GATE_STRUCTURED, in units of cap(n) = 2^-24 log2 n): noise rows keep the project's gate -- the cap, and twice the
yardstick's error on the same GPU.  Structured rows: twice the cap.  A float32 library FFT on the CPU reaches 0.69 of the cap on the
inverse single-bin rows (tests/test_fft_sweep_rows.py prints it), the fused inverse adds one float32 multiply by fl32(1 / n_fft) and has
measured up to 1.34 times the library's figure on noise, so a factor of two over the cap is the margin an honest kernel needs; any
indexing error is three orders of magnitude above it.
"""
import math

import numpy as np

from blackman_harris_win_amd import binding as B

import plan_cases as PC

SIZES = [n for n in range(B.MFFT_MIN_N, B.MFFT_MAX_N + 1) if B.mfft_supported(n)]
assert len(SIZES) == 95, len(SIZES)
POW2_REAL = [1 << e for e in range(4, 13)]                                # 16..4096
POW2_IQ = [1 << e for e in range(4, 12)]                                  # 16..2048
NB, NB_IQ, F_INV = 6, 7, 12

ROW_TYPES = ("noise", "impulse", "tone k0 = 1", "tone k0 = M // 2", "tone k0 = M - 1", "DC + Nyquist")
ROW_TYPES_IQ = ("noise", "impulse", "tone +1", "tone -1", "tone +(n / 2 - 1)", "tone -(n / 4)", "DC + Nyquist")
GATE_NOISE, GATE_STRUCTURED = 1.0, 2.0


def cap(n):
    return 2.0 ** -24 * math.log2(n)


def gate(n, row):
    """The absolute bound of row type `row` (its position in ROW_TYPES / ROW_TYPES_IQ) at n_fft n."""
    return (GATE_NOISE if row == 0 else GATE_STRUCTURED) * cap(n)


def index(n):
    for sizes in (SIZES, POW2_REAL):
        if n in sizes:
            return sizes.index(n)
    raise ValueError(n)


def setup_for(i, L):
    """plan_cases.SETUPS[i mod 5], or the next of the five whose 2^phi_width holds a window of L."""
    for k in range(5):
        s = (i + k) % 5
        if L <= 1 << PC.SETUPS[s][1]:
            return s
    raise ValueError(L)


def tone_bins(n):
    M = n // 2
    return (1, M // 2, M - 1)


# ---- geometry ----------------------------------------------------------------------------------------------------------------------

def forward_case(n, iq=False):
    """The forward call of size n as a case of tests/stft_mfft_cases.py (the keys its desc() and line() read), plus frames, col0, pad."""
    i = index(n)
    even = i % 2 == 0
    L = n if even else n - 3
    hop, T = n // 4 + 1, 4 * n + 7
    pad = n // 2 if even else 0
    c = dict(id=f"n{n}", setup=setup_for(i, L), n_fft=n, L=L, hop=hop, mode="reflect" if even else None, detrend=False, B=NB_IQ if iq else NB, T=T,
             col0=(n - L) // 2, pad=pad, frames=1 + (T + 2 * pad - n) // hop)
    assert c["B"] * c["frames"] >= 72 and (even or (L % 2 == 1 and c["col0"] == 1))
    return c


def inverse_case(n, iq=False):
    """The inverse call of size n as a case of tests/istft_mfft_cases.py (the keys its geometry(), desc() and line() read), plus col0,
    pad, t0 (the outputs start t0 columns into frame 0) and T, torch.istft's default length."""
    i = index(n)
    even = i % 2 == 0
    L = n if even else n - 3
    hop = n // 4 + 1
    pad, col0 = n // 2, (n - L) // 2
    return dict(id=f"n{n}", setup=setup_for(i, L), n_fft=n, L=L, hop=hop, center=True, normalize=even, B=NB_IQ if iq else NB, F=F_INV,
                col0=col0, pad=pad, t0=pad - col0, T=n + hop * (F_INV - 1) - 2 * pad)


# ---- forward signals ---------------------------------------------------------------------------------------------------------------

def forward_signals(n, T=None):
    """(6, T) float32, T = 4 n + 7 unless given: ROW_TYPES in order."""
    T = 4 * n + 7 if T is None else int(T)
    t = np.arange(T, dtype=np.float64)
    rng = np.random.default_rng(1000 + n)
    x = np.zeros((NB, T))
    x[0] = rng.standard_normal(T) * 1000 + 1e3 * np.cos(2 * np.pi * 0.1234 * t) + 1e-3 * np.cos(2 * np.pi * 0.31 * t + 1.0) + 250.0
    x[1, 3::n + 1] = 1000.0                                              # the impulse's column moves from frame to frame
    for b, k0 in zip((2, 3, 4), tone_bins(n)):
        x[b] = 1000.0 * np.cos(2 * np.pi * ((k0 * np.arange(T)) % n) / n + 0.3)      # the phase reduced in integers: exact-bin
    x[5] = 500.0 + 1000.0 * (1 - 2 * (np.arange(T) % 2))
    return x.astype(np.float32)


def forward_signals_iq(n, T=None):
    """(7, T) complex64, T = 4 n + 7 unless given: ROW_TYPES_IQ in order.  The tones at +k0 and -k0 land in the two halves fftshift
    swaps."""
    T = 4 * n + 7 if T is None else int(T)
    ti = np.arange(T)
    t = ti.astype(np.float64)
    rng = np.random.default_rng(2000 + n)
    x = np.zeros((NB_IQ, T), dtype=np.complex128)
    x[0] = (rng.standard_normal(T) + 1j * rng.standard_normal(T)) * 1000 + 1e3 * np.exp(2j * np.pi * 0.1234 * t) \
        + 1e-3 * np.exp(-2j * np.pi * 0.31 * t + 1.0j) + (250.0 - 90.0j)
    x[1, 3::n + 1] = 1000.0 - 600.0j
    for b, k0 in zip((2, 3, 4, 5), (1, -1, n // 2 - 1, -(n // 4))):
        x[b] = 1000.0 * np.exp(2j * np.pi * ((k0 * ti) % n) / n + 0.3j)
    x[6] = (500.0 - 200.0j) + (1000.0 + 300.0j) * (1 - 2 * (ti % 2))
    return x.astype(np.complex64)


# ---- inverse spectra ---------------------------------------------------------------------------------------------------------------

def impulse_columns(n):
    """j_f of the impulse spectra: inside the window's middle half.  At the edge of a Blackman-Harris window the reference output is
    about 1e-5 of the error floor under the rest of the window, and the relative error would measure the window, not the kernel."""
    j = n // 4 + (7 * np.arange(F_INV) + 1) % (n // 2)
    assert (j >= n // 4).all() and (j < n // 4 + n // 2).all()
    return j


def inverse_spectra(n):
    """(6, 12, M + 1) complex64: ROW_TYPES in order.  Bins 0 and M are purely real in every spectrum."""
    M = n // 2
    K = M + 1
    f = np.arange(F_INV)
    rng = np.random.default_rng(2400 + n)
    Y = np.zeros((NB, F_INV, K), dtype=np.complex128)
    Y[0] = (rng.standard_normal((F_INV, K)) + 1j * rng.standard_normal((F_INV, K))) * 100.0
    j = impulse_columns(n)
    Y[1] = (100.0 + f)[:, None] * np.exp(-2j * np.pi * ((j[:, None] * np.arange(K)[None, :]) % n) / n)
    for b, k0 in zip((2, 3, 4), tone_bins(n)):
        Y[b, :, k0] = (100.0 + 3 * f) * np.exp(1j * (0.3 + f))
    Y[5, :, 0] = 50.0 + f
    Y[5, :, M] = -(70.0 + f)
    Y = Y.astype(np.complex64)
    Y[..., 0] = Y[..., 0].real
    Y[..., M] = Y[..., M].real
    return Y


def inverse_spectra_iq(n):
    """(7, 12, n) complex64, bins in order: ROW_TYPES_IQ in order (the spectra of the forward I/Q rows' kinds)."""
    f = np.arange(F_INV)
    rng = np.random.default_rng(3000 + n)
    Y = np.zeros((NB_IQ, F_INV, n), dtype=np.complex128)
    Y[0] = (rng.standard_normal((F_INV, n)) + 1j * rng.standard_normal((F_INV, n))) * 100.0
    j = impulse_columns(n)
    Y[1] = ((100.0 + f) * np.exp(0.7j))[:, None] * np.exp(-2j * np.pi * ((j[:, None] * np.arange(n)[None, :]) % n) / n)
    for b, k0 in zip((2, 3, 4, 5), (1, n - 1, n // 2 - 1, n - n // 4)):
        Y[b, :, k0] = (100.0 + 3 * f) * np.exp(1j * (0.3 + f))
    Y[6, :, 0] = (50.0 + f) * (1 - 0.4j)
    Y[6, :, n // 2] = -(70.0 + f) * (1 + 0.3j)
    return Y.astype(np.complex64)


# ---- the restated steps around the transform, and the metrics (those of the kernels' own GPU files, per signal) ----------------------------

def frames(x, v, c):
    """x (B, T) float32 or complex64 -> the rows (B, frames, n_fft) the transform must see: pad, unfold, the window columns times the
    float32 v in float32, +0.0 elsewhere."""
    n, hop, col0, pad = c["n_fft"], c["hop"], c["col0"], c["pad"]
    xp = np.pad(x, ((0, 0), (pad, pad)), mode="reflect") if pad else x
    idx = np.arange(c["frames"])[:, None] * hop + np.arange(n)[None, :]
    y = np.zeros((x.shape[0], c["frames"], n), dtype=x.dtype)
    L = len(v)
    y[:, :, col0:col0 + L] = xp[:, idx[:, col0:col0 + L]] * v[None, None, :]
    return y


def row_error(Y, ref):
    """max over the rows of |Y - ref|_2 / |ref|_2, ref in float64 / complex128; a row whose reference is zero must be zero."""
    Y = np.asarray(Y).reshape(-1, Y.shape[-1]).astype(np.complex128)
    ref = np.asarray(ref).reshape(-1, ref.shape[-1])
    nr = np.sqrt((np.abs(ref) ** 2).sum(axis=-1))
    ne = np.sqrt((np.abs(Y - ref) ** 2).sum(axis=-1))
    zero = nr == 0
    assert not (ne[zero] != 0).any(), "an all-zero row must transform to zeros"
    return float((ne[~zero] / nr[~zero]).max()) if (~zero).any() else 0.0


def overlap_add64(rows, v, c):
    """rows (B, F, n_fft) float64 or complex128 -> (B, T): S = sum rows * v, E = sum v^2 over the frames reaching each output, in
    float64; S / E where normalised and E > 0."""
    nb, F, _ = rows.shape
    L, hop, col0, t0, T = len(v), c["hop"], c["col0"], c["t0"], c["T"]
    vd = v.astype(np.float64)
    W = max(t0 + T, (F - 1) * hop + L)
    S, E = np.zeros((nb, W), dtype=rows.dtype), np.zeros(W)
    for f in range(F):
        S[:, f * hop:f * hop + L] += rows[:, f, col0:col0 + L] * vd
        E[f * hop:f * hop + L] += vd * vd
    S, E = S[:, t0:t0 + T], E[t0:t0 + T]
    if not c["normalize"]:
        return S
    return np.where(E > 0, S / np.where(E > 0, E, 1.0), 0.0)


def signal_error(got, ref):
    """|got - ref|_2 / |ref|_2 of one signal (T,)."""
    ref = np.asarray(ref)
    got = np.asarray(got).astype(ref.dtype)
    nr = math.sqrt(float((np.abs(ref) ** 2).sum()))
    ne = math.sqrt(float((np.abs(got - ref) ** 2).sum()))
    assert nr > 0
    return ne / nr


def reached(c):
    """(T,) bool: the outputs some frame reaches."""
    w = np.arange(c["T"]) + c["t0"]
    r = np.zeros(c["T"], dtype=bool)
    for f in range(c["F"]):
        r |= (w >= f * c["hop"]) & (w < f * c["hop"] + c["L"])
    return r
