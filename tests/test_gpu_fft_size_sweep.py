"""Every n_fft of the fused FFT kernels on the GPU, on the rows of tests/fft_sweep_rows.py: noise, an impulse train, three exact-bin
tones and a DC-plus-Nyquist row.

The mixed-radix kernels (bhw.stft_mixed / spectrogram_mixed / istft_mixed and their ResidentTable forms) run at all 95 sizes, forward,
inverse and as a round trip: there a size is not a shape -- each n_fft has its own radix schedule, twiddle stride, (i, Ns) pairs of the
float-multiply `i mod Ns`, odd or even M, `cols` mask and ring step -- and the case tables of tests/stft_mfft_cases.py and
tests/istft_mfft_cases.py reach every class of the plan, not every size.  The power-of-two kernels (bhw.stft / istft at 16..4096,
bhw.stft_iq / istft_iq at 16..2048) run the same rows, which their own files -- noise at every size -- do not have.

References and metrics are those of the kernels' own GPU files, taken per signal so that no row type hides another: forward,
numpy.fft.rfft (fft) in float64 of the restated float32 rows, which the parent's stft_frames rows must equal bit for bit first, by
_row_errors; inverse, _ref64 by _err.  Gates (fft_sweep_rows.gate): the noise row keeps the project's gate, twice the yardstick's error
on the same GPU (torch.fft.rfft over the parent's rows; torch.fft.irfft + istft_overlap_add) under the cap 2^-24 log2 n_fft; a structured
row is held to twice the cap (the reasoning is in fft_sweep_rows.py; tests/test_fft_sweep_rows.py holds a float32 CPU library to the cap
itself on the same rows).  The yardstick's error on structured rows is printed, not gated.  Around the transform everything is held
word for word: library against table, +0.0 in the imaginary words of bins 0 and M, the power rows from the spectrum of the same call,
the shifted I/Q bins, +0.0 where no frame reaches.

Every test prints one line per row type: fused error, yardstick error, their ratio, fused / cap.  tools/sweep_fft_sizes.py records the
same figures (the *_figures functions below) in profiles/r21_fft_size_sweep.json."""
import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from test_gpu_stft import _frames_ref, _same
from test_gpu_stft_fft import _v, _row_errors
from test_gpu_spectrogram import _power_ref
from test_gpu_istft_mixed import _ref64, _err
import test_gpu_stft_iq as SQ
import test_gpu_istft_iq as XQ

import fft_sweep_rows as R
import plan_cases as PC
import stft_mfft_cases as MC
import istft_mfft_cases as XC

pytestmark = pytest.mark.gpu

FORWARD = {"mixed": ("stft_mixed", "k_stft_mfft_table"), "real": ("stft", None), "iq": ("stft_iq", None)}
INVERSE = {"mixed": ("istft_mixed", "k_istft_mfft_table"), "real": ("istft", None), "iq": ("istft_iq", None)}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


class Tables:
    """One resident table per parameter set, built at its first use and kept for the module."""

    def __init__(self):
        self.held = {}

    def __call__(self, setup):
        if setup not in self.held:
            self.held[setup] = bhw.ResidentTable(PC.params(setup))
        return self.held[setup]

    def close(self):
        for t in self.held.values():
            t.close()
        self.held = {}


@pytest.fixture(scope="module")
def tables(torch):
    t = Tables()
    yield t
    torch.cuda.synchronize()
    t.close()


def _words(torch, t):
    t = torch.view_as_real(t.contiguous()) if t.is_complex() else t.contiguous()
    return t.cpu().numpy().view(np.uint32)


def _names(kind):
    return R.ROW_TYPES_IQ if kind == "iq" else R.ROW_TYPES


def forward_figures(torch, tables, n, kind):
    """[(fused error, yardstick error)] per signal of the forward call of size n; kind "mixed", "real" or "iq".  Everything that is
    held word for word is asserted here."""
    iq = kind == "iq"
    c = R.forward_case(n, iq)
    p, tab = PC.params(c["setup"]), tables(c["setup"])
    hop, K = c["hop"], n if iq else n // 2 + 1
    xh = R.forward_signals_iq(n) if iq else R.forward_signals(n)
    v = _v(p, c["L"])
    kw = dict(win_length=c["L"], center=bool(c["mode"]), pad_mode=c["mode"] or "reflect")
    restated = _frames_ref(SQ._pairs(xh) if iq else xh[:, :, None], v, n, hop, c["col0"], c["pad"], c["mode"] or "constant")
    rows = SQ._complex(restated) if iq else restated[..., 0]
    assert rows.shape == (c["B"], c["frames"], n)
    x = torch.from_numpy(xh).cuda()
    parent = bhw.stft_frames(p, x, n, hop, **kw)
    assert _same((torch.view_as_real(parent) if iq else parent).cpu().numpy(), restated if iq else rows), "the parent's rows are the restated rows"
    yard = (torch.fft.fft if iq else torch.fft.rfft)(parent, dim=-1).cpu().numpy()
    name, kernel = FORWARD[kind]
    Y = getattr(bhw, name)(p, x, n, hop, **kw)
    Yt = getattr(tab, name)(p, x, n, hop, **kw)
    assert Y.dtype == torch.complex64 and tuple(Y.shape) == (c["B"], c["frames"], K)
    assert np.array_equal(_words(torch, Y), _words(torch, Yt)), "library against table"
    Yh = Y.cpu().numpy()
    if kind == "mixed":
        d = MC.parse(MC.line(c, table=tab._live()))
        assert d["table"] and kernel in d["kernels"] and d["rows"] == c["B"] * c["frames"] and d["groups"] > 1, d["line"]
        want = _power_ref(Yh).view(np.uint32)
        for src in (bhw, tab):
            P = src.spectrogram_mixed(p, x, n, hop, **kw)
            assert P.dtype == torch.float32 and np.array_equal(_words(torch, P), want), "the power rows are those of the spectrum of the same call"
    if iq:
        for src in (bhw, tab):
            S = src.stft_iq(p, x, n, hop, fftshift=True, **kw)
            assert np.array_equal(_words(torch, S), _words(torch, torch.fft.fftshift(Y, dim=-1))), "the shifted bins"
    else:
        im = np.ascontiguousarray(Yh.imag).view(np.uint32)
        assert not im[..., 0].any() and not im[..., -1].any(), "the imaginary words of bins 0 and M are +0.0"
    errors = SQ._row_errors if iq else _row_errors
    return [(errors(Yh[b], rows[b]), errors(yard[b], rows[b])) for b in range(c["B"])]


def inverse_figures(torch, tables, n, kind):
    """[(fused error, yardstick error)] per signal of the inverse call of size n; kind "mixed", "real" or "iq"."""
    iq = kind == "iq"
    c = R.inverse_case(n, iq)
    p, tab = PC.params(c["setup"]), tables(c["setup"])
    hop, T = c["hop"], c["T"]
    Yh = R.inverse_spectra_iq(n) if iq else R.inverse_spectra(n)
    v = _v(p, c["L"])
    kw = dict(win_length=c["L"], center=True, length=T, normalize=c["normalize"])
    ref = (XQ._ref64 if iq else _ref64)(Yh, v, n, hop, c["col0"], c["pad"], T, c["normalize"])
    Y = torch.from_numpy(Yh).cuda()
    rows = torch.fft.ifft(Y, dim=-1) if iq else torch.fft.irfft(Y, n=n, dim=-1)
    two = bhw.istft_overlap_add(p, rows, n, hop, **kw).cpu().numpy()
    name, kernel = INVERSE[kind]
    got = getattr(bhw, name)(p, Y, n, hop, **kw)
    gt = getattr(tab, name)(p, Y, n, hop, **kw)
    assert got.dtype == (torch.complex64 if iq else torch.float32) and tuple(got.shape) == (c["B"], T)
    assert np.array_equal(_words(torch, got), _words(torch, gt)), "library against table"
    if kind == "mixed":
        assert XC.geometry(c)[4] == T
        d = XC.parse(XC.line(c, table=tab._live()))
        assert d["table"] and kernel in d["kernels"], d["line"]
    assert not _words(torch, got)[:, ~R.reached(c)].any(), "outputs no frame reaches are +0.0"
    gh = got.cpu().numpy()
    err = XQ._err if iq else _err
    return [(err(gh[b:b + 1], ref[b:b + 1]), err(two[b:b + 1], ref[b:b + 1])) for b in range(c["B"])]


def round_trip_figures(torch, n):
    """(fused error, torch's error) of istft_mixed(stft_mixed(x), length=T) and torch.istft(torch.stft(x)) with the same float window,
    on signal 0 in the even-index geometry (L = n_fft, centred, reflect padding), against x."""
    hop, T = n // 4 + 1, 4 * n + 7
    p = PC.params(R.setup_for(R.index(n), n))
    xh = R.forward_signals(n)[0:1]
    x = torch.from_numpy(xh).cuda()
    v = bhw.window(p, n, dtype=torch.float32)
    back = bhw.istft_mixed(p, bhw.stft_mixed(p, x, n, hop, win_length=n), n, hop, win_length=n, length=T)
    St = torch.stft(x, n, hop, n, window=v, center=True, pad_mode="reflect", return_complex=True)
    tback = torch.istft(St, n, hop, n, window=v, center=True, length=T)
    assert back.shape == x.shape == tback.shape
    x64 = xh.astype(np.float64)
    return _err(back.cpu().numpy(), x64), _err(tback.cpu().numpy(), x64)


def _hold(what, kind, n, figures):
    """Print every figure, then hold the gates."""
    cap = R.cap(n)
    names = _names(kind)
    for b, (err, yard) in enumerate(figures):
        print(f"{what} {kind} n_fft {n}, {names[b]}: fused {err:.3e}, yardstick {yard:.3e}, ratio {err / yard if yard else float('nan'):.3f}, "
              f"cap {cap:.3e}, fused / cap {err / cap:.3f}")
    for b, (err, yard) in enumerate(figures):
        if b == 0:
            assert err <= 2.0 * yard, (what, kind, n, names[b], err, yard)
        assert err <= R.gate(n, b), (what, kind, n, names[b], err, R.gate(n, b))


@pytest.mark.parametrize("n", R.SIZES)
def test_forward_mixed_radix_every_size(torch, tables, n):
    _hold("stft", "mixed", n, forward_figures(torch, tables, n, "mixed"))


@pytest.mark.parametrize("n", R.SIZES)
def test_inverse_mixed_radix_every_size(torch, tables, n):
    _hold("istft", "mixed", n, inverse_figures(torch, tables, n, "mixed"))


@pytest.mark.parametrize("n", R.SIZES)
def test_round_trip_mixed_radix_every_size_as_well_as_torch(torch, n):
    """The gate of test_gpu_istft_mixed.test_round_trip_reproduces_the_signal_as_well_as_torch, which runs 400 and 480."""
    err, yard = round_trip_figures(torch, n)
    print(f"istft_mixed(stft_mixed(x)) n_fft {n} hop {n // 4 + 1}: fused {err:.3e}, torch.istft(torch.stft(x)) {yard:.3e}, ratio {err / yard:.3f}")
    assert err <= 2.0 * yard, (n, err, yard)


@pytest.mark.parametrize("n", R.POW2_REAL)
def test_forward_power_of_two_structured_rows(torch, tables, n):
    _hold("stft", "real", n, forward_figures(torch, tables, n, "real"))


@pytest.mark.parametrize("n", R.POW2_REAL)
def test_inverse_power_of_two_structured_rows(torch, tables, n):
    _hold("istft", "real", n, inverse_figures(torch, tables, n, "real"))


@pytest.mark.parametrize("n", R.POW2_IQ)
def test_forward_iq_structured_rows(torch, tables, n):
    _hold("stft", "iq", n, forward_figures(torch, tables, n, "iq"))


@pytest.mark.parametrize("n", R.POW2_IQ)
def test_inverse_iq_structured_rows(torch, tables, n):
    _hold("istft", "iq", n, inverse_figures(torch, tables, n, "iq"))
