"""Every n_fft of bhw.stft_iq_mixed on the GPU -- all 91 sizes 2^a 3^b 5^c in 16..2047 that are no power of two, 18 of them odd --
on the rows of tests/iq_mixed_sweep_rows.py: noise, impulses, exact-bin tones in both halves of the spectrum and the DC-plus-Nyquist
row (at an odd n_fft: DC plus the tone at (n - 1) / 2).  In the mixed-radix kernel a size is not a shape: each n_fft has its own radix
schedule, twiddle stride, (i, Ns) pairs of the float-multiply `i mod Ns`, folded or full twiddle table, `cols` mask and bin turn.

Gates, the project's (fft_sweep_rows): noise rows within the cap 2^-24 log2 n and twice torch.fft.fft's error on the parent's rows on
the same GPU; structured rows within twice the cap.  Word for word: library against table, the power rows and the shifted bins
against the spectrum of the same call.  And the done-when of the front: .transpose(-1, -2) of the call is torch.stft(onesided=False)
within test_gpu_stft_iq.test_against_torch_stft's bound, at every size.  The worst figure per row type is printed when the module
ends."""
import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from test_gpu_stft import _frames_ref, _same
from test_gpu_spectrogram import _power_ref
import test_gpu_stft_iq as SQ

import iq_mixed_sweep_rows as Q
import plan_cases as PC
import stft_cmfft_cases as XC

pytestmark = pytest.mark.gpu


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
            print(f"stft_iq_mixed over {w['sizes']} sizes, {name}: worst fused / cap {w[b][0]:.3f} at n_fft {w[b][1]}")
    if "noise ratio" in w:
        print(f"stft_iq_mixed over {w['sizes']} sizes, noise: worst fused / torch.fft.fft {w['noise ratio'][0]:.3f} at n_fft {w['noise ratio'][1]}")


def _words(torch, t):
    t = torch.view_as_real(t.contiguous()) if t.is_complex() else t.contiguous()
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n", Q.SIZES)
def test_forward_iq_mixed_every_size(torch, tables, worst, n):
    c = Q.forward_case(n)
    p, tab = PC.params(c["setup"]), tables(c["setup"])
    hop = c["hop"]
    xh = Q.forward_signals_iq(n)
    v = SQ._v(p, c["L"])
    kw = dict(win_length=c["L"], center=bool(c["mode"]), pad_mode=c["mode"] or "reflect")
    restated = _frames_ref(SQ._pairs(xh), v, n, hop, c["col0"], c["pad"], c["mode"] or "constant")
    rows = SQ._complex(restated)
    assert rows.shape == (c["B"], c["frames"], n)
    x = torch.from_numpy(xh).cuda()
    parent = bhw.stft_frames(p, x, n, hop, **kw)
    assert _same(torch.view_as_real(parent).cpu().numpy(), restated), "the parent's rows are the restated rows"
    yard = torch.fft.fft(parent, dim=-1).cpu().numpy()
    Y = bhw.stft_iq_mixed(p, x, n, hop, **kw)
    assert Y.dtype == torch.complex64 and tuple(Y.shape) == (c["B"], c["frames"], n)
    d = XC.parse(XC.line(c, table=tab._live()))
    assert d["table"] and "k_stft_cmfft_table" in d["kernels"] and d["rows"] == c["B"] * c["frames"] and d["groups"] > 1, d["line"]
    assert np.array_equal(_words(torch, Y), _words(torch, tab.stft_iq_mixed(p, x, n, hop, **kw))), "library against table"
    Yh = Y.cpu().numpy()
    want = _power_ref(Yh).view(np.uint32)
    for src in (bhw, tab):
        P = src.spectrogram_iq_mixed(p, x, n, hop, **kw)
        assert P.dtype == torch.float32 and np.array_equal(_words(torch, P), want), "the power rows are those of the spectrum of the same call"
        S = src.stft_iq_mixed(p, x, n, hop, fftshift=True, **kw)
        assert np.array_equal(_words(torch, S), _words(torch, torch.fft.fftshift(Y, dim=-1))), "the shifted bins"
    ref = torch.stft(x, n, hop, c["L"], window=bhw.window(p, c["L"], dtype=torch.float32), center=kw["center"], pad_mode=kw["pad_mode"],
                     onesided=False, return_complex=True)
    assert ref.shape == Y.transpose(-1, -2).shape
    assert float((Y.transpose(-1, -2) - ref).abs().max() / ref.abs().max()) < 1e-5, "against torch.stft"
    figures = [(SQ._row_errors(Yh[b], rows[b]), SQ._row_errors(yard[b], rows[b])) for b in range(c["B"])]
    cap = Q.cap(n)
    for b, (err, yd) in enumerate(figures):
        print(f"stft_iq_mixed n_fft {n}, {Q.ROW_TYPES_IQ[b]}: fused {err:.3e}, yardstick {yd:.3e}, ratio {err / yd if yd else float('nan'):.3f}, "
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
