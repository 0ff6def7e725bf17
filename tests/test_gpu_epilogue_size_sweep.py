"""Every n_fft of the four fused forward FFT families on the GPU under every epilogue that is not the stored spectrum, on the rows,
geometries, references and bounds of tests/epilogue_sweep_rows.py: 95 mixed-radix real sizes, 91 mixed-radix I/Q sizes, 9 and 8 powers
of two.  The size sweeps (test_gpu_fft_size_sweep.py, test_gpu_iq_mixed_size_sweep.py) hold the stored spectrum at every size; the
accumulating epilogues -- the power rows, the filter bank, the frame average, the hold traces -- were held only at the 6 to 16 sizes
their class tables name, though their lane-to-bin maps, frame masks and barriers depend on fy, K, M and the pass count of the size.

For each size Y = stft*(...) of the library is computed once; then, for the library form AND the ResidentTable form:

  real sizes   spectrogram* power rows bit for bit fl32(re^2 + im^2) of Y (test_gpu_spectrogram._power_ref); with the six-filter bank
               of epilogue_sweep_rows.bank bit for bit the binary64 ascending band sum rounded once (_bank_ref); welch_fft* with
               onesided_doubling True and False word for word test_gpu_welch_mixed._restate(Y); hold_fft* both traces, both
               doublings, test_gpu_hold_real._want of the power rows bit for bit, and traces="max" alone the max trace.
  I/Q sizes    the same without a bank, each with fftshift False and True; the shifted result must be the unshifted words turned by
               n // 2, odd n included.
  float64      every front above inside its derived bound (epilogue_sweep_rows: power_bound, bank_bound, welch_bound, hold_bound),
               per signal and so per row type, against numpy.fft in float64 of the restated rows.  This check does not lean on
               stft*: it fails where the store and an epilogue are wrong alike, and for a dropped last chunk or a stored chunk of
               padding.  The stored spectrum itself is held to the sweep's gate on the same rows, the premise of the bounds.
  sentinels    at the sizes with bin M aside (1536, 2560, 3072) and at the smallest and largest size of each list, every front again
               into sentinel-filled outputs with gaps behind the bins: the gaps stay untouched, the words are the same.

Each test prints its differing words and ratios; the worst ratio to the bound per family and front is printed when the module ends.
tools/sweep_fft_sizes.py --epilogues records the same figures (epilogue_figures below) in profiles/r39_epilogue_size_sweep.json."""
import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from test_gpu_stft_fft import _v
from test_gpu_spectrogram import _power_ref, _bank_ref, _padded_out, _gaps_intact
from test_gpu_welch_mixed import _restate as _restate_real
from test_gpu_welch_iq_mixed import _restate as _restate_iq
from test_gpu_hold_real import _want as _want_real, _sk
from test_gpu_hold_iq import _want as _want_iq
from test_gpu_fft_size_sweep import Tables

import epilogue_sweep_rows as E
import fft_sweep_rows as R
import plan_cases as PC

pytestmark = pytest.mark.gpu

SENTINEL = 12345.5
FRONTS = {"mixed": ("stft_mixed", "spectrogram_mixed", "welch_fft_mixed", "hold_fft_mixed"),
          "iq_mixed": ("stft_iq_mixed", "spectrogram_iq_mixed", "welch_fft_iq_mixed", "hold_fft_iq_mixed"),
          "real": ("stft", "spectrogram", "welch_fft", "hold_fft"),
          "iq": ("stft_iq", "spectrogram_iq", "welch_fft_iq", "hold_fft_iq")}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def tables(torch):
    t = Tables()
    yield t
    torch.cuda.synchronize()
    t.close()


@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    sizes = {fam: w.pop(("sizes", fam)) for fam in E.FAMILIES if ("sizes", fam) in w}
    for (fam, front), (ratio, n, name) in sorted(w.items()):
        print(f"{fam} over {sizes[fam]} sizes, {front}: worst ratio to the bound {ratio:.3f} at n_fft {n}, {name}")


def _words(t):
    return t.contiguous().cpu().numpy().view(np.uint32)


def _differ(got, want):
    """The number of differing 32-bit words of a float32 tensor against a float32 tensor or array of the same shape."""
    g = _words(got)
    w = _words(want) if hasattr(want, "cpu") else np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (g.shape, w.shape)
    return int((g != w).sum())


def _gap_intact(buf, K):
    return bool((buf[..., K:] == SENTINEL).all())


def epilogue_figures(torch, tables, fam, n):
    """[{front, form, words, differ, ratios}] of every front of family fam at size n: `differ` the words that differ from the exact
    reference (None where the entry has none), `ratios` the ratio to the derived float64 bound per signal (None where the entry has
    none).  The sentinel runs of epilogue_sweep_rows.sentinel_sizes are entries of their own with front "... into sentinels"; a
    written gap is asserted here."""
    iq = E.IQ[fam]
    c = E.case(fam, n)
    p, tab = PC.params(c["setup"]), tables(c["setup"])
    hop, nb, F, K = c["hop"], c["B"], c["frames"], E.bins(fam, n)
    kw = E.call_kw(c)
    stft_name, spec_name, welch_name, hold_name = FRONTS[fam]
    xh = E.signals(fam, n)
    x = torch.from_numpy(xh).cuda()
    Y64 = E.spectrum64(E.rows(xh, _v(p, c["L"]), c))                  # the float64 reference: no call of the library's transform
    P64 = E.power64(Y64)
    out = []

    def entry(front, form, got=None, want=None, ratios=None):
        out.append(dict(front=front, form=form, words=None if got is None else got.numel(),
                        differ=None if want is None else _differ(got, want), ratios=ratios))

    Y = getattr(bhw, stft_name)(p, x, n, hop, **kw)
    assert Y.dtype == torch.complex64 and tuple(Y.shape) == (nb, F, K)
    Yh = Y.cpu().numpy()
    entry("stored spectrum", "library", ratios=[R.row_error(Yh[b], Y64[b]) / E.gate(n, b) for b in range(nb)])
    Pw = _power_ref(Yh)                                                # (B, F, K) float32: the rows every exact contract is stated on
    Pt = torch.from_numpy(Pw).cuda()
    wscale = E.WELCH_SCALE_C / F
    sentinels = n in E.sentinel_sizes(fam)
    shifts = (False, True) if iq else (None,)
    turn = (lambda t: torch.roll(t, n // 2, dims=-1))                  # fftshift=True writes bin k to column (k + n // 2) % n
    back = (lambda a: np.roll(a, -(n // 2), axis=-1))
    if not iq:
        W = E.bank(n)
        fb = bhw.FilterBank(W.astype(np.float32), device="cuda")
        assert (fb.filters, fb.bins) == (E.FILTERS, K)
        want_bank = _bank_ref(Pw.reshape(-1, K), W.astype(np.float32))[0].reshape(nb, F, E.FILTERS)
    for form, src in (("library", bhw), ("table", tab)):
        spectro, welch, hold = getattr(src, spec_name), getattr(src, welch_name), getattr(src, hold_name)
        for shifted in shifts:
            skw = dict(kw, fftshift=shifted) if iq else kw
            tag = " shifted" if shifted else ""
            put = turn if shifted else (lambda t: t)
            get = back if shifted else (lambda a: a)
            # the power rows, and the bank
            S = spectro(p, x, n, hop, **skw)
            assert S.dtype == torch.float32 and tuple(S.shape) == (nb, F, K)
            entry("power" + tag, form, S, put(Pt), E.power_ratios(fam, n, get(S.cpu().numpy()), P64))
            if not iq:
                Sb = spectro(p, x, n, hop, fbank=fb, **kw)
                assert Sb.dtype == torch.float32 and tuple(Sb.shape) == (nb, F, E.FILTERS)
                entry("bank", form, Sb, want_bank, E.bank_ratios(fam, n, Sb.cpu().numpy(), P64, W))
            # the frame average
            for doubled in ((False,) if iq else (True, False)):
                dkw = skw if iq else dict(kw, onesided_doubling=doubled)
                want = _restate_iq(torch, Y, wscale) if iq else _restate_real(torch, Y, wscale, n, doubled)
                got = welch(p, x, n, hop, wscale, **dkw)
                assert got.dtype == torch.float32 and tuple(got.shape) == (nb, K)
                s = E.sk(fam, n, wscale, doubled)
                entry("welch" + tag + (" doubled" if doubled else ""), form, got, put(want),
                      E.welch_ratios(fam, n, get(got.cpu().numpy()), P64, s))
                if sentinels:
                    buf = torch.full((nb, K + 5), SENTINEL, device="cuda")
                    g2 = welch(p, x, n, hop, wscale, out=buf[:, :K], **dkw)
                    assert g2.data_ptr() == buf.data_ptr() and _gap_intact(buf, K), (fam, n, form, "welch: a gap was written")
                    entry("welch" + tag + (" doubled" if doubled else "") + " into sentinels", form, g2, put(want))
            # the hold traces
            for doubled in ((False,) if iq else (True, False)):
                dkw = skw if iq else dict(kw, onesided_doubling=doubled)
                wmax, wmin = _want_iq(Pt, E.HOLD_SCALE) if iq else _want_real(Pt, _sk(torch, n, E.HOLD_SCALE, doubled))
                pmax, pmin = hold(p, x, n, hop, E.HOLD_SCALE, **dkw)
                assert pmax.dtype == pmin.dtype == torch.float32 and tuple(pmax.shape) == tuple(pmin.shape) == (nb, K)
                s = E.sk(fam, n, E.HOLD_SCALE, doubled)
                name = "hold" + tag + (" doubled" if doubled else "")
                entry(name + " max", form, pmax, put(wmax), E.hold_ratios(fam, n, get(pmax.cpu().numpy()), P64, s, "max"))
                entry(name + " min", form, pmin, put(wmin), E.hold_ratios(fam, n, get(pmin.cpu().numpy()), P64, s, "min"))
                if sentinels:
                    buf = torch.full((2, nb, K + 5), SENTINEL, device="cuda")
                    qmax, qmin = hold(p, x, n, hop, E.HOLD_SCALE, out_max=buf[0, :, :K], out_min=buf[1, :, :K], **dkw)
                    assert _gap_intact(buf, K), (fam, n, form, "hold: a gap was written")
                    entry(name + " max into sentinels", form, qmax, put(wmax))
                    entry(name + " min into sentinels", form, qmin, put(wmin))
            only, none = hold(p, x, n, hop, E.HOLD_SCALE, traces="max", **dkw)
            assert none is None
            entry("hold" + tag + " max alone", form, only, put(wmax))
            if sentinels:
                buf, view = _padded_out(torch, nb, F, K)
                S2 = spectro(p, x, n, hop, out=view, **skw)
                assert S2.data_ptr() == view.data_ptr() and _gaps_intact(torch, buf, nb, F, K), (fam, n, form, "power: a gap was written")
                entry("power" + tag + " into sentinels", form, S2, put(Pt))
                if not iq:
                    buf, view = _padded_out(torch, nb, F, E.FILTERS)
                    S3 = spectro(p, x, n, hop, fbank=fb, out=view, **kw)
                    assert _gaps_intact(torch, buf, nb, F, E.FILTERS), (fam, n, form, "bank: a gap was written")
                    entry("bank into sentinels", form, S3, want_bank)
    torch.cuda.synchronize()
    return out


def _hold(fam, n, figures, worst):
    """Print every figure, then hold the contracts: no differing word, every ratio at most 1."""
    names = E.row_types(fam)
    worst[("sizes", fam)] = worst.get(("sizes", fam), 0) + 1
    for e in figures:
        r = "" if e["ratios"] is None else ", ratio to the bound " + " ".join(f"{v:.3f}" for v in e["ratios"])
        d = "" if e["differ"] is None else f", {e['differ']} differing words of {e['words']}"
        print(f"{fam} n_fft {n}, {e['front']} ({e['form']}){d}{r}")
        if e["ratios"] is not None:
            b = int(np.argmax(e["ratios"]))
            if e["ratios"][b] > worst.get((fam, e["front"]), (-1.0, 0, ""))[0]:
                worst[(fam, e["front"])] = (e["ratios"][b], n, names[b])
    for e in figures:
        assert e["differ"] in (None, 0), (fam, n, e["front"], e["form"], e["differ"], e["words"])
    for e in figures:
        if e["ratios"] is not None:
            assert len(e["ratios"]) == len(names)
            for b, v in enumerate(e["ratios"]):
                assert v <= 1.0, (fam, n, e["front"], e["form"], names[b], v)


@pytest.mark.parametrize("n", E.FAMILIES["mixed"])
def test_every_epilogue_mixed_radix_every_size(torch, tables, worst, n):
    _hold("mixed", n, epilogue_figures(torch, tables, "mixed", n), worst)


@pytest.mark.parametrize("n", E.FAMILIES["iq_mixed"])
def test_every_epilogue_iq_mixed_radix_every_size(torch, tables, worst, n):
    _hold("iq_mixed", n, epilogue_figures(torch, tables, "iq_mixed", n), worst)


@pytest.mark.parametrize("n", E.FAMILIES["real"])
def test_every_epilogue_power_of_two_every_size(torch, tables, worst, n):
    _hold("real", n, epilogue_figures(torch, tables, "real", n), worst)


@pytest.mark.parametrize("n", E.FAMILIES["iq"])
def test_every_epilogue_iq_power_of_two_every_size(torch, tables, worst, n):
    _hold("iq", n, epilogue_figures(torch, tables, "iq", n), worst)
