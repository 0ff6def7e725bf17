"""Every n_fft the fused filter-and-sum kernels take, on the GPU: all 8 power-of-two and all 73 mixed-radix sizes at C = 2 channels,
each at the smallest shape that still has a halo and both padding edges -- B 2, F 7, hop n_fft // 4 + 1, L n_fft - 3, centred, reflect
padding at the even positions of a family's list and constant at the odd ones, (B, C, F, K) weights (beam_cases.gains), from one
resident table -- word for word against istft*(reference(stft*(x) per channel, g)) from the same table.  A failure names n_fft, the
schedule and lanes per row x rows per workgroup."""
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import beam_cases as BC

pytestmark = pytest.mark.gpu

NB, NCH, F = 2, 2, 7
SWEEP = [(fam, i, n) for fam, f in BC.FAMILIES.items() for i, n in enumerate(f.sizes)]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def table(torch):
    p = BC.FAMILIES["fft"].cmask.real.params(4)
    with bhw.ResidentTable(p) as tab:
        yield p, tab
        torch.cuda.synchronize()


def _shape(n):
    hop, L = n // 4 + 1, n - 3
    pad, col0 = n // 2, (n - L) // 2
    T = n + hop * (F - 1) - 2 * pad
    return hop, L, pad, col0, T


def _line(f, p, n, mode, table=None):
    hop, L, pad, col0, T = _shape(n)
    K = n // 2 + 1
    sa = B.make_stft(NB, T, F, hop, n, col0=col0, pad=pad, pad_mode=1 if mode == "reflect" else 0, shift=31)
    ss = B.make_stft(NB, T, F, hop, n, col0=col0, pad=pad, shift=31)
    return f.cmask.real.parse(f.describe(p, L, sa, ss, NCH, normalize=True, g_stride=K, g_ch_stride=F * K, g_batch_stride=NCH * F * K, table=table))


def test_the_sweep_is_all_81_sizes_with_a_halo_and_both_edges():
    assert len(SWEEP) == 81 and len({(fam, n) for fam, _, n in SWEEP}) == 81
    p = BC.FAMILIES["fft"].cmask.real.params(4)
    assert bytes(p) == bytes(BC.FAMILIES["mfft"].cmask.real.params(4))
    for fam, i, n in SWEEP:
        hop, L, pad, col0, T = _shape(n)
        assert T > pad and 1 + (T + 2 * pad - n) // hop == F         # reflection is defined, and the forward call gives F frames
        d = _line(BC.FAMILIES[fam], p, n, "reflect" if i % 2 == 0 else "constant")
        assert d["halo"] >= 1 and d["cpl"] <= 8, d["line"]


@pytest.mark.parametrize("fam,i,n", SWEEP, ids=[f"{fam}-n{n}" for fam, _, n in SWEEP])
def test_word_for_word_at_every_size(torch, table, fam, i, n):
    p, tab = table
    f = BC.FAMILIES[fam]
    hop, L, pad, col0, T = _shape(n)
    mode = "reflect" if i % 2 == 0 else "constant"
    K = n // 2 + 1
    x = torch.from_numpy(BC.inputs(NB, NCH, T, seed=n)).cuda()
    g = torch.from_numpy(BC.gains(NB, NCH, F, K, seed=n)).cuda()
    Y = getattr(tab, f.stft)(p, x.reshape(NB * NCH, T), n, hop, win_length=L, pad_mode=mode)
    assert tuple(Y.shape) == (NB * NCH, F, K)
    want = getattr(tab, f.istft)(p, BC.reference(Y.reshape(NB, NCH, F, K), g), n, hop, win_length=L, length=T)
    got = getattr(bhw, f.call)(p, x, g, n, hop, win_length=L, pad_mode=mode, length=T, table=tab)
    torch.cuda.synchronize()
    a, b = got.view(torch.int32), want.view(torch.int32)
    if not torch.equal(a, b):
        d = _line(f, p, n, mode, table=tab._live())
        bad = (a != b).nonzero()
        raise AssertionError(f"{fam} n_fft {n}: schedule {d['schedule']}, {d['lpf']} lanes per row x {d['fy']} rows per workgroup, {mode} "
                             f"padding: {bad.shape[0]} of {a.numel()} words differ, first at {bad[:4].tolist()}")
    assert bool(torch.isfinite(got).all())
