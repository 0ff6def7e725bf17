"""Every n_fft the fused STFT + gain + inverse STFT kernels for I/Q input take, on the GPU: all 8 power-of-two and all 91 mixed-radix
sizes (18 of them odd), each at one small shape that still has a halo span and both padding edges -- B 2, F 12, hop n_fft // 4 + 1,
L n_fft - 3, centred, reflect padding at the even positions of a family's list and constant at the odd ones, the gain columns shifted
at every third size -- with (B, F, n_fft) pair gains AND real gains at every size, from one resident table, word for word against
istft_iq*(reference(stft_iq*(x), g)) from the same table.  A failure names n_fft, the schedule and lanes per row x spans per
workgroup."""
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import mask_iq_cases as MC

pytestmark = pytest.mark.gpu

NB, F = 2, 12
SWEEP = [(fam, i, n) for fam, f in MC.FAMILIES.items() for i, n in enumerate(f.sizes)]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def table(torch):
    p = MC.params_of(4)
    with bhw.ResidentTable(p) as tab:
        yield p, tab
        torch.cuda.synchronize()


def _shape(n):
    hop, L = n // 4 + 1, n - 3
    pad, col0 = n // 2, (n - L) // 2
    T = n + hop * (F - 1) - 2 * pad
    return hop, L, pad, col0, T


def _descs(n, i):
    hop, L, pad, col0, T = _shape(n)
    sa = B.make_stft(NB, T, F, hop, n, col0=col0, pad=pad, pad_mode=1 - i % 2, channels=2, shift=31)
    ss = B.make_stft(NB, T, F, hop, n, col0=col0, pad=pad, channels=2, shift=31)
    return sa, ss


def test_the_sweep_is_all_99_sizes_with_a_halo_and_both_edges():
    assert len(SWEEP) == 99 and len({(fam, n) for fam, _, n in SWEEP}) == 99 and sum(n & 1 for _, _, n in SWEEP) == 18
    p = MC.params_of(4)
    for fam, i, n in SWEEP:
        hop, L, pad, col0, T = _shape(n)
        assert T > pad and 1 + (T + 2 * pad - n) // hop == F         # reflection is defined, and the forward call gives F frames
        sa, ss = _descs(n, i)
        d = MC.parse(dict(family=fam), MC.describe(fam, "pair")(p, L, sa, ss, normalize=True, g_stride=n, g_batch_stride=F * n))
        assert d["halo"] >= 1 and d["spans"] >= 2 and d["cpl"] <= 8, d["line"]


@pytest.mark.parametrize("fam,i,n", SWEEP, ids=[f"{fam}-n{n}" for fam, _, n in SWEEP])
def test_word_for_word_at_every_size(torch, table, fam, i, n):
    p, tab = table
    f = MC.FAMILIES[fam]
    hop, L, pad, col0, T = _shape(n)
    mode = "reflect" if i % 2 == 0 else "constant"
    shifted = i % 3 == 2
    gen = torch.Generator(device="cuda").manual_seed(7500 + n)
    x = torch.view_as_complex(torch.randn((NB, T, 2), device="cuda", generator=gen) * 100.0 + 5.0)
    Y = getattr(tab, f.stft)(p, x, n, hop, win_length=L, pad_mode=mode)
    assert tuple(Y.shape) == (NB, F, n)
    for gtype in MC.GTYPES:
        g = torch.from_numpy(MC.gains(NB, F, n, seed=n, gtype=gtype)).cuda()
        want = getattr(tab, f.istft)(p, MC.reference(Y, MC.unshift(g, n) if shifted else g), n, hop, win_length=L, length=T)
        got = getattr(bhw, MC.call_name(fam, gtype))(p, x, g, n, hop, win_length=L, pad_mode=mode, length=T, fftshift=shifted, table=tab)
        torch.cuda.synchronize()
        a, b = torch.view_as_real(got).view(torch.int32), torch.view_as_real(want).view(torch.int32)
        if not torch.equal(a, b):
            sa, ss = _descs(n, i)
            d = MC.parse(dict(family=fam), MC.describe(fam, gtype)(p, L, sa, ss, normalize=True, fftshift=shifted, g_stride=n,
                                                                  g_batch_stride=F * n, table=tab._live()))
            bad = (a != b).nonzero()
            raise AssertionError(f"{fam} n_fft {n}, {gtype} gains: schedule {d['schedule']}, {d['lpf']} lanes per row x {d['fy']} spans per "
                                 f"workgroup, {mode} padding, columns {'shifted' if shifted else 'in order'}: {bad.shape[0]} of {a.numel()} "
                                 f"words differ, first at {bad[:4].tolist()}")
        assert bool(torch.isfinite(torch.view_as_real(got)).all())
