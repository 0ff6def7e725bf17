"""Every n_fft the mixed-radix fused STFT + mask + inverse STFT kernel takes, on the GPU: all 73 sizes (mask_mfft_cases.SIZES), each at
the smallest shape that still has a halo and both padding edges -- B 2, F 7, hop n_fft // 4 + 1, L n_fft - 3, centred, reflect padding
at the even positions of the list and constant at the odd ones, (B, F, K) gains, from one resident table -- word for word against
bhw.istft_mixed(bhw.stft_mixed(x) * g) from the same table.  A failure names n_fft, the schedule and lanes per row x rows per
workgroup."""
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import mask_mfft_cases as MM

pytestmark = pytest.mark.gpu

NB, F = 2, 7


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def table(torch):
    p = MM.params(4)
    with bhw.ResidentTable(p) as tab:
        yield p, tab
        torch.cuda.synchronize()


def _shape(n):
    hop, L = n // 4 + 1, n - 3
    pad, col0 = n // 2, (n - L) // 2
    T = n + hop * (F - 1) - 2 * pad
    return hop, L, pad, col0, T


def test_the_sweep_is_all_73_sizes_with_a_halo_and_both_edges():
    assert len(MM.SIZES) == 73
    p = MM.params(4)
    for i, n in enumerate(MM.SIZES):
        hop, L, pad, col0, T = _shape(n)
        assert T > pad and 1 + (T + 2 * pad - n) // hop == F         # reflection is defined, and stft_mixed gives F frames
        sa = B.make_stft(NB, T, F, hop, n, col0=col0, pad=pad, pad_mode=1 - i % 2, shift=31)
        ss = B.make_stft(NB, T, F, hop, n, col0=col0, pad=pad, shift=31)
        d = MM.parse(B.describe_mask_mfft(p, L, sa, ss, normalize=True, g_stride=n // 2 + 1, g_batch_stride=F * (n // 2 + 1)))
        assert d["halo"] >= 1 and d["cpl"] <= 8, d["line"]


@pytest.mark.parametrize("i,n", list(enumerate(MM.SIZES)), ids=[f"n{n}" for n in MM.SIZES])
def test_word_for_word_at_every_size(torch, table, i, n):
    p, tab = table
    hop, L, pad, col0, T = _shape(n)
    mode = "reflect" if i % 2 == 0 else "constant"
    K = n // 2 + 1
    g = torch.Generator(device="cuda").manual_seed(7300 + n)
    x = torch.randn((NB, T), device="cuda", generator=g) * 100.0 + 5.0
    gains = torch.rand((NB, F, K), device="cuda", generator=g) * 2.0
    gains[:, :, ::7] = 0.0
    gains[:, :, 3::11] = 1.0
    Y = tab.stft_mixed(p, x, n, hop, win_length=L, pad_mode=mode)
    assert tuple(Y.shape) == (NB, F, K)
    Ym = torch.view_as_complex((torch.view_as_real(Y) * gains[..., None]).contiguous())
    want = tab.istft_mixed(p, Ym, n, hop, win_length=L, length=T)
    got = bhw.stft_mask_istft_mixed(p, x, gains, n, hop, win_length=L, pad_mode=mode, length=T, table=tab)
    torch.cuda.synchronize()
    a, b = got.view(torch.int32), want.view(torch.int32)
    if not torch.equal(a, b):
        sa = B.make_stft(NB, T, F, hop, n, col0=col0, pad=pad, pad_mode=1 if mode == "reflect" else 0, shift=31)
        ss = B.make_stft(NB, T, F, hop, n, col0=col0, pad=pad, shift=31)
        d = MM.parse(B.describe_mask_mfft(p, L, sa, ss, normalize=True, g_stride=K, g_batch_stride=F * K, table=tab._live()))
        bad = (a != b).nonzero()
        raise AssertionError(f"n_fft {n}: schedule {d['schedule']}, {d['lpf']} lanes per row x {d['fy']} rows per workgroup, {mode} padding: "
                             f"{bad.shape[0]} of {a.numel()} words differ, first at {bad[:4].tolist()}")
    assert bool(torch.isfinite(got).all())
