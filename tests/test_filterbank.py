"""bhw.mel_weights against an independent float64 restatement of torchaudio's melscale_fbanks written here (both are float64
computations rounded once to float32, so they differ by one rounding at most: one float32 ulp), and the band extraction of
bhw.FilterBank through its host-side helpers (fbank_bands / fbank_dense), which need no device."""
import math

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd.selector import fbank_bands, fbank_dense


def _hz_to_mel(f, scale):
    if scale == "htk":
        return 2595.0 * math.log10(1.0 + f / 700.0)
    if f < 1000.0:
        return 3.0 * f / 200.0
    return 15.0 + math.log(f / 1000.0) * 27.0 / math.log(6.4)


def _mel_to_hz(m, scale):
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    if m < 15.0:
        return 200.0 * m / 3.0
    return 1000.0 * math.exp(math.log(6.4) / 27.0 * (m - 15.0))


def _mel_ref(n_fft, n_mels, sr, f_min, f_max, norm, scale):
    """Scalar float64 loops: triangle m over the mel points m, m + 1, m + 2."""
    K = n_fft // 2 + 1
    lo, hi = _hz_to_mel(f_min, scale), _hz_to_mel(f_max, scale)
    pts = [_mel_to_hz(lo + (hi - lo) * i / (n_mels + 1), scale) for i in range(n_mels + 2)]
    w = np.zeros((K, n_mels), dtype=np.float64)
    for k in range(K):
        f = (sr // 2) * k / (K - 1)
        for m in range(n_mels):
            up = (f - pts[m]) / (pts[m + 1] - pts[m])
            down = (pts[m + 2] - f) / (pts[m + 2] - pts[m + 1])
            v = max(0.0, min(up, down))
            if norm == "slaney":
                v *= 2.0 / (pts[m + 2] - pts[m])
            w[k, m] = v
    return w


@pytest.mark.parametrize("n_fft,n_mels,sr,f_min,f_max,norm,scale", [
    (512, 80, 16000, 0.0, None, None, "htk"), (256, 80, 16000, 0.0, None, None, "htk"), (4096, 128, 16000, 0.0, None, None, "htk"),
    (64, 10, 16000, 0.0, None, None, "htk"), (400, 40, 8000, 20.0, 3800.0, "slaney", "slaney"), (1024, 64, 22050, 0.0, None, "slaney", "htk"),
    (512, 23, 16000, 50.0, 7000.0, None, "slaney"),
])
def test_mel_weights_against_a_float64_restatement(n_fft, n_mels, sr, f_min, f_max, norm, scale):
    got = bhw.mel_weights(n_fft, n_mels, sr, f_min=f_min, f_max=f_max, norm=norm, mel_scale=scale)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (n_fft // 2 + 1, n_mels) and got.flags.c_contiguous
    ref64 = _mel_ref(n_fft, n_mels, sr, f_min, sr / 2 if f_max is None else f_max, norm, scale)
    ref = ref64.astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(ref), np.abs(got)))
    # the two float64 values agree to float64 rounding, so their float32 roundings are equal or neighbours; a weight that is 0 in one
    # is at most a float64 rounding error of its slope in the other
    zero = (ref == 0) | (got == 0)
    assert (np.abs(got - ref)[~zero] <= ulp[~zero]).all()
    assert (np.abs(got.astype(np.float64) - ref64)[zero] <= 1e-12 * max(1.0, float(ref64.max()))).all()
    assert (got >= 0).all() and got.max() > 0
    assert float(np.abs(got.astype(np.float64) - ref64).max()) <= 2.0 ** -24 * float(ref64.max())


def test_mel_weights_arguments():
    with pytest.raises(ValueError, match="mel_scale"):
        bhw.mel_weights(512, 80, 16000, mel_scale="bark")
    with pytest.raises(ValueError, match="norm"):
        bhw.mel_weights(512, 80, 16000, norm="l2")
    with pytest.raises(ValueError, match="f_min"):
        bhw.mel_weights(512, 80, 16000, f_min=9000.0)
    with pytest.raises(ValueError):
        bhw.mel_weights(512, 0, 16000)


def test_band_extraction():
    w = np.zeros((9, 6), dtype=np.float32)
    w[:, 0] = np.arange(1, 10)                       # all K bins
    w[0, 1] = 0.5                                    # bin 0 alone
    w[8, 2] = -2.0                                   # bin M alone, negative
    #        3: empty
    w[1, 4], w[6, 4] = 2.0, 3.0                      # interior zeros are kept as weights
    w[3:5, 5] = (1.0, -0.0)                          # -0.0 is a zero: the band ends at the last nonzero weight
    first, offset, weight = fbank_bands(w)
    assert first.dtype == np.uint32 and offset.dtype == np.uint32 and weight.dtype == np.float32
    assert first.tolist() == [0, 0, 8, 0, 1, 3]
    assert offset.tolist() == [0, 9, 10, 11, 11, 17, 18]
    assert weight.tolist() == list(range(1, 10)) + [0.5, -2.0, 2.0, 0, 0, 0, 0, 3.0, 1.0]
    dense = fbank_dense(first, offset, weight, 9)
    assert dense.dtype == np.float32 and np.array_equal(dense, w)
    # all-zero bank: every filter empty, no weights
    first, offset, weight = fbank_bands(np.zeros((5, 3)))
    assert first.tolist() == [0, 0, 0] and offset.tolist() == [0, 0, 0, 0] and weight.size == 0
    assert np.array_equal(fbank_dense(first, offset, weight, 5), np.zeros((5, 3), dtype=np.float32))
    # float64 and integer input is rounded once to float32; a round trip of a mel bank is exact
    m = bhw.mel_weights(256, 80, 16000)
    first, offset, weight = fbank_bands(m.astype(np.float64))
    assert np.array_equal(fbank_dense(first, offset, weight, 129), m)
    assert int((np.diff(offset.astype(np.int64)) == 0).sum()) == 2
    assert ((first.astype(np.int64) + np.diff(offset.astype(np.int64))) <= 129).all() and int(offset[-1]) == weight.size
    for bad in (np.zeros(5), np.zeros((0, 3)), np.zeros((3, 0)), np.array([[1.0, np.nan]]), np.array([[1.0, np.inf]]), np.zeros((2, 2), dtype=complex)):
        with pytest.raises(ValueError):
            fbank_bands(bad)
