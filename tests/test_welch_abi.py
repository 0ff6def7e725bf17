"""Welch's method around the FFT (bhw_window_sums_* / bhw_welch_frames_f32_* / bhw_welch_psd_f32 / bhw_describe_welch): the checks
that need no GPU -- exports and declarations, every argument error before any HIP call, the workspace sizes, the describe lines, the
block constant, the scale arithmetic of bhw.welch against hand values and the Python surface."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
NEW_SYMBOLS = ("bhw_window_sums_device", "bhw_window_sums_from_table", "bhw_welch_workspace_bytes", "bhw_welch_frames_f32_device",
               "bhw_welch_frames_f32_from_table", "bhw_welch_psd_workspace_bytes", "bhw_welch_psd_f32", "bhw_describe_welch")
# never dereferenced: every call below fails or has nothing to do
A, Z, W = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000), ctypes.c_void_p(0x4000000000)


def _err():
    return B.lib().bhw_last_error().decode()


def _seg(**kw):
    """T1's Welch framing: 4 signals of 16000, window 400 in rows of 512, hop 160, no padding."""
    a = dict(batch=4, samples=16000, frames=98, hop=160, n_fft=512, shift=31)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _frames_calls(s, flags=1, ws=W, ws_bytes=1 << 20, L=400):
    lib = B.lib()
    return (lambda p: lib.bhw_welch_frames_f32_device(p, L, 0, None, ctypes.byref(s), flags, A, Z, ws, ws_bytes),
            lambda p: lib.bhw_welch_frames_f32_from_table(None, p, L, None, ctypes.byref(s), flags, A, Z, ws, ws_bytes))


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\b(int|uint64_t) " + name + r"\(", header), name
    for line in ("#define BHW_SUMS_F32 1u", "#define BHW_WELCH_DETREND_CONSTANT 1u", "#define BHW_PSD_ONESIDED 1u",
                 "#define BHW_WELCH_BLOCK 256u"):
        assert line in header, line
    assert ctypes.sizeof(B.BhwPsd) == 72 and B.BhwPsd.scale.offset == 64
    assert L.bhw_abi_version() == 4


def test_block_constant_is_in_the_header_not_the_plan():
    """BHW_WELCH_BLOCK is part of the periodogram's summation order: a constant of bhw.h that the binding repeats and the describe
    line reports, whatever the shape."""
    assert B.WELCH_BLOCK == 256 and bhw.WELCH_BLOCK == 256
    for F in (1, 255, 256, 257, 775, 32767):
        d = B.describe_welch(psd=B.make_psd(1, F, 513, 1024, 1.0, onesided=True))
        blocks = -(-F // 256)
        assert f"{blocks} block{'' if blocks == 1 else 's'} of 256 frames" in d, d


def test_window_sums_argument_errors_before_any_hip_call():
    lib = B.lib()
    p = B.make_params(B.WIN_BH7, 16, 32)
    ref = ctypes.byref(p)
    assert lib.bhw_window_sums_device(ref, 400, 0, None, 2, A) == BADARG and "flags" in _err()
    assert lib.bhw_window_sums_device(ref, 400, 0, None, 1, None) == BADARG and "NULL" in _err()
    assert lib.bhw_window_sums_device(ref, 400, 0, None, 1, ctypes.c_void_p(0x10000004)) == BADARG and "aligned" in _err()
    assert lib.bhw_window_sums_device(ref, 0, 0, None, 0, A) == BADARG and "length 0" in _err()
    assert lib.bhw_window_sums_device(ref, (1 << 16) + 1, 0, None, 0, A) == BADARG and "length" in _err()
    assert lib.bhw_window_sums_device(None, 400, 0, None, 0, A) == BADARG
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    assert lib.bhw_window_sums_device(ctypes.byref(taylor), 400, 0, None, 0, A) == UNSUPPORTED
    assert lib.bhw_window_sums_from_table(None, ctypes.byref(taylor), 400, None, 0, A) == UNSUPPORTED
    assert lib.bhw_window_sums_from_table(None, ref, 400, None, 0, A) == BADARG and "table is NULL" in _err()
    assert lib.bhw_window_sums_from_table(None, ref, 400, None, 4, A) == BADARG and "flags" in _err()


def test_segments_argument_errors_before_any_hip_call():
    lib = B.lib()
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    cases = [
        (dict(struct_size=8), "struct_size"),
        (dict(channels=3), "channels"),
        (dict(batch=0), "batch is 0"),
        (dict(hop=0), "hop is 0"),
        (dict(n_fft=0), "n_fft"),
        (dict(n_fft=399), "col0 + L"),
        (dict(shift=63), "shift"),
        (dict(frames=99), "segment 98 leaves the signal"),
        (dict(samples=0), "samples is 0"),
        (dict(x_stride=15999), "x_stride"),
        (dict(y_stride=511), "y_stride"),
        (dict(y_batch_stride=97 * 512 + 511), "y_batch_stride"),
        (dict(batch=1 << 20, frames=98), "2^34"),
        # Welch's own: no padding, the window at column 0, pad_mode 0
        (dict(pad=256, frames=98), "pad 256"),
        (dict(col0=56), "col0 56"),
        (dict(pad_mode=B.PAD_REFLECT), "pad_mode 1"),
    ]
    for flags in (0, 1):
        for kw, text in cases:
            s = _seg(**{k: v for k, v in kw.items() if k != "struct_size"})
            if "struct_size" in kw:
                s.struct_size = kw["struct_size"]
            for call in _frames_calls(s, flags=flags):
                rc = call(ref)
                assert rc == BADARG and text in _err(), (kw, flags, rc, _err())
    s = _seg()
    need = 4 * 98 * 1 * 4
    assert lib.bhw_welch_workspace_bytes(ctypes.byref(s), 1) == need and lib.bhw_welch_workspace_bytes(ctypes.byref(s), 0) == 0
    assert lib.bhw_welch_workspace_bytes(ctypes.byref(_seg(channels=2, batch=64, frames=7)), 1) == 64 * 7 * 2 * 4
    assert lib.bhw_welch_workspace_bytes(None, 1) == 0
    # unknown flags; the workspace: missing, misaligned, short, overlapping -- only where detrending needs one
    assert _frames_calls(s, flags=2)[0](ref) == BADARG and "flags 0x2" in _err()
    assert _frames_calls(s, flags=3)[1](ref) == BADARG and "flags 0x3" in _err()
    assert _frames_calls(s, ws=None, ws_bytes=0)[0](ref) == BADARG and "workspace is NULL" in _err() and str(need) in _err()
    assert _frames_calls(s, ws=ctypes.c_void_p(0x4000000002))[0](ref) == BADARG and "4-byte aligned" in _err()
    assert _frames_calls(s, ws_bytes=need - 1)[0](ref) == WORKSPACE and str(need) in _err()
    assert _frames_calls(s, ws_bytes=need - 1)[1](ref) == WORKSPACE
    assert _frames_calls(s, ws=ctypes.c_void_p(0x10000000 + 4 * 100))[0](ref) == BADARG and "workspace overlaps" in _err()
    assert _frames_calls(s, ws=ctypes.c_void_p(0x80000000 + 4 * 100))[0](ref) == BADARG and "workspace overlaps" in _err()
    assert _frames_calls(s, ws_bytes=need)[1](ref) == BADARG and "table is NULL" in _err()         # every check passed
    # without detrending no workspace is looked at: every check passes, and the from-table call stops at its NULL handle
    assert _frames_calls(s, flags=0, ws=None, ws_bytes=0)[1](ref) == BADARG and "table is NULL" in _err()
    # pointers, overlap, length, Taylor, frames 0
    assert lib.bhw_welch_frames_f32_device(ref, 400, 0, None, ctypes.byref(s), 1, None, Z, W, need) == BADARG and "NULL" in _err()
    assert lib.bhw_welch_frames_f32_device(ref, 400, 0, None, ctypes.byref(s), 1, A, A, W, need) == BADARG and "overlap" in _err()
    assert lib.bhw_welch_frames_f32_device(ref, 400, 0, None, None, 1, A, Z, W, need) == BADARG and "descriptor is NULL" in _err()
    assert lib.bhw_welch_frames_f32_device(ref, 0, 0, None, ctypes.byref(s), 1, A, Z, W, need) == BADARG and "length 0" in _err()
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    assert lib.bhw_welch_frames_f32_device(ctypes.byref(taylor), 400, 0, None, ctypes.byref(s), 1, A, Z, W, need) == UNSUPPORTED
    assert lib.bhw_welch_frames_f32_device(ref, 400, 0, None, ctypes.byref(_seg(frames=0)), 1, None, None, None, 0) == 0


def _psd(**kw):
    a = dict(batch=2, frames=300, bins=257, n_fft=512, scale=0.5, onesided=True)
    a.update(kw)
    return B.make_psd(a.pop("batch"), a.pop("frames"), a.pop("bins"), a.pop("n_fft"), a.pop("scale"), **a)


def test_psd_argument_errors_and_workspace_sizes():
    lib = B.lib()

    def call(d, Y=A, P=Z, ws=W, ws_bytes=1 << 30):
        return lib.bhw_welch_psd_f32(0, None, ctypes.byref(d) if d is not None else None, Y, P, ws, ws_bytes)

    cases = [
        (dict(batch=0), "is 0"), (dict(frames=0), "is 0"), (dict(bins=0), "is 0"),
        (dict(n_fft=0), "n_fft"), (dict(n_fft=(1 << 31) + 1, bins=5, onesided=False), "n_fft"),
        (dict(bins=513, onesided=False), "above n_fft"),
        (dict(bins=256), "BHW_PSD_ONESIDED needs bins"),
        (dict(scale=float("inf")), "not finite"), (dict(scale=float("nan")), "not finite"),
        (dict(y_stride=256), "y_stride"),
        (dict(y_batch_stride=299 * 257 + 256), "y_batch_stride"),
        (dict(p_stride=256), "p_stride"),
        (dict(batch=1 << 17, frames=1 << 10, bins=513, n_fft=1024), "2^34"),
        (dict(batch=1 << 33, frames=1, bins=1, n_fft=1, onesided=True), "2^31 - 1 workgroups"),
    ]
    for kw, text in cases:
        assert call(_psd(**kw)) == BADARG and text in _err(), (kw, _err())
    d = _psd()
    d.struct_size = 64
    assert call(d) == BADARG and "struct_size" in _err()
    d = _psd()
    d.flags = 2
    assert call(d) == BADARG and "flags 0x2" in _err()
    assert call(None) == BADARG and "descriptor is NULL" in _err()
    d = _psd()
    need = 2 * 2 * 257 * 8                                          # B * ceil(300 / 256) * K doubles
    assert lib.bhw_welch_psd_workspace_bytes(ctypes.byref(d)) == need
    for F, blocks in ((1, 1), (255, 1), (256, 1), (257, 2), (3 * 256 + 7, 4)):
        want = 0 if blocks == 1 else 3 * blocks * 33 * 8
        assert lib.bhw_welch_psd_workspace_bytes(ctypes.byref(_psd(batch=3, frames=F, bins=33, n_fft=64))) == want, F
    assert lib.bhw_welch_psd_workspace_bytes(None) == 0
    assert call(d, Y=None) == BADARG and "NULL" in _err()
    assert call(d, Y=ctypes.c_void_p(0x10000004)) == BADARG and "8-byte aligned" in _err()
    assert call(d, P=ctypes.c_void_p(0x80000002)) == BADARG and "4-byte aligned" in _err()
    assert call(d, P=ctypes.c_void_p(0x10000000 + 64)) == BADARG and "overlap" in _err()
    assert call(d, ws=None, ws_bytes=0) == BADARG and "workspace is NULL" in _err() and str(need) in _err()
    assert call(d, ws=ctypes.c_void_p(0x4000000004)) == BADARG and "8-byte aligned" in _err()
    assert call(d, ws_bytes=need - 1) == WORKSPACE and str(need) in _err()
    assert call(d, ws=ctypes.c_void_p(0x80000000 + 8)) == BADARG and "workspace overlaps" in _err()


def test_describe_names_route_plan_and_kernel():
    p = B.make_params(B.WIN_BH4, 24, 32)
    d = B.describe_welch(p, 400, stft=_seg(), detrend=True)
    assert d.startswith("welch segments direct (L = 400, n_fft 512), constant detrend: mean pass k_welch_mean<0> (one wave per row"), d
    assert "workspace 1568 bytes" in d and "then k_welch_frames_direct<" in d and "4 signals x 98 frames = 392 rows" in d
    assert "G = " in d and "256 along the row" in d
    d2 = B.describe_welch(p, 400, stft=_seg(channels=2), detrend=True)
    assert "k_welch_mean<2> (<1> where the pairs are not 8-byte aligned)" in d2 and "2 channels" in d2 and "workspace 3136 bytes" in d2
    d0 = B.describe_welch(p, 400, stft=_seg(frames=97))          # 97 frames also fit the stft call's n_fft extent rule
    assert d0 == "welch segments direct, no detrending: " + B.describe_stft(p, 400, _seg(frames=97)), d0
    assert "98 frames" in B.describe_welch(p, 400, stft=_seg())  # the last segment reads 400 samples, not 512
    assert "k_stft_frames_direct<" in d0
    assert "nothing" in B.describe_welch(p, 400, stft=_seg(frames=0), detrend=True)
    ds = B.describe_welch(p, 400, sums_f32=True)
    assert ds.startswith("window sums direct (L = 400, u = fl32(w)): memset of 4 words, then k_window_sums_direct<"), ds
    assert "grid 1 x 256 lanes, 2 coefficients per lane" in ds and "3 integer atomics per workgroup" in ds
    assert "grid 4096 x 256 lanes, 16 coefficients per lane" in B.describe_welch(p, 1 << 24)
    dp = B.describe_welch(psd=_psd())
    assert dp.startswith("welch psd (one-sided, n_fft 512): k_welch_psd<1,16>, 2 signals x 300 frames x 257 bins, 2 blocks of 256 frames"), dp
    assert "grid 20 x 256 lanes (64 along the bins x 4 waves of 16 frames a pass), then k_welch_psd_join in block order, workspace 8224 bytes" in dp
    dp = B.describe_welch(psd=_psd(frames=200, onesided=False, bins=512))
    assert "two-sided" in dp and "k_welch_psd<0,16>" in dp and "1 block of 256 frames" in dp and "workspace 0 bytes" in dp and "join" not in dp
    dp = B.describe_welch(psd=_psd(batch=64, frames=998))         # 1280 workgroups: the streaming instance
    assert "k_welch_psd<1,8>" in dp and "grid 1280 x 256 lanes (64 along the bins x 4 waves of 8 frames a pass)" in dp, dp
    lib, buf = B.lib(), ctypes.create_string_buffer(64)
    s, dd = _seg(), _psd()
    assert lib.bhw_describe_welch(None, ctypes.byref(p), 400, ctypes.byref(s), 0, ctypes.byref(dd), buf, 64) == BADARG and "not both" in _err()
    assert lib.bhw_describe_welch(None, ctypes.byref(p), 400, ctypes.byref(s), 2, None, buf, 64) == BADARG and "flags" in _err()
    assert lib.bhw_describe_welch(None, ctypes.byref(p), 400, ctypes.byref(_seg(col0=1)), 1, None, buf, 64) == BADARG and "col0" in _err()


def test_scale_arithmetic_of_welch_against_hand_values():
    """bhw.welch turns the four result words into S1, S2 and the periodogram scale on the host: checked here on words written by hand."""
    # a window of four coefficients u = 3, -1, 2, 4 at shift 1: s1 = 8, s2 = 30; S1 = 4, S2 = 7.5
    r = B.sums_from_words([8, 30, 0, 4], 1, 4)
    assert (r["s1"], r["s2"], r["S1"], r["S2"]) == (8, 30, 4.0, 7.5)
    assert r["coherent_gain"] == 1.0 and r["enbw_bins"] == 4 * 7.5 / 16.0
    assert B.welch_scale(r, 5, fs=2.0, scaling="density") == 1.0 / (2.0 * 7.5 * 5)
    assert B.welch_scale(r, 5, fs=2.0, scaling="spectrum") == 1.0 / (16.0 * 5)
    with pytest.raises(ValueError):
        B.welch_scale(r, 5, scaling="power")
    # s1 arrives in two's complement; the split counters join as lo + hi * 2^32, beyond 64 bits at the bound L = 2^30, |u| = 2^31
    r = B.sums_from_words([(1 << 64) - 6, 5, 0, 2], 0, 2)
    assert r["s1"] == -6 and r["S1"] == -6.0
    L = 1 << 30
    r = B.sums_from_words([(1 << 64) - (L << 31), 0, L << 30, L], 31, L)
    assert r["s1"] == -(1 << 61) and r["s2"] == 1 << 92 and r["S1"] == -float(L) and r["S2"] == float(L)
    assert r["coherent_gain"] == -1.0 and r["enbw_bins"] == 1.0
    r = B.sums_from_words([7, (1 << 62) - 1, (1 << 62) - 1, 9], 0, 9)
    assert r["s2"] == ((1 << 62) - 1) * ((1 << 32) + 1)
    # S1 and S2 are rounded once, from the exact rational: 2^53 + 1 halves to a tie that goes to even
    assert B.sums_from_words([(1 << 53) + 1, 1, 0, 1], 1, 1)["S1"] == float(1 << 52)
    with pytest.raises(RuntimeError):
        B.sums_from_words([8, 30, 0, 3], 1, 4)                    # the count word disagrees with L


def test_python_surface():
    for name in ("window_sums", "welch_frames", "welch_psd", "welch", "describe_welch", "BhwPsd", "WELCH_BLOCK"):
        assert hasattr(bhw, name), name
    for name in ("window_sums", "welch_frames", "welch"):
        assert hasattr(bhw.ResidentTable, name), name
    sig = inspect.signature(bhw.welch)
    assert list(sig.parameters)[:3] == ["params", "x", "fs"] and sig.parameters["fs"].default == 1.0
    assert sig.parameters["length"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["length"].default is inspect.Parameter.empty
    assert sig.parameters["noverlap"].default is None and sig.parameters["nfft"].default is None
    assert sig.parameters["detrend"].default == "constant" and sig.parameters["return_onesided"].default is True
    assert sig.parameters["scaling"].default == "density" and sig.parameters["shift"].default is None
    assert inspect.signature(bhw.welch_frames).parameters["detrend"].default == "constant"
