"""The mixed-radix fused window + FFT calls (bhw_stft_mfft_f32_device / _from_table / bhw_describe_stft_mfft): the checks that need no
GPU -- exports and declarations, every refusal of include/bhw.h before any HIP call, frames 0, the describe line, the Python surface,
and that the power-of-two families still refuse what these calls take."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import stft_mfft_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED = 0, -1, -2
NEW_SYMBOLS = ("bhw_stft_mfft_f32_device", "bhw_stft_mfft_f32_from_table", "bhw_describe_stft_mfft")
DETREND, POWER = B.WELCH_DETREND_CONSTANT, B.MFFT_POWER
# never dereferenced: every call below fails or has nothing to do
A, Z = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000)
W1, W2, W3 = 0x40000000, 0x41000000, 0x42000000


def _err():
    return B.lib().bhw_last_error().decode()


def _seg(**kw):
    """Welch framing: 4 signals of 16000, window 320 in rows of 400, hop 160, no padding."""
    a = dict(batch=4, samples=16000, frames=99, hop=160, n_fft=400, shift=31)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _bank(**kw):
    a = dict(filters=80, bins=201, weights=1000, d_first=W1, d_offset=W2, d_weight=W3)
    a.update(kw)
    return B.make_fbank(a["filters"], a["bins"], a["weights"], a["d_first"], a["d_offset"], a["d_weight"])


def _calls(s, flags=DETREND, L=320, x=A, Y=Z, fb=None):
    lib = B.lib()
    sr = ctypes.byref(s) if s is not None else None
    fr = ctypes.byref(fb) if fb is not None else None
    return (lambda p: lib.bhw_stft_mfft_f32_device(p, L, 0, None, sr, flags, fr, x, Y),
            lambda p: lib.bhw_stft_mfft_f32_from_table(None, p, L, None, sr, flags, fr, x, Y))


def _passes(ref, s, flags, fb=None, L=320, x=A, Y=Z):
    """Every check passed: the from-table call with no table stops at "table is NULL", before any launch."""
    rc = B.lib().bhw_stft_mfft_f32_from_table(None, ref, L, None, ctypes.byref(s), flags, ctypes.byref(fb) if fb is not None else None, x, Y)
    return rc == BADARG and "table is NULL" in _err()


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert re.search(r"#define BHW_MFFT_POWER 2u", header) and B.MFFT_POWER == 2
    assert L.bhw_abi_version() == 4 and ctypes.sizeof(B.BhwStft) == 96          # additions only, no version bump


def test_descriptor_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    K2 = 402
    cases = [
        (dict(struct_size=8), BADARG, "struct_size"),
        (dict(channels=3), BADARG, "channels"),
        (dict(channels=2), UNSUPPORTED, "real input"),
        (dict(batch=0), BADARG, "batch is 0"),
        (dict(hop=0), BADARG, "hop is 0"),
        (dict(n_fft=0), BADARG, "n_fft"),
        (dict(n_fft=300), BADARG, "col0 + L"),
        (dict(n_fft=512), UNSUPPORTED, "bhw_stft_fft_f32_"),
        (dict(n_fft=8192), UNSUPPORTED, "bhw_stft_fft_f32_"),
        (dict(n_fft=405), UNSUPPORTED, "even 2^a 3^b 5^c"),
        (dict(n_fft=420), UNSUPPORTED, "even 2^a 3^b 5^c"),
        (dict(n_fft=4500), UNSUPPORTED, "even 2^a 3^b 5^c"),
        (dict(shift=63), BADARG, "shift"),
        (dict(frames=100), BADARG, "segment 99 leaves the signal"),
        (dict(samples=0), BADARG, "samples is 0"),
        (dict(x_stride=15999), BADARG, "x_stride"),
        (dict(y_stride=K2 - 2), BADARG, "y_stride"),
        (dict(y_stride=K2 + 1), BADARG, "even"),
        (dict(y_batch_stride=98 * K2 + K2 - 2), BADARG, "y_batch_stride"),
        (dict(y_batch_stride=99 * K2 + 1), BADARG, "even"),
        (dict(batch=1 << 20, frames=99), BADARG, "2^34"),
    ]
    for flags in (0, DETREND):
        for kw, code, text in cases:
            s = _seg(**{k: v for k, v in kw.items() if k != "struct_size"})
            if "struct_size" in kw:
                s.struct_size = kw["struct_size"]
            for call in _calls(s, flags=flags):
                assert call(ref) == code and text in _err(), (flags, kw, _err())
    # power rows: W = K floats, no evenness rule; bank rows: W = filters
    for flags in (POWER, POWER | DETREND):
        assert _passes(ref, _seg(y_stride=201), flags) and _passes(ref, _seg(y_stride=203, y_batch_stride=99 * 203 + 1), flags)
        for call in _calls(_seg(y_stride=200), flags=flags):
            assert call(ref) == BADARG and "y_stride" in _err()
        for call in _calls(_seg(y_batch_stride=98 * 201 + 200), flags=flags):
            assert call(ref) == BADARG and "y_batch_stride" in _err()
        assert _passes(ref, _seg(y_stride=80), flags, fb=_bank())
        for call in _calls(_seg(y_stride=79), flags=flags, fb=_bank()):
            assert call(ref) == BADARG and "y_stride" in _err()
    # with the detrend flag, the restrictions of the segments call
    for kw, text in ((dict(pad=200), "pad 200"), (dict(col0=40), "col0 40"), (dict(pad_mode=B.PAD_REFLECT), "pad_mode 1")):
        for call in _calls(_seg(**kw), flags=DETREND):
            assert call(ref) == BADARG and text in _err(), (kw, _err())
    # without it they are a centred STFT under the frames call's extent rule
    assert _passes(ref, _seg(pad=200, col0=40, pad_mode=B.PAD_REFLECT, frames=101), 0)
    for call in _calls(_seg(pad=200, col0=40, pad_mode=B.PAD_REFLECT, frames=102), flags=0):
        assert call(ref) == BADARG and "leaves the padded signal" in _err()
    for call in _calls(_seg(pad=200, pad_mode=B.PAD_REFLECT, samples=150, frames=1), flags=0, L=400):
        assert call(ref) == BADARG and "reflect padding" in _err()
    for call in _calls(_seg(pad_mode=7), flags=0):
        assert call(ref) == BADARG and "pad_mode" in _err()
    # the extent rule without padding is the segments' one with and without the flag: 99 segments of 320 fit, rows of 400 would not
    assert 98 * 160 + 400 > 16000 >= 98 * 160 + 320
    for flags in (0, DETREND):
        assert _passes(ref, _seg(), flags)


def test_argument_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    s = _seg()
    for flags in (4, 8, 0x80000000, 4 | POWER):
        for call in _calls(s, flags=flags):
            assert call(ref) == BADARG and "flags" in _err()
    for call in _calls(None):
        assert call(ref) == BADARG and "descriptor is NULL" in _err()
    for call in _calls(s):
        assert call(None) == BADARG
    for call in _calls(s, L=0):
        assert call(ref) == BADARG and "length" in _err()
    for call in _calls(s, x=None):
        assert call(ref) == BADARG and "NULL" in _err()
    for call in _calls(s, Y=None):
        assert call(ref) == BADARG and "NULL" in _err()
    for call in _calls(s, Y=ctypes.c_void_p(0x80000004)):
        assert call(ref) == BADARG and "8-byte aligned" in _err()
    assert _passes(ref, s, POWER, Y=ctypes.c_void_p(0x80000004))                 # power rows are floats
    for call in _calls(s, flags=POWER, Y=ctypes.c_void_p(0x80000002)):
        assert call(ref) == BADARG and "4-byte aligned" in _err()
    for call in _calls(s, x=ctypes.c_void_p(0x10000002)):
        assert call(ref) == BADARG and "4-byte aligned" in _err()
    # d_out inside x, x inside d_out, and the first byte behind each: x holds 4 * 16000 floats, the spectrum 4 * 99 * 402
    xb, yb = 4 * 16000 * 4, 4 * 99 * 402 * 4
    for x, Y, bad in ((0x10000000, 0x10000000 + xb - 8, True), (0x10000000, 0x10000000 + xb, False), (0x80000000 + yb - 4, 0x80000000, True),
                      (0x80000000 + yb, 0x80000000, False)):
        rc = B.lib().bhw_stft_mfft_f32_from_table(None, ref, 320, None, ctypes.byref(s), DETREND, None, ctypes.c_void_p(x), ctypes.c_void_p(Y))
        assert rc == BADARG and ("overlap" if bad else "table is NULL") in _err(), (hex(x), hex(Y), _err())
        if bad:
            assert B.lib().bhw_stft_mfft_f32_device(ref, 320, 0, None, ctypes.byref(s), DETREND, None, ctypes.c_void_p(x), ctypes.c_void_p(Y)) == BADARG
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    for call in _calls(s):
        assert call(ctypes.byref(taylor)) == UNSUPPORTED
    assert _passes(ref, s, DETREND)


def test_filter_bank_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    s = _seg()
    for flags in (0, DETREND):                                                   # fb needs BHW_MFFT_POWER
        for call in _calls(s, flags=flags, fb=_bank()):
            assert call(ref) == BADARG and "BHW_MFFT_POWER" in _err()
    assert _passes(ref, s, POWER, fb=_bank()) and _passes(ref, s, POWER | DETREND, fb=_bank())
    bad = [(dict(filters=0), "filters"), (dict(filters=4097), "filters"), (dict(bins=257), "bins"), (dict(bins=200), "bins"),
           (dict(weights=(1 << 24) + 1), "weights"), (dict(d_first=None), "d_first"), (dict(d_offset=None), "d_offset"),
           (dict(d_weight=None), "d_weight"), (dict(d_first=W1 + 2), "aligned"), (dict(d_weight=W3 + 1), "aligned"),
           (dict(d_offset=0x80000000 + 64), "overlap"), (dict(d_weight=0x80000000 - 8), "overlap")]
    for kw, text in bad:
        for call in _calls(s, flags=POWER, fb=_bank(**kw)):
            assert call(ref) == BADARG and text in _err(), (kw, _err())
    fb = _bank()
    fb.struct_size = 40
    for call in _calls(s, flags=POWER, fb=fb):
        assert call(ref) == BADARG and "struct_size" in _err()
    fb = _bank()
    fb.reserved = 1
    for call in _calls(s, flags=POWER, fb=fb):
        assert call(ref) == BADARG and "reserved" in _err()
    assert _passes(ref, s, POWER, fb=_bank(weights=0, d_weight=None))             # an empty bank needs no weights


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1024)
    for n in range(1, 5001):
        s = B.make_stft(2, 100000, 3, 7, n, shift=31)
        rc = lib.bhw_describe_stft_mfft(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), DETREND, None, buf, 1024)
        assert rc == (OK if B.mfft_supported(n) else UNSUPPORTED), (n, rc, _err())
        assert not (B.mfft_supported(n) and B.fft_supported(n)), n                # one transform per n_fft
    ok = [n for n in range(1, 5001) if B.mfft_supported(n)]
    assert len(ok) == 95 and all(n % 2 == 0 and n & (n - 1) and 16 <= n < 4096 for n in ok)
    assert all(n in ok for n in (400, 480, 960, 1000, 1200, 1920, 18, 4050))
    assert [n for n in range(1, 8300) if B.fft_supported(n)] == [1 << k for k in range(4, 13)]        # unchanged


def test_the_power_of_two_families_still_refuse_these_sizes():
    p = B.make_params(B.WIN_BH7, 16, 32)
    ref = ctypes.byref(p)
    lib = B.lib()
    for n in (400, 500):
        s = B.make_stft(2, 100000, 3, 7, n, shift=31)
        sr = ctypes.byref(s)
        for flags in (0, 1):
            assert lib.bhw_stft_fft_f32_device(ref, 16, 0, None, sr, flags, A, Z) == UNSUPPORTED and "power of two" in _err()
            assert lib.bhw_stft_fft_f32_from_table(None, ref, 16, None, sr, flags, A, Z) == UNSUPPORTED and "power of two" in _err()
            assert lib.bhw_spectrogram_f32_device(ref, 16, 0, None, sr, flags, None, A, Z) == UNSUPPORTED and "power of two" in _err()
            assert lib.bhw_spectrogram_f32_from_table(None, ref, 16, None, sr, flags, None, A, Z) == UNSUPPORTED and "power of two" in _err()
        with pytest.raises(B.BhwError):
            B.describe_stft_fft(p, 16, s)
        with pytest.raises(B.BhwError):
            B.describe_spectrogram(p, 16, s)


def test_frames_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    for flags in (0, DETREND, POWER, POWER | DETREND):
        s = _seg(frames=0)
        assert B.lib().bhw_stft_mfft_f32_device(ctypes.byref(p), 320, 0, None, ctypes.byref(s), flags, None, None, None) == OK
        assert "nothing (frames 0)" in B.describe_stft_mfft(p, 320, s, detrend=bool(flags & DETREND), power=bool(flags & POWER))
        # still refused: a size the kernel does not have, a bank of other bins
        assert B.lib().bhw_stft_mfft_f32_device(ctypes.byref(p), 320, 0, None, ctypes.byref(_seg(frames=0, n_fft=512)), flags, None, None, None) == UNSUPPORTED
        assert B.lib().bhw_stft_mfft_f32_device(ctypes.byref(p), 320, 0, None, ctypes.byref(_seg(frames=0, n_fft=420)), flags, None, None, None) == UNSUPPORTED
    fb = _bank(bins=257)
    assert B.lib().bhw_stft_mfft_f32_device(ctypes.byref(p), 320, 0, None, ctypes.byref(_seg(frames=0)), POWER, ctypes.byref(fb), None, None) == BADARG


def test_describe_line_parses():
    p = B.make_params(B.WIN_BH7, 16, 32)
    d = MC.parse(B.describe_stft_mfft(p, 400, _seg(batch=64, samples=160000, frames=998), detrend=True))
    assert d["line"].startswith("stft mfft direct (L = 400, n_fft 400, col0 0, pad 0 constant, constant detrend), spectrum rows, K = 201: "
                                "k_stft_mfft_direct<2>")
    assert (d["signals"], d["frames"], d["rows"], d["m"], d["schedule"]) == (64, 998, 63872, 200, "5x5x4x2")
    assert (d["lpf"], d["fy"], d["cpl"], d["groups"], d["grid"], d["lds"]) == (64, 4, 7, 15968, 2048, 2 * 4 * 200 * 8 + 200 * 8 + 16)
    d = MC.parse(B.describe_stft_mfft(p, 4050, B.make_stft(1, 8192, 3, 2048, 4050, pad=2025, pad_mode=B.PAD_REFLECT, shift=31), power=True))
    assert (d["schedule"], d["lpf"], d["fy"], d["cpl"], d["lds"]) == ("5x5x3x3x3x3", 256, 1, 16, 48604) and d["reflect"] and not d["detrend"]
    assert d["form"] == "power" and "power rows, W = 2026" in d["line"]
    d = MC.parse(B.describe_stft_mfft(p, 320, _seg(), power=True, fbank=_bank()))
    assert d["form"] == "bank" and "bank rows, W = 80 (80 filters, 1000 weights, 2 filters per lane)" in d["line"]
    with pytest.raises(B.BhwError):
        B.describe_stft_mfft(p, 320, _seg(n_fft=512))
    with pytest.raises(B.BhwError):
        B.describe_stft_mfft(p, 320, _seg(), fbank=_bank())                      # a bank without power
    # a short buffer truncates, a missing one is an error
    buf = ctypes.create_string_buffer(16)
    s = _seg()
    assert B.lib().bhw_describe_stft_mfft(None, ctypes.byref(p), 320, ctypes.byref(s), 0, None, buf, 16) == OK and len(buf.value) == 15
    assert B.lib().bhw_describe_stft_mfft(None, ctypes.byref(p), 320, ctypes.byref(s), 0, None, None, 0) == BADARG


def test_python_surface():
    for name in ("stft_mixed", "spectrogram_mixed", "describe_stft_mfft", "mfft_supported", "MFFT_POWER"):
        assert name in bhw.__all__ and hasattr(bhw, name)
    assert list(inspect.signature(bhw.stft_mixed).parameters) == list(inspect.signature(bhw.stft).parameters)
    assert list(inspect.signature(bhw.spectrogram_mixed).parameters) == list(inspect.signature(bhw.spectrogram).parameters)
    for a, b in ((bhw.stft_mixed, bhw.stft), (bhw.spectrogram_mixed, bhw.spectrogram)):
        for name, par in inspect.signature(a).parameters.items():
            assert par.default == inspect.signature(b).parameters[name].default and par.kind == inspect.signature(b).parameters[name].kind
    assert list(inspect.signature(bhw.ResidentTable.stft_mixed).parameters)[1:] == list(inspect.signature(bhw.stft_mixed).parameters)
    assert list(inspect.signature(bhw.ResidentTable.spectrogram_mixed).parameters)[1:] == list(inspect.signature(bhw.spectrogram_mixed).parameters)
    assert "transpose(-1, -2)" in bhw.stft_mixed.__doc__ and "torch.stft" in bhw.stft_mixed.__doc__ and "welch_psd" in bhw.stft_mixed.__doc__
    from blackman_harris_win_amd import selector
    with pytest.raises(ValueError, match="'torch' or 'fused'"):                                  # no new fft= value
        selector._fft_check("mixed")
