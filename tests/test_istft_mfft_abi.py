"""The fused inverse mixed-radix FFT + overlap-add calls (bhw_istft_mfft_f32_device / _from_table / bhw_describe_istft_mfft): the checks
that need no GPU -- exports and declarations, every refusal of include/bhw.h before any HIP call, samples 0, the describe line over
every n_fft, the unchanged refusals of the power-of-two family and the Python surface."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import istft_mfft_cases as XC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED = 0, -1, -2
NEW_SYMBOLS = ("bhw_istft_mfft_f32_device", "bhw_istft_mfft_f32_from_table", "bhw_describe_istft_mfft")
# never dereferenced: every call below fails or has nothing to do
A, Z = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000)


def _err():
    return B.lib().bhw_last_error().decode()


def _desc(**kw):
    """torch.istft's framing: 4 signals, 101 frames of 400 at hop 160, window 400, centred: 16000 samples."""
    a = dict(batch=4, samples=16000, frames=101, hop=160, n_fft=400, col0=0, pad=200, shift=31)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _calls(s, flags=1, L=400, Y=Z, x=A):
    lib = B.lib()
    return (lambda p: lib.bhw_istft_mfft_f32_device(p, L, 0, None, ctypes.byref(s) if s is not None else None, flags, Y, x),
            lambda p: lib.bhw_istft_mfft_f32_from_table(None, p, L, None, ctypes.byref(s) if s is not None else None, flags, Y, x))


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert L.bhw_abi_version() == 4 and ctypes.sizeof(B.BhwStft) == 96
    assert "#define BHW_ABI_VERSION 4u" in header
    assert "c = (float)(1.0 / (double) n_fft)" in header and "one rounding more" in header and "W[i + M] = -W[i]" in header
    assert "The inverse at these lengths is bhw_istft_mfft_f32_*" in header and "calls of its own:\n *     bhw_istft_mfft_f32_*" in header
    assert L.bhw_istft_mfft_f32_device.argtypes == L.bhw_istft_fft_f32_device.argtypes
    assert L.bhw_istft_mfft_f32_from_table.argtypes == L.bhw_istft_fft_f32_from_table.argtypes
    assert L.bhw_describe_istft_mfft.argtypes == L.bhw_describe_istft_fft.argtypes


def test_descriptor_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    K2 = 402
    cases = [
        (dict(struct_size=8), BADARG, "struct_size"),
        (dict(channels=3), BADARG, "channels"),
        (dict(channels=2), UNSUPPORTED, "real output"),
        (dict(batch=0), BADARG, "batch is 0"),
        (dict(hop=0), BADARG, "hop is 0"),
        (dict(n_fft=0), BADARG, "n_fft"),
        (dict(n_fft=250), BADARG, "col0 + L"),
        (dict(n_fft=512, col0=56, pad=256), UNSUPPORTED, "bhw_istft_fft_f32_*"),          # a power of two: the other family, by name
        (dict(n_fft=4096, col0=1848, pad=2048), UNSUPPORTED, "bhw_istft_fft_f32_*"),
        (dict(n_fft=8192, col0=3896, pad=4096), UNSUPPORTED, "power of two"),
        (dict(n_fft=405, col0=2, pad=202), UNSUPPORTED, "even 2^a 3^b 5^c"),                # odd
        (dict(n_fft=420, col0=10, pad=210), UNSUPPORTED, "even 2^a 3^b 5^c"),               # a factor 7
        (dict(n_fft=402, col0=1, pad=201), UNSUPPORTED, "even 2^a 3^b 5^c"),                # a factor 67
        (dict(n_fft=4374, col0=1987, pad=2187), UNSUPPORTED, "16..4095"),                   # 2 * 3^7, above the range
        (dict(n_fft=4800, col0=2200, pad=2400), UNSUPPORTED, "16..4095"),
        (dict(shift=63), BADARG, "shift"),
        (dict(n_fft=480, col0=40, pad=39), BADARG, "pad 39 < col0 40"),
        (dict(frames=0), BADARG, "frames is 0 with samples"),
        (dict(pad_mode=B.PAD_REFLECT), BADARG, "pad_mode 1: the overlap-add takes 0"),
        (dict(samples=(1 << 34) + 1), BADARG, "2^34 per signal"),
        (dict(x_stride=15999), BADARG, "x_stride"),
        (dict(y_stride=K2 - 2), BADARG, "y_stride"),
        (dict(y_stride=K2 + 1), BADARG, "even"),
        (dict(y_batch_stride=100 * K2 + K2 - 2), BADARG, "y_batch_stride"),
        (dict(y_batch_stride=101 * K2 + 1), BADARG, "even"),
        (dict(batch=1 << 20, frames=101), BADARG, "2^34"),
    ]
    for flags in (0, 1):
        for kw, code, text in cases:
            s = _desc(**{k: v for k, v in kw.items() if k != "struct_size"})
            if "struct_size" in kw:
                s.struct_size = kw["struct_size"]
            for call in _calls(s, flags=flags):
                assert call(ref) == code and text in _err(), (flags, kw, _err())
    # below the range: 12 = 2^2 * 3 (a window of 8 in it)
    s = _desc(n_fft=12, col0=2, pad=6)
    for call in _calls(s, L=8):
        assert call(ref) == UNSUPPORTED and "16..4095" in _err(), _err()
    # every check passed: the from-table call stops at the missing table, before any launch
    for flags in (0, 1):
        assert B.lib().bhw_istft_mfft_f32_from_table(None, ref, 400, None, ctypes.byref(_desc()), flags, Z, A) == BADARG
        assert "table is NULL" in _err()


def test_argument_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    s = _desc()
    for flags in (2, 4, 0x80000000):
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
        assert call(ref) == BADARG and "d_Y is not 8-byte aligned" in _err()
    for call in _calls(s, x=ctypes.c_void_p(0x10000002)):
        assert call(ref) == BADARG and "4-byte aligned" in _err()
    # d_Y inside x, x inside d_Y, and the first byte behind each: x holds 4 * 16000 floats, Y 4 * 101 * 402
    xb, yb = 4 * 16000 * 4, 4 * 101 * 402 * 4
    for x, Y, bad in ((0x10000000, 0x10000000 + xb - 8, True), (0x10000000, 0x10000000 + xb, False), (0x80000000 + yb - 4, 0x80000000, True),
                      (0x80000000 + yb, 0x80000000, False)):
        rc = B.lib().bhw_istft_mfft_f32_from_table(None, ref, 400, None, ctypes.byref(s), 1, ctypes.c_void_p(Y), ctypes.c_void_p(x))
        assert rc == BADARG and ("overlap" if bad else "table is NULL") in _err(), (hex(x), hex(Y), _err())
        if bad:
            assert B.lib().bhw_istft_mfft_f32_device(ref, 400, 0, None, ctypes.byref(s), 1, ctypes.c_void_p(Y), ctypes.c_void_p(x)) == BADARG
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    for call in _calls(s):
        assert call(ctypes.byref(taylor)) == UNSUPPORTED


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1024)
    passed = 0
    for n in range(1, 5001):
        s = B.make_stft(2, 1000, 3, 7, n, col0=(n - min(n, 16)) // 2, pad=n // 2, shift=31)
        rc = lib.bhw_describe_istft_mfft(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), 1, buf, 1024)
        assert rc == (OK if B.mfft_supported(n) else UNSUPPORTED), (n, rc, _err())
        if rc == OK:
            passed += 1
            assert not B.fft_supported(n)                          # one transform per n_fft
        elif B.fft_supported(n):
            assert "bhw_istft_fft_f32_*" in _err(), (n, _err())
    assert passed == 95


def test_the_power_of_two_family_still_refuses_these_sizes():
    """bhw_istft_fft_f32_* and bhw.istft at 400 and 500: the code and the message they had before the mixed-radix calls."""
    p = B.make_params(B.WIN_BH4, 24, 32)
    for n in (400, 500):
        s = _desc(n_fft=n, col0=(n - 400) // 2, pad=n // 2, samples=n + 160 * 100 - 2 * (n // 2))
        assert B.lib().bhw_istft_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), 1, Z, A) == UNSUPPORTED
        assert _err().endswith(f"n_fft {n}: the fused inverse FFT takes a power of two in 16..4096"), _err()
        assert B.lib().bhw_istft_fft_f32_from_table(None, ctypes.byref(p), 400, None, ctypes.byref(s), 1, Z, A) == UNSUPPORTED
        with pytest.raises(B.BhwError) as e:
            B.describe_istft_fft(p, 400, s)
        assert e.value.code == UNSUPPORTED and "power of two" in e.value.detail
    src = inspect.getsource(bhw.selector._istft)
    assert 'f"the fused inverse FFT takes n_fft a power of two in {B.FFT_MIN_N}..{B.FFT_MAX_N}, got {n_fft}"' in src


def test_samples_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    for flags in (0, 1):
        for frames in (0, 101):
            s = _desc(samples=0, frames=frames)
            assert B.lib().bhw_istft_mfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, None, None) == OK
            assert "nothing (samples 0)" in B.describe_istft_mfft(p, 400, s, normalize=bool(flags))
        s = _desc(samples=0, n_fft=512, col0=56, pad=256)
        assert B.lib().bhw_istft_mfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, None, None) == UNSUPPORTED


def test_describe_line_parses():
    p = B.make_params(B.WIN_BH7, 16, 32)
    d = XC.parse(B.describe_istft_mfft(p, 400, _desc(batch=64, samples=159520, frames=998), normalize=True))
    assert d["line"].startswith("istft mfft direct (L = 400, n_fft 400, col0 0, pad 200: t0 = 200), normalised by the window envelope: "
                                "k_istft_mfft_direct<2>")
    assert (d["signals"], d["frames"], d["rows"], d["m"], d["schedule"]) == (64, 998, 63872, 200, "5x5x4x2")
    assert (d["lpf"], d["fy"], d["cpl"], d["lds"]) == (64, 4, 7, 2 * 4 * 200 * 8 + 200 * 8 + 400 * 4)
    # S: 64 * 998 rows over 1024 groups of 4 slots; halo: ceil(400 / 160) - 1; the repeats: 2 of every 17 transforms
    assert (d["S"], d["halo"], d["spans"], d["trips"], d["repeated"]) == (15, 2, 67, 17, 11)
    assert (d["groups"], d["grid"]) == (1072, 1072) and not d["heavy"]
    d = XC.parse(B.describe_istft_mfft(p, 4050, B.make_stft(1, 8100, 5, 2025, 4050, pad=2025, shift=31)))
    assert (d["schedule"], d["lpf"], d["fy"], d["cpl"], d["lds"]) == ("5x5x3x3x3x3", 256, 1, 16, 64800) and not d["normalize"]
    # heavy overlap and one short signal: the halo sets S, few workgroups run, and the line says so
    d = XC.parse(B.describe_istft_mfft(p, 1200, B.make_stft(1, 8792, 1100, 8, 1200, pad=600, shift=31), normalize=True))
    assert (d["halo"], d["S"], d["groups"]) == (149, 596, 2) and d["heavy"] and "irfft + istft overlap-add" in d["line"]
    # a short buffer truncates, a missing one is an error
    buf = ctypes.create_string_buffer(16)
    s = _desc()
    assert B.lib().bhw_describe_istft_mfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, buf, 16) == OK and len(buf.value) == 15
    assert B.lib().bhw_describe_istft_mfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, None, 0) == BADARG


def test_python_surface():
    for name in ("istft_mixed", "describe_istft_mfft"):
        assert name in bhw.__all__ and hasattr(bhw, name)
    sig = inspect.signature(bhw.istft_mixed)
    assert list(sig.parameters) == list(inspect.signature(bhw.istft).parameters)
    assert sig.parameters["center"].default is True and sig.parameters["normalize"].default is True and sig.parameters["length"].default is None
    for name in ("win_length", "center", "length", "normalize", "shift", "out"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(bhw.ResidentTable.istft_mixed).parameters)[1:] == list(sig.parameters)
    doc = bhw.istft_mixed.__doc__
    assert "transpose(-1, -2)" in doc and "torch.istft" in doc and "does not reroute" in doc and "fl32(1 / n_fft)" in doc
