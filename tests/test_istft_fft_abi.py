"""The fused inverse FFT + overlap-add calls (bhw_istft_fft_f32_device / _from_table / bhw_describe_istft_fft): the checks that need no
GPU -- exports and declarations, every refusal of include/bhw.h before any HIP call, samples 0, the describe line and the Python
surface."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import istft_fft_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED = 0, -1, -2
NEW_SYMBOLS = ("bhw_istft_fft_f32_device", "bhw_istft_fft_f32_from_table", "bhw_describe_istft_fft")
# never dereferenced: every call below fails or has nothing to do
A, Z = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000)


def _err():
    return B.lib().bhw_last_error().decode()


def _desc(**kw):
    """torch.istft's framing: 4 signals, 101 frames of 512 at hop 160, window 400, centred: 16000 samples."""
    a = dict(batch=4, samples=16000, frames=101, hop=160, n_fft=512, col0=56, pad=256, shift=31)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _calls(s, flags=1, L=400, Y=Z, x=A):
    lib = B.lib()
    return (lambda p: lib.bhw_istft_fft_f32_device(p, L, 0, None, ctypes.byref(s) if s is not None else None, flags, Y, x),
            lambda p: lib.bhw_istft_fft_f32_from_table(None, p, L, None, ctypes.byref(s) if s is not None else None, flags, Y, x))


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert L.bhw_abi_version() == 4 and ctypes.sizeof(B.BhwStft) == 96
    assert "The inverse is bhw_istft_fft_f32_*" in header and "ASCENDING f" in header
    assert L.bhw_istft_fft_f32_device.argtypes == L.bhw_stft_fft_f32_device.argtypes
    assert L.bhw_istft_fft_f32_from_table.argtypes == L.bhw_stft_fft_f32_from_table.argtypes
    assert L.bhw_describe_istft_fft.argtypes == L.bhw_describe_stft_fft.argtypes


def test_descriptor_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    K2 = 514
    cases = [
        (dict(struct_size=8), BADARG, "struct_size"),
        (dict(channels=3), BADARG, "channels"),
        (dict(channels=2), UNSUPPORTED, "real output"),
        (dict(batch=0), BADARG, "batch is 0"),
        (dict(hop=0), BADARG, "hop is 0"),
        (dict(n_fft=0), BADARG, "n_fft"),
        (dict(n_fft=256), BADARG, "col0 + L"),
        (dict(n_fft=500, col0=50), UNSUPPORTED, "power of two"),
        (dict(n_fft=8192), UNSUPPORTED, "power of two"),
        (dict(shift=63), BADARG, "shift"),
        (dict(pad=55), BADARG, "pad 55 < col0 56"),
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
    # every check passed: the from-table call stops at the missing table, before any launch
    for flags in (0, 1):
        assert B.lib().bhw_istft_fft_f32_from_table(None, ref, 400, None, ctypes.byref(_desc()), flags, Z, A) == BADARG
        assert "table is NULL" in _err()


def test_argument_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    s = _desc()
    for call in _calls(s, flags=2):
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
    # d_Y inside x, x inside d_Y, and the first byte behind each: x holds 4 * 16000 floats, Y 4 * 101 * 514
    xb, yb = 4 * 16000 * 4, 4 * 101 * 514 * 4
    for x, Y, bad in ((0x10000000, 0x10000000 + xb - 8, True), (0x10000000, 0x10000000 + xb, False), (0x80000000 + yb - 4, 0x80000000, True),
                      (0x80000000 + yb, 0x80000000, False)):
        rc = B.lib().bhw_istft_fft_f32_from_table(None, ref, 400, None, ctypes.byref(s), 1, ctypes.c_void_p(Y), ctypes.c_void_p(x))
        assert rc == BADARG and ("overlap" if bad else "table is NULL") in _err(), (hex(x), hex(Y), _err())
        if bad:
            assert B.lib().bhw_istft_fft_f32_device(ref, 400, 0, None, ctypes.byref(s), 1, ctypes.c_void_p(Y), ctypes.c_void_p(x)) == BADARG
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    for call in _calls(s):
        assert call(ctypes.byref(taylor)) == UNSUPPORTED


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1024)
    for n in range(1, 8300):
        s = B.make_stft(2, 1000, 3, 7, n, pad=n // 2, shift=31)
        rc = lib.bhw_describe_istft_fft(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), 1, buf, 1024)
        assert rc == (OK if B.fft_supported(n) else UNSUPPORTED), (n, rc, _err())


def test_samples_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    for flags in (0, 1):
        for frames in (0, 101):
            s = _desc(samples=0, frames=frames)
            assert B.lib().bhw_istft_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, None, None) == OK
            assert "nothing (samples 0)" in B.describe_istft_fft(p, 400, s, normalize=bool(flags))
        s = _desc(samples=0, n_fft=768, col0=184, pad=384)
        assert B.lib().bhw_istft_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, None, None) == UNSUPPORTED


def test_describe_line_parses():
    p = B.make_params(B.WIN_BH7, 16, 32)
    d = IC.parse(B.describe_istft_fft(p, 400, _desc(batch=64, samples=159520, frames=998), normalize=True))
    assert d["line"].startswith("istft fft direct (L = 400, n_fft 512, col0 56, pad 256: t0 = 200), normalised by the window envelope: "
                                "k_istft_fft_direct<2>")
    assert (d["signals"], d["frames"], d["rows"], d["m"], d["schedule"]) == (64, 998, 63872, 256, "4x4x4x4")
    assert (d["lpf"], d["fy"], d["cpl"], d["lds"]) == (64, 4, 8, 2 * 4 * 256 * 8 + 256 * 8 + 512 * 4)
    # S: 64 * 998 rows over 1024 groups of 4 slots; halo: ceil(400 / 160) - 1; the repeats: 2 of every 17 transforms
    assert (d["S"], d["halo"], d["spans"], d["trips"], d["repeated"]) == (15, 2, 67, 17, 11)
    assert (d["groups"], d["grid"]) == (1072, 1072) and not d["heavy"]
    d = IC.parse(B.describe_istft_fft(p, 4096, B.make_stft(1, 8192, 5, 2048, 4096, pad=2048, shift=31)))
    assert (d["schedule"], d["lpf"], d["fy"], d["cpl"], d["lds"]) == ("4x4x4x4x4x2", 256, 1, 16, 65536) and not d["normalize"]
    # heavy overlap and one short signal: the halo sets S, few workgroups run, and the line says so
    d = IC.parse(B.describe_istft_fft(p, 2048, B.make_stft(1, 34000, 2126, 16, 2048, pad=1024, shift=31), normalize=True))
    assert (d["halo"], d["S"], d["groups"]) == (127, 508, 5) and d["heavy"] and "irfft + istft overlap-add" in d["line"]
    with pytest.raises(B.BhwError):
        B.describe_istft_fft(p, 400, _desc(n_fft=500, col0=50))
    # a short buffer truncates, a missing one is an error
    buf = ctypes.create_string_buffer(16)
    s = _desc()
    assert B.lib().bhw_describe_istft_fft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, buf, 16) == OK and len(buf.value) == 15
    assert B.lib().bhw_describe_istft_fft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, None, 0) == BADARG


def test_python_surface():
    for name in ("istft", "describe_istft_fft"):
        assert name in bhw.__all__ and hasattr(bhw, name)
    sig = inspect.signature(bhw.istft)
    assert list(sig.parameters) == ["params", "Y", "n_fft", "hop", "win_length", "center", "length", "normalize", "shift", "out"]
    assert sig.parameters["center"].default is True and sig.parameters["normalize"].default is True and sig.parameters["length"].default is None
    for name in ("win_length", "center", "length", "normalize", "shift", "out"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(bhw.ResidentTable.istft).parameters)[1:] == list(sig.parameters)
    assert list(inspect.signature(bhw.istft_overlap_add).parameters)[2:] == list(sig.parameters)[2:]
    assert "transpose(-1, -2)" in bhw.istft.__doc__ and "torch.istft" in bhw.istft.__doc__ and "does not reroute" in bhw.istft.__doc__
