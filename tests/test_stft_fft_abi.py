"""The fused window + FFT calls (bhw_stft_fft_f32_device / _from_table / bhw_describe_stft_fft): the checks that need no GPU --
exports and declarations, every refusal of include/bhw.h before any HIP call, frames 0, the describe line and the Python surface."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import stft_fft_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED = 0, -1, -2
NEW_SYMBOLS = ("bhw_stft_fft_f32_device", "bhw_stft_fft_f32_from_table", "bhw_describe_stft_fft")
# never dereferenced: every call below fails or has nothing to do
A, Z = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000)


def _err():
    return B.lib().bhw_last_error().decode()


def _seg(**kw):
    """Welch framing: 4 signals of 16000, window 400 in rows of 512, hop 160, no padding."""
    a = dict(batch=4, samples=16000, frames=98, hop=160, n_fft=512, shift=31)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _calls(s, flags=1, L=400, x=A, Y=Z):
    lib = B.lib()
    return (lambda p: lib.bhw_stft_fft_f32_device(p, L, 0, None, ctypes.byref(s) if s is not None else None, flags, x, Y),
            lambda p: lib.bhw_stft_fft_f32_from_table(None, p, L, None, ctypes.byref(s) if s is not None else None, flags, x, Y))


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert L.bhw_abi_version() == 4 and ctypes.sizeof(B.BhwStft) == 96
    assert "NOT pinned bit" in header                       # the header says the FFT is not a bit-level contract


def test_descriptor_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    K2 = 514
    cases = [
        (dict(struct_size=8), BADARG, "struct_size"),
        (dict(channels=3), BADARG, "channels"),
        (dict(channels=2), UNSUPPORTED, "real input"),
        (dict(batch=0), BADARG, "batch is 0"),
        (dict(hop=0), BADARG, "hop is 0"),
        (dict(n_fft=0), BADARG, "n_fft"),
        (dict(n_fft=256), BADARG, "col0 + L"),
        (dict(n_fft=500), UNSUPPORTED, "power of two"),
        (dict(n_fft=8192), UNSUPPORTED, "power of two"),
        (dict(shift=63), BADARG, "shift"),
        (dict(frames=99), BADARG, "segment 98 leaves the signal"),
        (dict(samples=0), BADARG, "samples is 0"),
        (dict(x_stride=15999), BADARG, "x_stride"),
        (dict(y_stride=K2 - 2), BADARG, "y_stride"),
        (dict(y_stride=K2 + 1), BADARG, "even"),
        (dict(y_batch_stride=97 * K2 + K2 - 2), BADARG, "y_batch_stride"),
        (dict(y_batch_stride=98 * K2 + 1), BADARG, "even"),
        (dict(batch=1 << 20, frames=98), BADARG, "2^34"),
    ]
    for flags in (0, 1):
        for kw, code, text in cases:
            s = _seg(**{k: v for k, v in kw.items() if k != "struct_size"})
            if "struct_size" in kw:
                s.struct_size = kw["struct_size"]
            for call in _calls(s, flags=flags):
                assert call(ref) == code and text in _err(), (flags, kw, _err())
    # with the flag, the restrictions of the segments call
    for kw, text in ((dict(pad=256), "pad 256"), (dict(col0=56), "col0 56"), (dict(pad_mode=B.PAD_REFLECT), "pad_mode 1")):
        for call in _calls(_seg(**kw), flags=1):
            assert call(ref) == BADARG and text in _err(), (kw, _err())
    # without it they are a centred STFT under the frames call's extent rule
    s = _seg(pad=256, col0=56, pad_mode=B.PAD_REFLECT, frames=101)
    assert B.lib().bhw_stft_fft_f32_from_table(None, ref, 400, None, ctypes.byref(s), 0, A, Z) == BADARG and "table is NULL" in _err()
    s = _seg(pad=256, col0=56, pad_mode=B.PAD_REFLECT, frames=102)
    for call in _calls(s, flags=0):
        assert call(ref) == BADARG and "leaves the padded signal" in _err()
    s = _seg(pad=256, pad_mode=B.PAD_REFLECT, samples=200, frames=1)
    for call in _calls(s, flags=0, L=512):
        assert call(ref) == BADARG and "reflect padding" in _err()
    for call in _calls(_seg(pad_mode=7), flags=0):
        assert call(ref) == BADARG and "pad_mode" in _err()
    # the extent rule without padding is the segments' one with and without the flag: 98 segments of 400 fit, rows of 512 would not
    assert 97 * 160 + 512 > 16000 >= 97 * 160 + 400
    for flags in (0, 1):
        assert B.lib().bhw_stft_fft_f32_from_table(None, ref, 400, None, ctypes.byref(_seg()), flags, A, Z) == BADARG
        assert "table is NULL" in _err()                        # every check passed


def test_argument_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    s = _seg()
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
        assert call(ref) == BADARG and "8-byte aligned" in _err()
    for call in _calls(s, x=ctypes.c_void_p(0x10000002)):
        assert call(ref) == BADARG and "4-byte aligned" in _err()
    # d_Y inside x, x inside d_Y, and the first byte behind each: x holds 4 * 16000 floats, Y 4 * 98 * 514
    xb, yb = 4 * 16000 * 4, 4 * 98 * 514 * 4
    for x, Y, bad in ((0x10000000, 0x10000000 + xb - 8, True), (0x10000000, 0x10000000 + xb, False), (0x80000000 + yb - 4, 0x80000000, True),
                      (0x80000000 + yb, 0x80000000, False)):
        # (the from-table call with no table: when every check passes it stops at "table is NULL", before any launch)
        rc = B.lib().bhw_stft_fft_f32_from_table(None, ref, 400, None, ctypes.byref(s), 1, ctypes.c_void_p(x), ctypes.c_void_p(Y))
        assert rc == BADARG and ("overlap" if bad else "table is NULL") in _err(), (hex(x), hex(Y), _err())
        if bad:
            assert B.lib().bhw_stft_fft_f32_device(ref, 400, 0, None, ctypes.byref(s), 1, ctypes.c_void_p(x), ctypes.c_void_p(Y)) == BADARG
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    for call in _calls(s):
        assert call(ctypes.byref(taylor)) == UNSUPPORTED
    assert B.lib().bhw_stft_fft_f32_from_table(None, ref, 400, None, ctypes.byref(s), 1, A, Z) == BADARG and "table is NULL" in _err()


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(768)
    for n in range(1, 8300):
        s = B.make_stft(2, 100000, 3, 7, n, shift=31)
        rc = lib.bhw_describe_stft_fft(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), 1, buf, 768)
        assert rc == (OK if B.fft_supported(n) else UNSUPPORTED), (n, rc, _err())
    assert [n for n in range(1, 8300) if B.fft_supported(n)] == [1 << k for k in range(4, 13)]


def test_frames_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    for flags in (0, 1):
        s = _seg(frames=0)
        assert B.lib().bhw_stft_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, None, None) == OK
        assert "nothing (frames 0)" in B.describe_stft_fft(p, 400, s, detrend=bool(flags))
        # still refused: a size the kernel does not have
        s = _seg(frames=0, n_fft=768)
        assert B.lib().bhw_stft_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, None, None) == UNSUPPORTED


def test_describe_line_parses():
    p = B.make_params(B.WIN_BH7, 16, 32)
    d = FC.parse(B.describe_stft_fft(p, 400, _seg(batch=64, samples=160000, frames=998), detrend=True))
    assert d["line"].startswith("stft fft direct (L = 400, n_fft 512, col0 0, pad 0 constant, constant detrend): k_stft_fft_direct<2>")
    assert (d["signals"], d["frames"], d["rows"], d["m"], d["schedule"]) == (64, 998, 63872, 256, "4x4x4x4")
    assert (d["lpf"], d["fy"], d["cpl"], d["groups"], d["grid"], d["lds"]) == (64, 4, 8, 15968, 2048, 2 * 4 * 256 * 8 + 256 * 8 + 16)
    d = FC.parse(B.describe_stft_fft(p, 4096, B.make_stft(1, 8192, 3, 2048, 4096, pad=2048, pad_mode=B.PAD_REFLECT, shift=31)))
    assert (d["schedule"], d["lpf"], d["fy"], d["cpl"], d["lds"]) == ("4x4x4x4x4x2", 256, 1, 16, 49156) and d["reflect"] and not d["detrend"]
    with pytest.raises(B.BhwError):
        B.describe_stft_fft(p, 400, _seg(n_fft=500))
    # a short buffer truncates, a missing one is an error
    buf = ctypes.create_string_buffer(16)
    s = _seg()
    assert B.lib().bhw_describe_stft_fft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, buf, 16) == OK and len(buf.value) == 15
    assert B.lib().bhw_describe_stft_fft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, None, 0) == BADARG


def test_python_surface():
    for name in ("stft", "describe_stft_fft"):
        assert name in bhw.__all__ and hasattr(bhw, name)
    sig = inspect.signature(bhw.stft)
    assert list(sig.parameters) == ["params", "x", "n_fft", "hop", "win_length", "center", "pad_mode", "detrend", "shift", "out"]
    assert sig.parameters["center"].default is True and sig.parameters["pad_mode"].default == "reflect"
    assert sig.parameters["detrend"].default is False
    assert list(inspect.signature(bhw.ResidentTable.stft).parameters)[1:] == list(sig.parameters)
    assert "transpose(-1, -2)" in bhw.stft.__doc__ and "torch.stft" in bhw.stft.__doc__
    for name in ("welch", "csd", "coherence", "transfer_function", "cross_spectra"):
        for fn in (getattr(bhw, name), getattr(bhw.ResidentTable, name)):
            par = inspect.signature(fn).parameters["fft"]
            assert par.default == "torch" and par.kind is inspect.Parameter.KEYWORD_ONLY, (name, fn)
