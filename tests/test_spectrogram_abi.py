"""The fused spectrogram calls (bhw_spectrogram_f32_device / _from_table / bhw_describe_spectrogram): the checks that need no GPU --
exports and declarations, every refusal of include/bhw.h before any HIP call, frames 0, the describe line and the Python surface."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import spectrogram_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED = 0, -1, -2
NEW_SYMBOLS = ("bhw_spectrogram_f32_device", "bhw_spectrogram_f32_from_table", "bhw_describe_spectrogram")
# never dereferenced: every call below fails or has nothing to do
A, Z = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000)
FIRST, OFFSET, WEIGHT = 0x20000000, 0x20100000, 0x20200000
K = 257


def _err():
    return B.lib().bhw_last_error().decode()


def _seg(**kw):
    """Welch framing: 4 signals of 16000, window 400 in rows of 512, hop 160, no padding."""
    a = dict(batch=4, samples=16000, frames=98, hop=160, n_fft=512, shift=31)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _bank(**kw):
    a = dict(filters=80, bins=K, weights=1000, d_first=FIRST, d_offset=OFFSET, d_weight=WEIGHT)
    a.update(kw)
    fb = B.make_fbank(a["filters"], a["bins"], a["weights"], a["d_first"], a["d_offset"], a["d_weight"])
    if "struct_size" in a:
        fb.struct_size = a["struct_size"]
    if "reserved" in a:
        fb.reserved = a["reserved"]
    return fb


def _calls(s, fb=None, flags=1, L=400, x=A, P=Z):
    lib = B.lib()
    sr = ctypes.byref(s) if s is not None else None
    fr = ctypes.byref(fb) if fb is not None else None
    return (lambda p: lib.bhw_spectrogram_f32_device(p, L, 0, None, sr, flags, fr, x, P),
            lambda p: lib.bhw_spectrogram_f32_from_table(None, p, L, None, sr, flags, fr, x, P))


def _passes(ref, s, fb=None, flags=1, L=400, x=A, P=Z):
    """Every check passed: the from-table call with no table stops at 'table is NULL', before any launch."""
    sr, fr = ctypes.byref(s), ctypes.byref(fb) if fb is not None else None
    rc = B.lib().bhw_spectrogram_f32_from_table(None, ref, L, None, sr, flags, fr, x, P)
    return rc == BADARG and "table is NULL" in _err()


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert L.bhw_abi_version() == 4 and ctypes.sizeof(B.BhwFbank) == 48 and "} bhw_fbank;" in header
    assert "never an access outside d_weight or the power row" in header         # the header states the kernel's memory safety
    for word in ("Not built", "magnitude", "log", "complex input"):
        assert word in header


def test_input_side_errors_are_the_forward_calls():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
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
    ]
    for fb in (None, _bank()):
        for flags in (0, 1):
            for kw, code, text in cases:
                s = _seg(**{k: v for k, v in kw.items() if k != "struct_size"})
                if "struct_size" in kw:
                    s.struct_size = kw["struct_size"]
                for call in _calls(s, fb, flags=flags):
                    assert call(ref) == code and text in _err(), (flags, kw, _err())
            assert _passes(ref, _seg(), fb, flags=flags)
        for kw, text in ((dict(pad=256), "pad 256"), (dict(col0=56), "col0 56"), (dict(pad_mode=B.PAD_REFLECT), "pad_mode 1")):
            for call in _calls(_seg(**kw), fb, flags=1):
                assert call(ref) == BADARG and text in _err(), (kw, _err())
        assert _passes(ref, _seg(pad=256, col0=56, pad_mode=B.PAD_REFLECT, frames=101), fb, flags=0)
        for call in _calls(_seg(pad=256, col0=56, pad_mode=B.PAD_REFLECT, frames=102), fb, flags=0):
            assert call(ref) == BADARG and "leaves the padded signal" in _err()
        for call in _calls(_seg(), fb, flags=2):
            assert call(ref) == BADARG and "flags" in _err()
        for call in _calls(None, fb):
            assert call(ref) == BADARG and "descriptor is NULL" in _err()
        for call in _calls(_seg(), fb):
            assert call(None) == BADARG
        for call in _calls(_seg(), fb, L=0):
            assert call(ref) == BADARG and "length" in _err()
        taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
        for call in _calls(_seg(), fb):
            assert call(ctypes.byref(taylor)) == UNSUPPORTED


def test_output_side_errors_with_w_in_place_of_2k():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    for fb, W in ((None, K), (_bank(), 80), (_bank(filters=4096), 4096)):
        for kw, text in ((dict(y_stride=W - 1), "y_stride"), (dict(y_batch_stride=97 * W + W - 1), "y_batch_stride"),
                         (dict(y_stride=W + 3, y_batch_stride=97 * (W + 3) + W - 1), "y_batch_stride")):
            for call in _calls(_seg(**kw), fb):
                assert call(ref) == BADARG and text in _err(), (kw, _err())
        # no evenness rule: odd strides pass
        assert _passes(ref, _seg(y_stride=W + 3, y_batch_stride=97 * (W + 3) + W), fb)
        assert _passes(ref, _seg(y_stride=W, y_batch_stride=98 * W + 1), fb)
        # batch * frames * W above 2^34
        big = -(-(1 << 34) // (98 * W)) + 1
        for call in _calls(_seg(batch=big), fb):
            assert call(ref) == BADARG and "2^34" in _err(), _err()
        s = _seg()
        for call in _calls(s, fb, x=None):
            assert call(ref) == BADARG and "NULL" in _err()
        for call in _calls(s, fb, P=None):
            assert call(ref) == BADARG and "NULL" in _err()
        for call in _calls(s, fb, P=ctypes.c_void_p(0x80000002)):
            assert call(ref) == BADARG and "d_P is not 4-byte aligned" in _err()
        assert _passes(ref, s, fb, P=ctypes.c_void_p(0x80000004))            # 4-byte alignment is enough
        for call in _calls(s, fb, x=ctypes.c_void_p(0x10000002)):
            assert call(ref) == BADARG and "d_x is not 4-byte aligned" in _err()
        # d_P inside x, x inside d_P, and the first byte behind each: x holds 4 * 16000 floats, P 4 * 98 * W
        xb, pb = 4 * 16000 * 4, 4 * 98 * W * 4
        for x, P, bad in ((0x10000000, 0x10000000 + xb - 4, True), (0x10000000, 0x10000000 + xb, False), (0x80000000 + pb - 4, 0x80000000, True),
                          (0x80000000 + pb, 0x80000000, False)):
            if bad:
                for call in _calls(s, fb, x=ctypes.c_void_p(x), P=ctypes.c_void_p(P)):
                    assert call(ref) == BADARG and "overlap" in _err(), (hex(x), hex(P), _err())
            else:
                assert _passes(ref, s, fb, x=ctypes.c_void_p(x), P=ctypes.c_void_p(P)), (hex(x), hex(P), _err())


def test_bank_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    s = _seg()
    pb = 4 * 98 * 80 * 4                                       # the bytes of P at 0x80000000
    cases = [
        (dict(struct_size=40), "struct_size"), (dict(reserved=1), "reserved"), (dict(filters=0), "filters"), (dict(filters=4097), "filters"),
        (dict(bins=256), "bins"), (dict(bins=258), "bins"), (dict(weights=(1 << 24) + 1), "weights"),
        (dict(d_first=None), "NULL"), (dict(d_offset=None), "NULL"), (dict(d_weight=None), "d_weight is NULL"),
        (dict(d_first=FIRST + 2), "d_first is not 4-byte aligned"), (dict(d_offset=OFFSET + 1), "d_offset is not 4-byte aligned"),
        (dict(d_weight=WEIGHT + 2), "d_weight is not 4-byte aligned"),
        (dict(d_first=0x80000000 - 80 * 4 + 4), "d_first and d_P overlap"), (dict(d_offset=0x80000000 + pb - 4), "d_offset and d_P overlap"),
        (dict(d_weight=0x80000000 + 1000), "d_weight and d_P overlap"),
    ]
    for kw, text in cases:
        for call in _calls(s, _bank(**kw)):
            assert call(ref) == BADARG and text in _err(), (kw, _err())
    for kw in (dict(), dict(weights=1 << 24), dict(weights=0, d_weight=None), dict(filters=1), dict(filters=4096),
               dict(d_first=0x80000000 - 80 * 4), dict(d_offset=0x80000000 + pb), dict(d_weight=0x80000000 - 4000)):
        assert _passes(ref, s, _bank(**kw)), (kw, _err())
    # the describe call checks the bank's fields but not its pointers
    buf = ctypes.create_string_buffer(1024)
    fb = _bank(d_first=None, d_offset=None, d_weight=None)
    assert B.lib().bhw_describe_spectrogram(None, ref, 400, ctypes.byref(s), 1, ctypes.byref(fb), buf, 1024) == OK
    fb = _bank(bins=256)
    assert B.lib().bhw_describe_spectrogram(None, ref, 400, ctypes.byref(s), 1, ctypes.byref(fb), buf, 1024) == BADARG and "bins" in _err()


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1024)
    for n in list(range(1, 300)) + [500, 511, 512, 513, 1024, 2048, 3000, 4096, 4097, 8192]:
        s = B.make_stft(2, 100000, 3, 7, n, shift=31)
        fb = _bank(bins=n // 2 + 1)
        for f in (None, ctypes.byref(fb)):
            rc = lib.bhw_describe_spectrogram(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), 1, f, buf, 1024)
            assert rc == (OK if B.fft_supported(n) else UNSUPPORTED), (n, rc, _err())


def test_frames_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    for fb in (None, _bank(d_first=None, d_offset=None, d_weight=None)):
        fr = ctypes.byref(fb) if fb is not None else None
        for flags in (0, 1):
            s = _seg(frames=0)
            assert B.lib().bhw_spectrogram_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, fr, None, None) == OK
            assert "nothing (frames 0)" in B.describe_spectrogram(p, 400, s, detrend=bool(flags), fbank=fb)
            s = _seg(frames=0, n_fft=768)
            assert B.lib().bhw_spectrogram_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, fr, None, None) == UNSUPPORTED


def test_describe_line_parses():
    p = B.make_params(B.WIN_BH7, 16, 32)
    s = _seg(batch=64, samples=160000, frames=998)
    d = SC.parse(B.describe_spectrogram(p, 400, s, detrend=True))
    assert d["line"].startswith("spectrogram direct (L = 400, n_fft 512, col0 0, pad 0 constant, constant detrend), power mode, W = 257: "
                                "k_spectrogram_direct<2>")
    assert (d["signals"], d["frames"], d["rows"], d["m"], d["schedule"]) == (64, 998, 63872, 256, "4x4x4x4")
    assert (d["lpf"], d["fy"], d["cpl"], d["groups"], d["grid"], d["lds"]) == (64, 4, 8, 15968, 2048, 2 * 4 * 256 * 8 + 256 * 8 + 16)
    d = SC.parse(B.describe_spectrogram(p, 400, s, detrend=True, fbank=_bank(filters=130)))
    assert (d["mode"], d["W"], d["filters"], d["weights"], d["fpl"]) == ("bank", 130, 130, 1000, 3)
    with pytest.raises(B.BhwError):
        B.describe_spectrogram(p, 400, _seg(n_fft=500))
    buf = ctypes.create_string_buffer(16)
    assert B.lib().bhw_describe_spectrogram(None, ctypes.byref(p), 400, ctypes.byref(s), 0, None, buf, 16) == OK and len(buf.value) == 15
    assert B.lib().bhw_describe_spectrogram(None, ctypes.byref(p), 400, ctypes.byref(s), 0, None, None, 0) == BADARG


def test_python_surface():
    for name in ("spectrogram", "FilterBank", "mel_weights", "describe_spectrogram", "make_fbank"):
        assert name in bhw.__all__ and hasattr(bhw, name)
    sig = inspect.signature(bhw.spectrogram)
    assert list(sig.parameters) == ["params", "x", "n_fft", "hop", "win_length", "center", "pad_mode", "detrend", "fbank", "shift", "out"]
    assert sig.parameters["center"].default is True and sig.parameters["pad_mode"].default == "reflect"
    assert sig.parameters["detrend"].default is False and sig.parameters["fbank"].default is None
    assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for n, q in sig.parameters.items() if n not in ("params", "x", "n_fft", "hop"))
    assert list(inspect.signature(bhw.ResidentTable.spectrogram).parameters)[1:] == list(sig.parameters)
    assert "transpose(-1, -2)" in bhw.spectrogram.__doc__
    sig = inspect.signature(bhw.mel_weights)
    assert list(sig.parameters) == ["n_fft", "n_mels", "sample_rate", "f_min", "f_max", "norm", "mel_scale"]
    assert sig.parameters["mel_scale"].default == "htk" and sig.parameters["norm"].default is None
    # the existing fronts keep their signatures
    assert list(inspect.signature(bhw.stft).parameters) == ["params", "x", "n_fft", "hop", "win_length", "center", "pad_mode", "detrend", "shift", "out"]
