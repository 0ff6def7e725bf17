"""The fused window + complex FFT calls for I/Q input (bhw_stft_cfft_f32_device / _from_table / bhw_describe_stft_cfft): the checks
that need no GPU -- exports and declarations, every refusal of include/bhw.h before any HIP call and in the header's order, frames 0,
the describe line, the refusals the real entry points keep, and the Python surface."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from blackman_harris_win_amd import selector as S

import stft_cfft_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED = 0, -1, -2
NEW_SYMBOLS = ("bhw_stft_cfft_f32_device", "bhw_stft_cfft_f32_from_table", "bhw_describe_stft_cfft")
DETREND, POWER, SHIFT = 1, 2, 4
# never dereferenced: every call below fails or has nothing to do
A, Z = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000)


def _err():
    return B.lib().bhw_last_error().decode()


def _seg(**kw):
    """Welch framing of I/Q signals: 4 signals of 16000 complex samples, window 400 in rows of 512, hop 160, no padding."""
    a = dict(batch=4, samples=16000, frames=98, hop=160, n_fft=512, shift=31, channels=2)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _calls(s, flags=DETREND, L=400, x=A, Y=Z):
    lib = B.lib()
    sr = ctypes.byref(s) if s is not None else None
    return (lambda p: lib.bhw_stft_cfft_f32_device(p, L, 0, None, sr, flags, x, Y),
            lambda p: lib.bhw_stft_cfft_f32_from_table(None, p, L, None, sr, flags, x, Y))


def _passes(ref, s, flags=DETREND, L=400, x=A, Y=Z):
    """Every check passed: the from-table call with no table stops at 'table is NULL', before any launch."""
    rc = B.lib().bhw_stft_cfft_f32_from_table(None, ref, L, None, ctypes.byref(s), flags, x, Y)
    return rc == BADARG and "table is NULL" in _err()


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert L.bhw_abi_version() == 4 and ctypes.sizeof(B.BhwStft) == 96
    assert "#define BHW_CFFT_POWER 2u" in header and "#define BHW_CFFT_SHIFT 4u" in header
    assert (B.CFFT_POWER, B.CFFT_SHIFT, B.WELCH_DETREND_CONSTANT) == (POWER, SHIFT, DETREND)
    assert (B.CFFT_MIN_N, B.CFFT_MAX_N) == (16, 2048)
    block = header[header.index("Fused window and complex FFT for interleaved I/Q input"):header.index("#define BHW_CFFT_POWER")]
    # the header says the transform is no bit-level contract, the row is, and why 4096 is out
    for phrase in ("The transform is NOT pinned bit for bit", "The row is pinned bit for bit", "80 KiB of dynamic LDS",
                   "16\n *     complex columns", "Not built", "bhw_stft_fft_f32_*"):
        assert phrase in block, phrase


def test_descriptor_errors_are_the_frames_and_segments_calls():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    cases = [
        (dict(struct_size=8), BADARG, "struct_size"),
        (dict(channels=3), BADARG, "channels 3"),
        (dict(channels=1), UNSUPPORTED, "bhw_stft_fft_f32_*"),
        (dict(batch=0), BADARG, "batch is 0"),
        (dict(hop=0), BADARG, "hop is 0"),
        (dict(n_fft=0), BADARG, "n_fft"),
        (dict(n_fft=256), BADARG, "col0 + L"),
        (dict(n_fft=500), UNSUPPORTED, "power of two"),
        (dict(n_fft=4096), UNSUPPORTED, "power of two in 16..2048"),
        (dict(n_fft=8192), UNSUPPORTED, "power of two"),
        (dict(shift=63), BADARG, "shift"),
        (dict(frames=99), BADARG, "segment 98 leaves the signal"),
        (dict(samples=0), BADARG, "samples is 0"),
        (dict(x_stride=31999), BADARG, "x_stride 31999 < samples * channels = 32000"),
    ]
    for flags in range(8):
        for kw, code, text in cases:
            s = _seg(**{k: v for k, v in kw.items() if k != "struct_size"})
            if "struct_size" in kw:
                s.struct_size = kw["struct_size"]
            for call in _calls(s, flags=flags):
                assert call(ref) == code and text in _err(), (flags, kw, _err())
        assert _passes(ref, _seg(), flags=flags)
        assert _passes(ref, _seg(x_stride=32001), flags=flags)             # an odd signal stride: x is read under the frames call's rule
        assert _passes(ref, _seg(), flags=flags, x=ctypes.c_void_p(0x10000004))
    # with the detrend flag the segments call's restrictions; without it the frames call's padded extent
    for more in (0, POWER, SHIFT, POWER | SHIFT):
        for kw, text in ((dict(pad=256), "pad 256"), (dict(col0=56), "col0 56"), (dict(pad_mode=B.PAD_REFLECT), "pad_mode 1")):
            for call in _calls(_seg(**kw), flags=DETREND | more):
                assert call(ref) == BADARG and text in _err(), (kw, _err())
        assert _passes(ref, _seg(pad=256, col0=56, pad_mode=B.PAD_REFLECT, frames=101), flags=more)
        for call in _calls(_seg(pad=256, col0=56, pad_mode=B.PAD_REFLECT, frames=102), flags=more):
            assert call(ref) == BADARG and "leaves the padded signal" in _err()
        # without padding a row reads its L window columns only: the segments' extent rule, with or without the detrend flag
        assert _passes(ref, _seg(samples=97 * 160 + 400), flags=more) and _passes(ref, _seg(samples=97 * 160 + 400), flags=more | DETREND)
        for call in _calls(_seg(samples=97 * 160 + 399), flags=more):
            assert call(ref) == BADARG and "segment 97 leaves the signal" in _err()
    for call in _calls(None):
        assert call(ref) == BADARG and "descriptor is NULL" in _err()
    for call in _calls(_seg()):
        assert call(None) == BADARG
    for call in _calls(_seg(), L=0):
        assert call(ref) == BADARG and "length" in _err()
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    for call in _calls(_seg()):
        assert call(ctypes.byref(taylor)) == UNSUPPORTED


def test_the_order_of_the_checks():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    # 1 before 2: a descriptor error with an unknown flag bit is the descriptor's; 2 before 3: unknown flags with an unsupported n_fft
    for call in _calls(_seg(hop=0), flags=8):
        assert call(ref) == BADARG and "hop is 0" in _err()
    for call in _calls(_seg(n_fft=4096), flags=8):
        assert call(ref) == BADARG and "flags 0x8" in _err()
    for call in _calls(_seg(channels=1), flags=16 | DETREND):
        assert call(ref) == BADARG and "flags 0x11" in _err()
    for flags in (8, 16, 0x80000000, 8 | DETREND | POWER | SHIFT):
        for call in _calls(_seg(), flags=flags):
            assert call(ref) == BADARG and "flags" in _err() and "BHW_CFFT_POWER" in _err()
    # 3 before 4 and 5: an unsupported size with frames 0, and with a bad stride
    for call in _calls(_seg(n_fft=4096, frames=0)):
        assert call(ref) == UNSUPPORTED
    for call in _calls(_seg(channels=1, y_stride=3)):
        assert call(ref) == UNSUPPORTED
    # 4 before 5: frames 0 with bad strides and NULL pointers is BHW_OK
    dev, tab = _calls(_seg(frames=0, y_stride=3, y_batch_stride=5), x=None, Y=None)
    assert dev(ref) == OK
    assert tab(ref) == BADARG and "table is NULL" in _err()           # every check passed there too
    # 5: strides before pointers, NULL before alignment, alignment before overlap
    for call in _calls(_seg(y_stride=3), x=None, Y=None):
        assert call(ref) == BADARG and "y_stride" in _err()
    for call in _calls(_seg(), x=None, Y=ctypes.c_void_p(0x80000004)):
        assert call(ref) == BADARG and "NULL" in _err()
    for call in _calls(_seg(), x=ctypes.c_void_p(0x80000000), Y=ctypes.c_void_p(0x80000004)):
        assert call(ref) == BADARG and "d_Y is not 8-byte aligned" in _err()


def test_output_side_errors_of_both_forms():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    for flags, W, align in ((DETREND, 1024, 8), (DETREND | SHIFT, 1024, 8), (0, 1024, 8), (DETREND | POWER, 512, 4), (POWER | SHIFT, 512, 4)):
        power = bool(flags & POWER)
        for kw, text in ((dict(y_stride=W - 1), "y_stride"), (dict(y_stride=W - 2), "y_stride"),
                         (dict(y_batch_stride=97 * W + W - 2), "y_batch_stride"),
                         (dict(y_stride=W + 4, y_batch_stride=97 * (W + 4) + W - 2), "y_batch_stride")):
            for call in _calls(_seg(**kw), flags=flags):
                assert call(ref) == BADARG and text in _err(), (kw, _err())
        # the evenness rule is the spectrum form's alone
        for kw, text in ((dict(y_stride=W + 3), "y_stride"), (dict(y_batch_stride=98 * W + 1), "y_batch_stride")):
            if power:
                assert _passes(ref, _seg(**kw), flags=flags), (kw, _err())
            else:
                for call in _calls(_seg(**kw), flags=flags):
                    assert call(ref) == BADARG and text in _err() and "even" in _err(), (kw, _err())
        assert _passes(ref, _seg(y_stride=W + 4, y_batch_stride=97 * (W + 4) + W), flags=flags)
        s = _seg()
        for call in _calls(s, flags=flags, x=None):
            assert call(ref) == BADARG and "NULL" in _err()
        for call in _calls(s, flags=flags, Y=None):
            assert call(ref) == BADARG and "NULL" in _err()
        for call in _calls(s, flags=flags, Y=ctypes.c_void_p(0x80000002)):
            assert call(ref) == BADARG and f"d_Y is not {align}-byte aligned" in _err()
        if power:
            assert _passes(ref, s, flags=flags, Y=ctypes.c_void_p(0x80000004))        # 4-byte alignment is enough for the power rows
        else:
            for call in _calls(s, flags=flags, Y=ctypes.c_void_p(0x80000004)):
                assert call(ref) == BADARG and "d_Y is not 8-byte aligned" in _err()
        for call in _calls(s, flags=flags, x=ctypes.c_void_p(0x10000002)):
            assert call(ref) == BADARG and "d_x is not 4-byte aligned" in _err()
        # d_Y inside x, x inside d_Y, and the first byte behind each: x holds 4 * 16000 * 2 floats, Y 4 * 98 * W
        xb, yb = 4 * 16000 * 2 * 4, 4 * 98 * W * 4
        for x, Y, bad in ((0x10000000, 0x10000000 + xb - 8, True), (0x10000000, 0x10000000 + xb, False), (0x80000000 + yb - 8, 0x80000000, True),
                          (0x80000000 + yb, 0x80000000, False)):
            if bad:
                for call in _calls(s, flags=flags, x=ctypes.c_void_p(x), Y=ctypes.c_void_p(Y)):
                    assert call(ref) == BADARG and "overlap" in _err(), (hex(x), hex(Y), _err())
            else:
                assert _passes(ref, s, flags=flags, x=ctypes.c_void_p(x), Y=ctypes.c_void_p(Y)), (hex(x), hex(Y), _err())
    # batch * frames * n_fft above 2^34
    big = -(-(1 << 34) // (98 * 512)) + 1
    for call in _calls(_seg(batch=big)):
        assert call(ref) == BADARG and "2^34" in _err(), _err()


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1024)
    for n in list(range(1, 300)) + [500, 511, 512, 513, 1024, 2047, 2048, 2049, 3000, 4096, 4097, 8192]:
        s = B.make_stft(2, 100000, 3, 7, n, channels=2, shift=31)
        for flags in range(8):
            rc = lib.bhw_describe_stft_cfft(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), flags, buf, 1024)
            assert rc == (OK if B.cfft_supported(n) else UNSUPPORTED), (n, rc, _err())
    assert [n for n in range(1, 5000) if B.cfft_supported(n)] == [16, 32, 64, 128, 256, 512, 1024, 2048]


def test_frames_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    for flags in range(8):
        s = _seg(frames=0)
        assert B.lib().bhw_stft_cfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, None, None) == OK
        assert "nothing (frames 0)" in B.describe_stft_cfft(p, 400, s, detrend=bool(flags & 1), power=bool(flags & 2), fftshift=bool(flags & 4))
        s = _seg(frames=0, n_fft=768)
        assert B.lib().bhw_stft_cfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, None, None) == UNSUPPORTED


def test_describe_line_parses():
    p = B.make_params(B.WIN_BH7, 16, 32)
    s = _seg(batch=64, samples=160000, frames=998)
    d = CC.parse(B.describe_stft_cfft(p, 400, s, detrend=True))
    assert d["line"].startswith("stft cfft direct (L = 400, n_fft 512, col0 0, pad 0 constant, constant detrend), spectrum rows, bins in order: "
                                "k_stft_cfft_direct<2>")
    assert "complex FFT of 512 points in passes 4x4x4x4x2 (no split)" in d["line"]
    assert (d["signals"], d["frames"], d["rows"], d["m"], d["schedule"]) == (64, 998, 63872, 512, "4x4x4x4x2")
    assert (d["lpf"], d["fy"], d["cpl"], d["groups"], d["grid"], d["lds"]) == (128, 2, 4, 31936, 2048, 2 * 2 * 512 * 8 + 256 * 8 + 16)
    d = CC.parse(B.describe_stft_cfft(p, 400, s, power=True, fftshift=True))
    assert d["power"] and d["shifted"] and not d["detrend"] and "power rows, bins shifted" in d["line"]
    with pytest.raises(B.BhwError):
        B.describe_stft_cfft(p, 400, _seg(n_fft=500))
    buf = ctypes.create_string_buffer(16)
    assert B.lib().bhw_describe_stft_cfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, buf, 16) == OK and len(buf.value) == 15
    assert B.lib().bhw_describe_stft_cfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, None, 0) == BADARG


def test_the_real_entry_points_still_refuse_two_channels():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    lib = B.lib()
    s = _seg()
    sr = ctypes.byref(s)
    calls = (lambda: lib.bhw_stft_fft_f32_device(ref, 400, 0, None, sr, 1, A, Z),
             lambda: lib.bhw_stft_fft_f32_from_table(None, ref, 400, None, sr, 1, A, Z),
             lambda: lib.bhw_spectrogram_f32_device(ref, 400, 0, None, sr, 1, None, A, Z),
             lambda: lib.bhw_spectrogram_f32_from_table(None, ref, 400, None, sr, 1, None, A, Z))
    for call in calls:
        assert call() == UNSUPPORTED and "real input" in _err(), _err()
    o = B.make_stft(4, 16000, 98, 160, 512, shift=31, channels=2, pad=256)
    for call in (lambda: lib.bhw_istft_fft_f32_device(ref, 400, 0, None, ctypes.byref(o), 0, A, Z),
                 lambda: lib.bhw_istft_fft_f32_from_table(None, ref, 400, None, ctypes.byref(o), 0, A, Z)):
        assert call() == UNSUPPORTED and "channels 2" in _err(), _err()


def test_python_surface():
    for name in ("stft_iq", "spectrogram_iq", "describe_stft_cfft"):
        assert name in bhw.__all__ and hasattr(bhw, name)
    want = ["params", "x", "n_fft", "hop", "win_length", "center", "pad_mode", "detrend", "shift", "fftshift", "out"]
    for fn, method in ((bhw.stft_iq, bhw.ResidentTable.stft_iq), (bhw.spectrogram_iq, bhw.ResidentTable.spectrogram_iq)):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == want
        assert sig.parameters["center"].default is True and sig.parameters["pad_mode"].default == "reflect"
        assert sig.parameters["detrend"].default is False and sig.parameters["fftshift"].default is False
        assert sig.parameters["win_length"].default is None and sig.parameters["shift"].default is None and sig.parameters["out"].default is None
        assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for n, q in sig.parameters.items() if n not in ("params", "x", "n_fft", "hop"))
        assert list(inspect.signature(method).parameters)[1:] == want
    assert "transpose(-1, -2)" in bhw.stft_iq.__doc__ and "onesided=False" in bhw.stft_iq.__doc__
    assert "welch_psd(stft_iq(" in bhw.stft_iq.__doc__
    # the existing fronts keep their signatures
    assert list(inspect.signature(bhw.stft).parameters) == ["params", "x", "n_fft", "hop", "win_length", "center", "pad_mode", "detrend", "shift", "out"]
    assert list(inspect.signature(bhw.spectrogram).parameters) == ["params", "x", "n_fft", "hop", "win_length", "center", "pad_mode", "detrend",
                                                                   "fbank", "shift", "out"]


def test_python_value_errors_need_no_device():
    """Every ValueError of stft_iq / spectrogram_iq is raised before the device is looked at: the shared front is called with host
    tensors here (the public functions refuse to start without a HIP device)."""
    torch = pytest.importorskip("torch")
    p = B.make_params(B.WIN_BH7, 16, 32)
    xc = torch.zeros((2, 4000), dtype=torch.complex64)

    def call(x, n_fft, hop, power=False, **kw):
        a = dict(win_length=None, center=True, pad_mode="reflect", detrend=False, shift=None, fftshift=False, out=None)
        a.update(kw)
        return S._stft_iq(torch, p, x, n_fft, hop, a["win_length"], a["center"], a["pad_mode"], a["detrend"], a["shift"], a["fftshift"],
                          a["out"], None, None, power)

    for power in (False, True):
        with pytest.raises(ValueError, match="complex64"):
            call(torch.zeros((2, 4000)), 64, 16, power)
        with pytest.raises(ValueError, match="complex64"):
            call(xc.to(torch.complex128), 64, 16, power)
        with pytest.raises(ValueError, match="complex64"):
            call([0.0] * 100, 64, 16, power)
        for n in (4096, 100, 8):
            with pytest.raises(ValueError, match="power of two in 16..2048"):
                call(xc, n, 4, power)
        with pytest.raises(ValueError, match="center=False"):
            call(xc, 64, 16, power, detrend=True)
        with pytest.raises(ValueError, match="pad_mode"):
            call(xc, 64, 16, power, pad_mode="edge")
        with pytest.raises(ValueError, match="hop"):
            call(xc, 64, 0, power)
        with pytest.raises(ValueError, match=r"\(T,\) or \(B, T\)"):
            call(xc[None], 64, 16, power)
        frames = 1 + 4000 // 16
        good, other = (torch.float32, torch.complex64) if power else (torch.complex64, torch.float32)
        with pytest.raises(ValueError, match="out must be"):
            call(xc, 64, 16, power, out=torch.zeros((2, frames, 64), dtype=other))
        with pytest.raises(ValueError, match="out must be"):
            call(xc, 64, 16, power, out=torch.zeros((2, frames, 33), dtype=good))
        with pytest.raises(ValueError, match="out must be"):
            call(xc, 64, 16, power, out=torch.zeros((2, frames + 1, 64), dtype=good))
        # every check passed: the device is the last thing asked for
        with pytest.raises(ValueError, match="CUDA tensor"):
            call(xc, 64, 16, power, out=torch.zeros((2, frames, 64), dtype=good))
