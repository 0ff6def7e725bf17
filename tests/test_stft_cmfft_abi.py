"""The mixed-radix fused window + complex FFT calls for I/Q input (bhw_stft_cmfft_f32_device / _from_table / bhw_describe_stft_cmfft):
the checks that need no GPU -- exports and declarations, every refusal before any HIP call and in the order of bhw_stft_cfft_f32_*,
the three refusals that name the route that takes the call, frames 0, the describe line, the refusals the four existing fronts keep,
and the Python surface."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from blackman_harris_win_amd import selector as S

import stft_cmfft_cases as XC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED = 0, -1, -2
NEW_SYMBOLS = ("bhw_stft_cmfft_f32_device", "bhw_stft_cmfft_f32_from_table", "bhw_describe_stft_cmfft")
DETREND, POWER, SHIFT = 1, 2, 4
# never dereferenced: every call below fails or has nothing to do
A, Z = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000)


def _err():
    return B.lib().bhw_last_error().decode()


def _seg(**kw):
    """Welch framing of I/Q signals: 4 signals of 16000 complex samples, window 400 in rows of 480, hop 160, no padding."""
    a = dict(batch=4, samples=16000, frames=98, hop=160, n_fft=480, shift=31, channels=2)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _calls(s, flags=DETREND, L=400, x=A, Y=Z):
    lib = B.lib()
    sr = ctypes.byref(s) if s is not None else None
    return (lambda p: lib.bhw_stft_cmfft_f32_device(p, L, 0, None, sr, flags, x, Y),
            lambda p: lib.bhw_stft_cmfft_f32_from_table(None, p, L, None, sr, flags, x, Y))


def _passes(ref, s, flags=DETREND, L=400, x=A, Y=Z):
    """Every check passed: the from-table call with no table stops at 'table is NULL', before any launch."""
    rc = B.lib().bhw_stft_cmfft_f32_from_table(None, ref, L, None, ctypes.byref(s), flags, x, Y)
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
    # no new flag values: the three flags of the power-of-two I/Q calls
    assert "#define BHW_CFFT_POWER 2u" in header and "#define BHW_CFFT_SHIFT 4u" in header and "BHW_CMFFT_" not in header
    assert (B.CFFT_POWER, B.CFFT_SHIFT, B.WELCH_DETREND_CONSTANT) == (POWER, SHIFT, DETREND)
    assert (B.CMFFT_MIN_N, B.CMFFT_MAX_N) == (16, 2047)
    block = header[header.index("Mixed-radix fused window and complex FFT for interleaved I/Q input"):header.index("int bhw_stft_cmfft_f32_device")]
    for phrase in ("The transform is NOT pinned bit for bit", "odd lengths included", "bhw_stft_cfft_f32_*", "bhw_stft_mfft_f32_*",
                   "(k + n_fft / 2) mod n_fft", "Not built", "one transform per n_fft"):
        assert phrase in block, phrase
    # the prototypes are those of the power-of-two I/Q calls word for word
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
        twin = re.search(r"\bint " + name.replace("cmfft", "cfft") + r"\(([^;]*)\);", header).group(1)
        assert " ".join(proto.split()) == " ".join(twin.split()), name
        assert getattr(L, name).argtypes == getattr(L, name.replace("cmfft", "cfft")).argtypes


def test_descriptor_errors_are_the_frames_and_segments_calls():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    cases = [
        (dict(struct_size=8), BADARG, "struct_size"),
        (dict(channels=3), BADARG, "channels 3"),
        (dict(channels=1), UNSUPPORTED, "bhw_stft_mfft_f32_*"),
        (dict(batch=0), BADARG, "batch is 0"),
        (dict(hop=0), BADARG, "hop is 0"),
        (dict(n_fft=0), BADARG, "n_fft"),
        (dict(n_fft=256), BADARG, "col0 + L"),
        (dict(n_fft=512), UNSUPPORTED, "bhw_stft_cfft_f32_*"),
        (dict(n_fft=512), UNSUPPORTED, "one transform per n_fft"),
        (dict(n_fft=4096), UNSUPPORTED, "power of two"),
        (dict(n_fft=420), UNSUPPORTED, "2^a 3^b 5^c in 16..2047"),
        (dict(n_fft=2160), UNSUPPORTED, "2^a 3^b 5^c in 16..2047"),
        (dict(n_fft=4050), UNSUPPORTED, "2^a 3^b 5^c in 16..2047"),
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
        assert _passes(ref, _seg(n_fft=405), flags=flags)                  # an odd n_fft
        assert _passes(ref, _seg(x_stride=32001), flags=flags)             # an odd signal stride: x is read under the frames call's rule
        assert _passes(ref, _seg(), flags=flags, x=ctypes.c_void_p(0x10000004))
    # with the detrend flag the segments call's restrictions; without it the frames call's padded extent
    for more in (0, POWER, SHIFT, POWER | SHIFT):
        for kw, text in ((dict(pad=240), "pad 240"), (dict(col0=40), "col0 40"), (dict(pad_mode=B.PAD_REFLECT), "pad_mode 1")):
            for call in _calls(_seg(**kw), flags=DETREND | more):
                assert call(ref) == BADARG and text in _err(), (kw, _err())
        assert _passes(ref, _seg(pad=240, col0=40, pad_mode=B.PAD_REFLECT, frames=101), flags=more)
        for call in _calls(_seg(pad=240, col0=40, pad_mode=B.PAD_REFLECT, frames=102), flags=more):
            assert call(ref) == BADARG and "leaves the padded signal" in _err()
        # an odd n_fft centred as torch.stft centres it: pad = n_fft // 2 on both sides
        assert _passes(ref, _seg(n_fft=405, pad=202, col0=2, pad_mode=B.PAD_REFLECT, frames=1 + (16000 + 404 - 405) // 160), flags=more)
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
    for n in (512, 420):
        for call in _calls(_seg(n_fft=n), flags=8):
            assert call(ref) == BADARG and "flags 0x8" in _err()
    for call in _calls(_seg(channels=1), flags=16 | DETREND):
        assert call(ref) == BADARG and "flags 0x11" in _err()
    for flags in (8, 16, 0x80000000, 8 | DETREND | POWER | SHIFT):
        for call in _calls(_seg(), flags=flags):
            assert call(ref) == BADARG and "flags" in _err() and "BHW_CFFT_POWER" in _err()
    # within 3: channels before the size (a real call at a power of two is sent to the real mixed-radix route's refusal, not here)
    for call in _calls(_seg(channels=1, n_fft=512)):
        assert call(ref) == UNSUPPORTED and "bhw_stft_mfft_f32_*" in _err()
    # 3 before 4 and 5: the three refusals that name a route, with frames 0 and with a bad stride
    for kw in (dict(n_fft=512), dict(n_fft=420), dict(channels=1)):
        for more in (dict(frames=0), dict(y_stride=3)):
            for call in _calls(_seg(**kw, **more)):
                assert call(ref) == UNSUPPORTED, (kw, more, _err())
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
    for flags, W, align in ((DETREND, 960, 8), (DETREND | SHIFT, 960, 8), (0, 960, 8), (DETREND | POWER, 480, 4), (POWER | SHIFT, 480, 4)):
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
    # an odd n_fft: the power rows may have an odd width, the spectrum rows hold 2 * n_fft floats
    odd = _seg(n_fft=405)
    assert _passes(ref, odd, flags=POWER) and _passes(ref, _seg(n_fft=405, y_stride=405), flags=POWER)
    assert _passes(ref, _seg(n_fft=405, y_stride=810), flags=0)
    for call in _calls(_seg(n_fft=405, y_stride=809), flags=0):
        assert call(ref) == BADARG and "y_stride" in _err()
    # batch * frames * n_fft above 2^34
    big = -(-(1 << 34) // (98 * 480)) + 1
    for call in _calls(_seg(batch=big)):
        assert call(ref) == BADARG and "2^34" in _err(), _err()


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1024)
    sizes = [n for n in range(1, 5000) if B.cmfft_supported(n)]
    assert len(sizes) == 91 and sizes[0] == 18 and sizes[-1] == 2025 and len([n for n in sizes if n % 2]) == 18
    for n in sorted(set(list(range(1, 300)) + sizes + [m + d for m in sizes for d in (-1, 1)] + [2047, 2048, 2049, 2160, 2187, 3000, 4050, 4096])):
        s = B.make_stft(2, 100000, 3, 7, n, channels=2, shift=31)
        for flags in range(8):
            rc = lib.bhw_describe_stft_cmfft(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), flags, buf, 1024)
            assert rc == (OK if n in sizes else UNSUPPORTED), (n, rc, _err())
            if rc and n >= 1 and n & (n - 1) == 0:
                assert "bhw_stft_cfft_f32_*" in _err()
            elif rc:
                assert "2^a 3^b 5^c in 16..2047" in _err()


def test_frames_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    for flags in range(8):
        s = _seg(frames=0)
        assert B.lib().bhw_stft_cmfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, None, None) == OK
        assert "nothing (frames 0)" in B.describe_stft_cmfft(p, 400, s, detrend=bool(flags & 1), power=bool(flags & 2), fftshift=bool(flags & 4))
        for n in (420, 512):
            s = _seg(frames=0, n_fft=n)
            assert B.lib().bhw_stft_cmfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, None, None) == UNSUPPORTED


def test_describe_line_parses():
    p = B.make_params(B.WIN_BH7, 16, 32)
    s = _seg(batch=64, samples=160000, frames=998)
    d = XC.parse(B.describe_stft_cmfft(p, 400, s, detrend=True))
    assert d["line"].startswith("stft cmfft direct (L = 400, n_fft 480, col0 0, pad 0 constant, constant detrend), spectrum rows, bins in order: "
                                "k_stft_cmfft_direct<2>")
    assert "complex FFT of 480 points in passes 5x3x4x4x2 (no split)" in d["line"]
    assert (d["signals"], d["frames"], d["rows"], d["m"], d["schedule"], d["radices"]) == (64, 998, 63872, 480, "5x3x4x4x2", [5, 3, 4, 4, 2])
    assert (d["lpf"], d["fy"], d["cpl"], d["groups"], d["grid"], d["lds"], d["fold"]) == (128, 2, 4, 31936, 2048, 2 * 2 * 480 * 8 + 240 * 8 + 16, 240)
    d = XC.parse(B.describe_stft_cmfft(p, 400, _seg(n_fft=405), power=True, fftshift=True))
    assert d["power"] and d["shifted"] and not d["detrend"] and "power rows, bins shifted" in d["line"]
    assert (d["schedule"], d["fold"], d["lpf"], d["cpl"], d["lds"]) == ("5x3x3x3x3", 405, 128, 4, 2 * 2 * 405 * 8 + 405 * 8 + 16)
    with pytest.raises(B.BhwError):
        B.describe_stft_cmfft(p, 400, _seg(n_fft=512))
    buf = ctypes.create_string_buffer(16)
    assert B.lib().bhw_describe_stft_cmfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, buf, 16) == OK and len(buf.value) == 15
    assert B.lib().bhw_describe_stft_cmfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, None, 0) == BADARG


def test_the_existing_entry_points_still_refuse_what_they_refused():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    lib = B.lib()
    s = _seg()
    sr = ctypes.byref(s)
    # I/Q input at a mixed-radix n_fft: the power-of-two I/Q calls, in their words
    for call in (lambda: lib.bhw_stft_cfft_f32_device(ref, 400, 0, None, sr, 1, A, Z),
                 lambda: lib.bhw_stft_cfft_f32_from_table(None, ref, 400, None, sr, 1, A, Z)):
        assert call() == UNSUPPORTED and "power of two in 16..2048" in _err(), _err()
    # ... and the real mixed-radix calls, in theirs
    for call in (lambda: lib.bhw_stft_mfft_f32_device(ref, 400, 0, None, sr, 1, None, A, Z),
                 lambda: lib.bhw_stft_mfft_f32_from_table(None, ref, 400, None, sr, 1, None, A, Z)):
        assert call() == UNSUPPORTED and "real input" in _err(), _err()
    # an odd n_fft stays out of the real mixed-radix calls
    o = _seg(n_fft=405, channels=1)
    for call in (lambda: lib.bhw_stft_mfft_f32_device(ref, 400, 0, None, ctypes.byref(o), 1, None, A, Z),):
        assert call() == UNSUPPORTED and "even 2^a 3^b 5^c" in _err(), _err()
    # the real power-of-two calls keep refusing two channels
    t = _seg(n_fft=512)
    for call in (lambda: lib.bhw_stft_fft_f32_device(ref, 400, 0, None, ctypes.byref(t), 1, A, Z),
                 lambda: lib.bhw_spectrogram_f32_device(ref, 400, 0, None, ctypes.byref(t), 1, None, A, Z)):
        assert call() == UNSUPPORTED and "real input" in _err(), _err()


def test_python_surface():
    for name in ("stft_iq_mixed", "spectrogram_iq_mixed", "describe_stft_cmfft"):
        assert name in bhw.__all__ and hasattr(bhw, name)
    assert bhw.describe_stft_cmfft is B.describe_stft_cmfft
    for fn, twin, method in ((bhw.stft_iq_mixed, bhw.stft_iq, bhw.ResidentTable.stft_iq_mixed),
                             (bhw.spectrogram_iq_mixed, bhw.spectrogram_iq, bhw.ResidentTable.spectrogram_iq_mixed)):
        assert inspect.signature(fn) == inspect.signature(twin)
        assert list(inspect.signature(method).parameters)[1:] == list(inspect.signature(fn).parameters)
        defaults = [q.default for q in inspect.signature(fn).parameters.values()]
        assert [q.default for q in inspect.signature(method).parameters.values()][1:] == defaults
    assert list(inspect.signature(bhw.stft_iq_mixed).parameters) == ["params", "x", "n_fft", "hop", "win_length", "center", "pad_mode", "detrend",
                                                                     "shift", "fftshift", "out"]
    assert "transpose(-1, -2)" in bhw.stft_iq_mixed.__doc__ and "onesided=False" in bhw.stft_iq_mixed.__doc__
    assert "welch_psd(stft_iq_mixed(" in bhw.stft_iq_mixed.__doc__
    assert [n for n in range(1, 5000) if B.cmfft_supported(n)] == XC.SIZES and len(XC.SIZES) == 91
    # the existing fronts keep their signatures
    assert list(inspect.signature(bhw.stft_iq).parameters) == list(inspect.signature(bhw.stft_iq_mixed).parameters)
    assert list(inspect.signature(bhw.stft_mixed).parameters) == ["params", "x", "n_fft", "hop", "win_length", "center", "pad_mode", "detrend", "shift",
                                                                  "out"]


def test_python_value_errors_need_no_device():
    """Every ValueError of stft_iq_mixed / spectrogram_iq_mixed is raised before the device is looked at: the shared front is called
    with host tensors here (the public functions refuse to start without a HIP device)."""
    torch = pytest.importorskip("torch")
    p = B.make_params(B.WIN_BH7, 16, 32)
    xc = torch.zeros((2, 4000), dtype=torch.complex64)

    def call(x, n_fft, hop, power=False, mixed=True, **kw):
        a = dict(win_length=None, center=True, pad_mode="reflect", detrend=False, shift=None, fftshift=False, out=None)
        a.update(kw)
        return S._stft_iq(torch, p, x, n_fft, hop, a["win_length"], a["center"], a["pad_mode"], a["detrend"], a["shift"], a["fftshift"],
                          a["out"], None, None, power, mixed)

    for power in (False, True):
        with pytest.raises(ValueError, match="complex64"):
            call(torch.zeros((2, 4000)), 100, 16, power)
        with pytest.raises(ValueError, match="complex64"):
            call(xc.to(torch.complex128), 100, 16, power)
        with pytest.raises(ValueError, match="complex64"):
            call([0.0] * 100, 100, 16, power)
        for n in (16, 64, 2048, 4096):
            with pytest.raises(ValueError, match="stft_iq"):
                call(xc, n, 4, power)
        for n in (17, 28, 2160, 4050):
            with pytest.raises(ValueError, match=r"2\^a·3\^b·5\^c in 16..2047"):
                call(xc, n, 4, power)
        with pytest.raises(ValueError, match="center=False"):
            call(xc, 100, 16, power, detrend=True)
        with pytest.raises(ValueError, match="pad_mode"):
            call(xc, 100, 16, power, pad_mode="edge")
        with pytest.raises(ValueError, match="hop"):
            call(xc, 100, 0, power)
        with pytest.raises(ValueError, match=r"\(T,\) or \(B, T\)"):
            call(xc[None], 100, 16, power)
        for n in (100, 75):
            frames = 1 + (4000 + 2 * (n // 2) - n) // 16
            good, other = (torch.float32, torch.complex64) if power else (torch.complex64, torch.float32)
            with pytest.raises(ValueError, match="out must be"):
                call(xc, n, 16, power, out=torch.zeros((2, frames, n), dtype=other))
            with pytest.raises(ValueError, match="out must be"):
                call(xc, n, 16, power, out=torch.zeros((2, frames, n // 2 + 1), dtype=good))
            with pytest.raises(ValueError, match="out must be"):
                call(xc, n, 16, power, out=torch.zeros((2, frames + 1, n), dtype=good))
            # every check passed: the device is the last thing asked for
            with pytest.raises(ValueError, match="CUDA tensor"):
                call(xc, n, 16, power, out=torch.zeros((2, frames, n), dtype=good))
        # the power-of-two I/Q front keeps its message
        with pytest.raises(ValueError, match="power of two in 16..2048"):
            call(xc, 100, 16, power, mixed=False)
    # the real mixed-radix front refuses complex input and an odd n_fft as before (its checks start at the device: the GPU file
    # holds its words)
    with pytest.raises(ValueError):
        S._stft_mixed(torch, p, xc, 100, 16, None, True, "reflect", False, False, None, None, None, None, None)
    assert not B.mfft_supported(75) and B.mfft_supported(100)
