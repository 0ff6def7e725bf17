"""The fused inverse mixed-radix complex FFT + overlap-add calls for I/Q output (bhw_istft_cmfft_f32_device / _from_table /
bhw_describe_istft_cmfft): the checks that need no GPU -- exports and declarations, every refusal of include/bhw.h before any HIP call
and the order of the checks, samples 0, the describe sweep against B.cmfft_supported, the refusals the three older inverse fronts
keep, the describe line and the Python surface with host tensors."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from blackman_harris_win_amd import selector as S

import istft_cmfft_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED = 0, -1, -2
NEW_SYMBOLS = ("bhw_istft_cmfft_f32_device", "bhw_istft_cmfft_f32_from_table", "bhw_describe_istft_cmfft")
# never dereferenced: every call below fails or has nothing to do
A, Z = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000)


def _err():
    return B.lib().bhw_last_error().decode()


def _desc(**kw):
    """torch.istft's framing of complex signals: 4 signals, 101 frames of 600 at hop 160, window 400, centred: 16000 samples."""
    a = dict(batch=4, samples=16000, frames=101, hop=160, n_fft=600, col0=100, pad=300, shift=31, channels=2)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _calls(s, flags=1, L=400, Y=Z, x=A, route="cmfft"):
    lib = B.lib()
    dev, tab = getattr(lib, f"bhw_istft_{route}_f32_device"), getattr(lib, f"bhw_istft_{route}_f32_from_table")
    return (lambda p: dev(p, L, 0, None, ctypes.byref(s) if s is not None else None, flags, Y, x),
            lambda p: tab(None, p, L, None, ctypes.byref(s) if s is not None else None, flags, Y, x))


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert L.bhw_abi_version() == 4 and ctypes.sizeof(B.BhwStft) == 96
    own = header[header.index("Fused inverse mixed-radix complex FFT"):]
    own = own[:own.index("int bhw_describe_istft_cmfft")]
    assert "(float)(1.0 / (double) n_fft)" in own and "one rounding more" in own and "swap(DFT(swap(Y)))" in own
    assert "(k + n_fft / 2) mod n_fft with integer division" in own and "91\n *     sizes, 18 of them odd" in own
    assert L.bhw_istft_cmfft_f32_device.argtypes == L.bhw_istft_cfft_f32_device.argtypes
    assert L.bhw_istft_cmfft_f32_from_table.argtypes == L.bhw_istft_cfft_f32_from_table.argtypes
    assert L.bhw_describe_istft_cmfft.argtypes == L.bhw_describe_istft_cfft.argtypes


def test_descriptor_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    W = 1200
    cases = [
        (dict(struct_size=8), BADARG, "struct_size"),
        (dict(channels=3), BADARG, "channels"),
        (dict(channels=1), UNSUPPORTED, "bhw_istft_mfft_f32_*"),
        (dict(batch=0), BADARG, "batch is 0"),
        (dict(hop=0), BADARG, "hop is 0"),
        (dict(n_fft=0), BADARG, "n_fft"),
        (dict(n_fft=300), BADARG, "col0 + L"),
        (dict(n_fft=512, col0=56, pad=256), UNSUPPORTED, "power of two: bhw_istft_cfft_f32_*"),
        (dict(n_fft=4096), UNSUPPORTED, "power of two: bhw_istft_cfft_f32_*"),
        (dict(n_fft=8, col0=0, pad=4), UNSUPPORTED, "power of two: bhw_istft_cfft_f32_*"),
        (dict(n_fft=700, col0=100, pad=350), UNSUPPORTED, "2^a 3^b 5^c in 16..2047"),
        (dict(n_fft=2160, col0=100, pad=1080), UNSUPPORTED, "2^a 3^b 5^c in 16..2047"),
        (dict(n_fft=15, col0=0, pad=7), UNSUPPORTED, "2^a 3^b 5^c in 16..2047"),
        (dict(shift=63), BADARG, "shift"),
        (dict(pad=99), BADARG, "pad 99 < col0 100"),
        (dict(frames=0), BADARG, "frames is 0 with samples"),
        (dict(pad_mode=B.PAD_REFLECT), BADARG, "pad_mode 1: the overlap-add takes 0"),
        (dict(samples=(1 << 34) + 1), BADARG, "2^34 per signal"),
        (dict(x_stride=31999), BADARG, "x_stride"),
        (dict(y_stride=W - 2), BADARG, "y_stride"),
        (dict(y_stride=W + 1), BADARG, "even"),
        (dict(y_batch_stride=100 * W + W - 2), BADARG, "y_batch_stride"),
        (dict(y_batch_stride=101 * W + 1), BADARG, "even"),
        (dict(batch=1 << 20, frames=101), BADARG, "2^34"),
    ]
    for flags in (0, 1, 4, 5):
        for kw, code, text in cases:
            L = 8 if kw.get("n_fft") in (8, 15) else 400
            s = _desc(**{k: v for k, v in kw.items() if k != "struct_size"})
            if "struct_size" in kw:
                s.struct_size = kw["struct_size"]
            for call in _calls(s, flags=flags, L=L):
                assert call(ref) == code and text in _err(), (flags, kw, _err())
    # an odd x_stride from 2 * samples is no error: every check passed, and the from-table call stops at the missing table, before any
    # launch
    for flags in (0, 1, 4, 5):
        for s in (_desc(), _desc(x_stride=32001), _desc(y_stride=W + 6, y_batch_stride=101 * (W + 6) + 10)):
            assert B.lib().bhw_istft_cmfft_f32_from_table(None, ref, 400, None, ctypes.byref(s), flags, Z, A) == BADARG
            assert "table is NULL" in _err()


def test_the_order_of_the_checks():
    """The order of bhw_istft_cfft_f32_*: the overlap-add's checks on the packed descriptor, unknown flag bits, the unsupported channels
    and n_fft, samples 0, the stride rules, the pointers, the table."""
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    bad = ctypes.c_void_p(0x80000004)
    # everything wrong at once, then one error fewer at every step
    steps = [
        (dict(hop=0, channels=1, n_fft=700, col0=0, pad=350, y_stride=7), 8, None, "hop is 0", BADARG),
        (dict(channels=1, n_fft=700, col0=0, pad=350, y_stride=7), 8, None, "flags 0x8", BADARG),
        (dict(channels=1, n_fft=700, col0=0, pad=350, y_stride=7), 5, None, "channels 1", UNSUPPORTED),
        (dict(n_fft=700, col0=0, pad=350, y_stride=7), 5, None, "n_fft 700", UNSUPPORTED),
        (dict(n_fft=512, col0=0, pad=256, y_stride=7), 5, None, "n_fft 512 is a power of two", UNSUPPORTED),
        (dict(y_stride=7), 5, None, "y_stride 7", BADARG),
        (dict(y_batch_stride=7), 5, None, "y_batch_stride 7", BADARG),
        (dict(), 5, None, "NULL", BADARG),
        (dict(), 5, bad, "8-byte aligned", BADARG),
        (dict(), 5, A, "overlap", BADARG),
    ]
    for kw, flags, Y, text, code in steps:
        s = _desc(**kw)
        for call in _calls(s, flags=flags, Y=Y, x=A):
            assert call(ref) == code and text in _err(), (kw, flags, _err())
    assert B.lib().bhw_istft_cmfft_f32_from_table(None, ref, 400, None, ctypes.byref(_desc()), 5, Z, A) == BADARG and "table is NULL" in _err()
    # samples 0 comes after the flags and the unsupported sizes and before the strides and the pointers
    s = _desc(samples=0, y_stride=7)
    device, from_table = _calls(s, flags=5, Y=None, x=None)
    assert device(ref) == OK
    assert from_table(ref) == BADARG and "table is NULL" in _err()         # every check passed
    for call in _calls(s, flags=8, Y=None, x=None):
        assert call(ref) == BADARG and "flags" in _err()
    for call in _calls(_desc(samples=0, channels=1), flags=5, Y=None, x=None):
        assert call(ref) == UNSUPPORTED


def test_argument_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    s = _desc()
    for flags in (2, 3, 8, 16, 1 << 31):
        for call in _calls(s, flags=flags):
            assert call(ref) == BADARG and "flags" in _err() and "BHW_OLA_NORMALIZE, BHW_CFFT_SHIFT" in _err(), flags
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
    # x one float off the 8-byte grid is no error
    assert B.lib().bhw_istft_cmfft_f32_from_table(None, ref, 400, None, ctypes.byref(s), 1, Z, ctypes.c_void_p(0x10000004)) == BADARG
    assert "table is NULL" in _err()
    # d_Y inside x, x inside d_Y, and the first byte behind each: x holds 4 * 2 * 16000 floats, Y 4 * 101 * 1200
    xb, yb = 4 * 2 * 16000 * 4, 4 * 101 * 1200 * 4
    for x, Y, bad in ((0x10000000, 0x10000000 + xb - 8, True), (0x10000000, 0x10000000 + xb, False), (0x80000000 + yb - 4, 0x80000000, True),
                      (0x80000000 + yb, 0x80000000, False)):
        rc = B.lib().bhw_istft_cmfft_f32_from_table(None, ref, 400, None, ctypes.byref(s), 1, ctypes.c_void_p(Y), ctypes.c_void_p(x))
        assert rc == BADARG and ("overlap" if bad else "table is NULL") in _err(), (hex(x), hex(Y), _err())
        if bad:
            assert B.lib().bhw_istft_cmfft_f32_device(ref, 400, 0, None, ctypes.byref(s), 1, ctypes.c_void_p(Y), ctypes.c_void_p(x)) == BADARG
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    for call in _calls(s):
        assert call(ctypes.byref(taylor)) == UNSUPPORTED


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1024)
    took = []
    for n in range(1, 5001):
        s = B.make_stft(2, 1000, 3, 7, n, pad=n // 2, channels=2, shift=31)
        rc = lib.bhw_describe_istft_cmfft(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), 5, buf, 1024)
        assert rc == (OK if B.cmfft_supported(n) else UNSUPPORTED), (n, rc, _err())
        if rc == OK:
            took.append(n)
            assert buf.value.decode().startswith("istft cmfft direct"), buf.value
        elif n & (n - 1) == 0:
            assert "bhw_istft_cfft_f32_*" in _err(), (n, _err())
        else:
            assert "2^a 3^b 5^c in 16..2047" in _err(), (n, _err())
    assert len(took) == 91 and sum(n % 2 for n in took) == 18 and took[:5] == [18, 20, 24, 25, 27] and took[-2:] == [2000, 2025]


def test_samples_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    for flags in (0, 1, 4, 5):
        for frames in (0, 101):
            s = _desc(samples=0, frames=frames)
            assert B.lib().bhw_istft_cmfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, None, None) == OK
            line = B.describe_istft_cmfft(p, 400, s, normalize=bool(flags & 1), fftshift=bool(flags & 4))
            assert line.startswith("istft cmfft direct") and "nothing (samples 0)" in line
        s = _desc(samples=0, n_fft=512, col0=56, pad=256)
        assert B.lib().bhw_istft_cmfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, None, None) == UNSUPPORTED


def test_the_older_inverse_fronts_keep_their_refusals():
    """bhw_istft_cfft_f32_* still refuses 1536 in its own words, bhw_istft_mfft_f32_* and bhw_istft_fft_f32_* still refuse channels 2,
    and their Python fronts keep their messages."""
    torch = pytest.importorskip("torch")
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    s = _desc(n_fft=1536, col0=568, pad=768)
    for call in _calls(s, route="cfft"):
        assert call(ref) == UNSUPPORTED and "n_fft 1536: the fused inverse complex FFT takes a power of two in 16..2048" in _err()
    for call in _calls(s, route="mfft"):
        assert call(ref) == UNSUPPORTED and "channels 2: the mixed-radix fused inverse FFT gives real output (1)" in _err()
    for call in _calls(s, route="fft"):
        assert call(ref) == UNSUPPORTED and "real output" in _err()
    for call in _calls(_desc(channels=1), flags=4, route="mfft"):
        assert call(ref) == BADARG and "flags" in _err()
    Y = torch.zeros(2, 3, 1536, dtype=torch.complex64)
    with pytest.raises(ValueError, match="the fused inverse complex FFT takes n_fft a power of two in 16..2048, got 1536"):
        S._istft(torch, p, Y, 1536, 384, None, True, None, True, None, None, None, None, S._icfft_input, torch.complex64, False)
    with pytest.raises(ValueError, match="Y rows hold 1536 bins, n_fft // 2 \\+ 1 is 769"):
        S._istft(torch, p, Y, 1536, 384, None, True, None, True, None, None, None, None, S._imfft_input)
    with pytest.raises(ValueError, match="CUDA tensor"):
        S._istft(torch, p, Y, 1536, 384, None, True, None, True, None, None, None, None)


def test_describe_line_parses():
    p = B.make_params(B.WIN_BH7, 16, 32)
    d = IC.parse(B.describe_istft_cmfft(p, 400, _desc(batch=64, samples=159520, frames=998), normalize=True))
    assert d["line"].startswith("istft cmfft direct (L = 400, n_fft 600, col0 100, pad 300: t0 = 200), normalised by the window envelope, "
                                "bins in order: k_istft_cmfft_direct<2>")
    assert (d["signals"], d["frames"], d["rows"], d["m"], d["schedule"], d["fold"]) == (64, 998, 63872, 600, "5x5x3x4x2", 300)
    assert (d["lpf"], d["fy"], d["cpl"], d["lds"]) == (256, 1, 3, 2 * 600 * 8 + 300 * 8 + 600 * 4)
    assert d["halo"] == 2 and not d["heavy"] and "(no split)" in d["line"]
    d = IC.parse(B.describe_istft_cmfft(p, 2025, B.make_stft(1, 8100, 9, 1012, 2025, pad=1012, channels=2, shift=31), fftshift=True))
    assert (d["schedule"], d["lpf"], d["fy"], d["cpl"], d["lds"], d["fold"]) == ("5x5x3x3x3x3", 256, 1, 8, 56700, 2025)
    assert not d["normalize"] and d["shifted"]
    d = IC.parse(B.describe_istft_cmfft(p, 2000, B.make_stft(1, 8000, 9, 1000, 2000, pad=1000, channels=2, shift=31)))
    assert (d["lds"], d["fold"]) == (48000, 1000)
    # heavy overlap and one short signal: the halo sets S, few workgroups run, and the line says so
    d = IC.parse(B.describe_istft_cmfft(p, 2000, B.make_stft(1, 34000, 2126, 16, 2000, pad=1000, channels=2, shift=31), normalize=True))
    assert d["halo"] == 124 and d["S"] == 4 * 124 and d["heavy"] and "ifft + istft overlap-add" in d["line"]
    with pytest.raises(B.BhwError):
        B.describe_istft_cmfft(p, 400, _desc(n_fft=512, col0=56, pad=256))
    # a short buffer truncates, a missing one is an error
    buf = ctypes.create_string_buffer(16)
    s = _desc()
    assert B.lib().bhw_describe_istft_cmfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, buf, 16) == OK and len(buf.value) == 15
    assert B.lib().bhw_describe_istft_cmfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, None, 0) == BADARG


def test_python_surface():
    for name in ("istft_iq_mixed", "describe_istft_cmfft"):
        assert name in bhw.__all__ and hasattr(bhw, name)
    assert bhw.describe_istft_cmfft is B.describe_istft_cmfft
    sig = inspect.signature(bhw.istft_iq_mixed)
    assert sig == inspect.signature(bhw.istft_iq)
    assert list(sig.parameters) == ["params", "Y", "n_fft", "hop", "win_length", "center", "length", "normalize", "shift", "fftshift", "out"]
    for name in ("win_length", "center", "length", "normalize", "shift", "fftshift", "out"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(bhw.ResidentTable.istft_iq_mixed).parameters)[1:] == list(sig.parameters)
    doc = bhw.istft_iq_mixed.__doc__
    assert "stft_iq_mixed" in doc and "fl32(1 / n_fft)" in doc and "does not" in doc and "reroute to it" in doc and "odd" in doc


def test_python_value_errors_need_no_device():
    """Every ValueError of istft_iq_mixed is raised before the device is looked at: the shared body is called with host tensors here
    (the public functions refuse to start without a HIP device), which reach all of them, and a good host tensor reaches the device
    check last."""
    torch = pytest.importorskip("torch")
    p = B.make_params(B.WIN_BH4, 24, 32)
    Y = torch.zeros(2, 11, 600, dtype=torch.complex64)
    bad = [
        (dict(Y=torch.zeros(2, 11, 600)), "complex64"),
        (dict(Y=torch.zeros(2, 11, 600, dtype=torch.complex128)), "complex64"),
        (dict(Y=[1, 2, 3]), "complex64"),
        (dict(Y=torch.zeros(600, dtype=torch.complex64)), r"\(frames, n_fft\)"),
        (dict(Y=torch.zeros(2, 11, 301, dtype=torch.complex64)), "301 bins"),
        (dict(Y=torch.zeros(2, 0, 600, dtype=torch.complex64)), "zero frames"),
        (dict(n_fft=512, Y=torch.zeros(2, 3, 512, dtype=torch.complex64)), "power of two: bhw.istft_iq"),
        (dict(n_fft=4096, Y=torch.zeros(2, 3, 4096, dtype=torch.complex64)), "2\\^a 3\\^b 5\\^c in 16..2047"),
        (dict(n_fft=700, Y=torch.zeros(2, 3, 700, dtype=torch.complex64)), "2\\^a 3\\^b 5\\^c in 16..2047"),
        (dict(n_fft=2160, Y=torch.zeros(2, 3, 2160, dtype=torch.complex64)), "2\\^a 3\\^b 5\\^c in 16..2047"),
        (dict(n_fft=15, Y=torch.zeros(2, 3, 15, dtype=torch.complex64)), "2\\^a 3\\^b 5\\^c in 16..2047"),
        (dict(hop=0), "hop"),
        (dict(center=False, win_length=400), "center=False"),
        (dict(length=-1), "length"),
        (dict(out=torch.zeros(2, 1600)), "out must be"),
        (dict(out=torch.zeros(2, 1601, dtype=torch.complex64)), "out must be"),
        (dict(out=torch.zeros(1600, 2, dtype=torch.complex64).t()), "out must be"),
        (dict(), "CUDA tensor"),
        (dict(out=torch.zeros(2, 1600, dtype=torch.complex64)), "CUDA tensor"),
    ]
    for kw, text in bad:
        a = dict(Y=Y, n_fft=600, hop=160)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            S._istft(torch, p, a["Y"], a["n_fft"], a["hop"], a.get("win_length"), a.get("center", True), a.get("length"), True, None,
                     a.get("out"), None, None, S._icmfft_input, torch.complex64, False)
