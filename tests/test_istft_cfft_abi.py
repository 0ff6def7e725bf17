"""The fused inverse complex FFT + overlap-add calls for I/Q output (bhw_istft_cfft_f32_device / _from_table /
bhw_describe_istft_cfft): the checks that need no GPU -- exports and declarations, every refusal of include/bhw.h before any HIP call
and the order of the checks, samples 0, the refusals bhw_istft_fft_f32_* keeps, the describe line and the Python surface with host
tensors."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from blackman_harris_win_amd import selector as S

import istft_cfft_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED = 0, -1, -2
NEW_SYMBOLS = ("bhw_istft_cfft_f32_device", "bhw_istft_cfft_f32_from_table", "bhw_describe_istft_cfft")
# never dereferenced: every call below fails or has nothing to do
A, Z = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000)


def _err():
    return B.lib().bhw_last_error().decode()


def _desc(**kw):
    """torch.istft's framing of complex signals: 4 signals, 101 frames of 512 at hop 160, window 400, centred: 16000 samples."""
    a = dict(batch=4, samples=16000, frames=101, hop=160, n_fft=512, col0=56, pad=256, shift=31, channels=2)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _calls(s, flags=1, L=400, Y=Z, x=A, real=False):
    lib = B.lib()
    dev, tab = (lib.bhw_istft_fft_f32_device, lib.bhw_istft_fft_f32_from_table) if real else \
        (lib.bhw_istft_cfft_f32_device, lib.bhw_istft_cfft_f32_from_table)
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
    assert "bhw_istft_fft_f32_* keeps\n * refusing channels 2" in header and "one E for both parts" in header
    assert "Checks before any HIP call, in this order" in header[header.index("Fused inverse complex FFT"):]
    assert L.bhw_istft_cfft_f32_device.argtypes == L.bhw_istft_fft_f32_device.argtypes
    assert L.bhw_istft_cfft_f32_from_table.argtypes == L.bhw_istft_fft_f32_from_table.argtypes
    assert L.bhw_describe_istft_cfft.argtypes == L.bhw_describe_istft_fft.argtypes


def test_descriptor_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    W = 1024
    cases = [
        (dict(struct_size=8), BADARG, "struct_size"),
        (dict(channels=3), BADARG, "channels"),
        (dict(channels=1), UNSUPPORTED, "bhw_istft_fft_f32_*"),
        (dict(batch=0), BADARG, "batch is 0"),
        (dict(hop=0), BADARG, "hop is 0"),
        (dict(n_fft=0), BADARG, "n_fft"),
        (dict(n_fft=256), BADARG, "col0 + L"),
        (dict(n_fft=500, col0=50), UNSUPPORTED, "power of two"),
        (dict(n_fft=4096), UNSUPPORTED, "power of two in 16..2048"),
        (dict(n_fft=8, col0=0, pad=4), UNSUPPORTED, "power of two"),
        (dict(shift=63), BADARG, "shift"),
        (dict(pad=55), BADARG, "pad 55 < col0 56"),
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
            L = 8 if kw.get("n_fft") == 8 else 400
            s = _desc(**{k: v for k, v in kw.items() if k != "struct_size"})
            if "struct_size" in kw:
                s.struct_size = kw["struct_size"]
            for call in _calls(s, flags=flags, L=L):
                assert call(ref) == code and text in _err(), (flags, kw, _err())
    # an odd x_stride from 2 * samples is no error: every check passed, and the from-table call stops at the missing table, before any
    # launch
    for flags in (0, 1, 4, 5):
        for s in (_desc(), _desc(x_stride=32001), _desc(y_stride=W + 6, y_batch_stride=101 * (W + 6) + 10)):
            assert B.lib().bhw_istft_cfft_f32_from_table(None, ref, 400, None, ctypes.byref(s), flags, Z, A) == BADARG
            assert "table is NULL" in _err()


def test_the_order_of_the_checks():
    """include/bhw.h: the overlap-add's checks on the packed descriptor, unknown flag bits, the unsupported channels and n_fft, samples
    0, the stride rules, the pointers, the table."""
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    bad = ctypes.c_void_p(0x80000004)
    # everything wrong at once, then one error fewer at every step
    steps = [
        (dict(hop=0, channels=1, n_fft=4096, col0=0, pad=2048, y_stride=7), 8, None, "hop is 0", BADARG),
        (dict(channels=1, n_fft=4096, col0=0, pad=2048, y_stride=7), 8, None, "flags 0x8", BADARG),
        (dict(channels=1, n_fft=4096, col0=0, pad=2048, y_stride=7), 5, None, "channels 1", UNSUPPORTED),
        (dict(n_fft=4096, col0=0, pad=2048, y_stride=7), 5, None, "n_fft 4096", UNSUPPORTED),
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
    assert B.lib().bhw_istft_cfft_f32_from_table(None, ref, 400, None, ctypes.byref(_desc()), 5, Z, A) == BADARG and "table is NULL" in _err()
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
            assert call(ref) == BADARG and "flags" in _err(), flags
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
    assert B.lib().bhw_istft_cfft_f32_from_table(None, ref, 400, None, ctypes.byref(s), 1, Z, ctypes.c_void_p(0x10000004)) == BADARG
    assert "table is NULL" in _err()
    # d_Y inside x, x inside d_Y, and the first byte behind each: x holds 4 * 2 * 16000 floats, Y 4 * 101 * 1024
    xb, yb = 4 * 2 * 16000 * 4, 4 * 101 * 1024 * 4
    for x, Y, bad in ((0x10000000, 0x10000000 + xb - 8, True), (0x10000000, 0x10000000 + xb, False), (0x80000000 + yb - 4, 0x80000000, True),
                      (0x80000000 + yb, 0x80000000, False)):
        rc = B.lib().bhw_istft_cfft_f32_from_table(None, ref, 400, None, ctypes.byref(s), 1, ctypes.c_void_p(Y), ctypes.c_void_p(x))
        assert rc == BADARG and ("overlap" if bad else "table is NULL") in _err(), (hex(x), hex(Y), _err())
        if bad:
            assert B.lib().bhw_istft_cfft_f32_device(ref, 400, 0, None, ctypes.byref(s), 1, ctypes.c_void_p(Y), ctypes.c_void_p(x)) == BADARG
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    for call in _calls(s):
        assert call(ctypes.byref(taylor)) == UNSUPPORTED


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1024)
    for n in range(1, 4200):
        s = B.make_stft(2, 1000, 3, 7, n, pad=n // 2, channels=2, shift=31)
        rc = lib.bhw_describe_istft_cfft(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), 5, buf, 1024)
        assert rc == (OK if B.cfft_supported(n) else UNSUPPORTED), (n, rc, _err())
    assert [n for n in (8, 16, 500, 2048, 4096) if B.cfft_supported(n)] == [16, 2048]


def test_samples_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    for flags in (0, 1, 4, 5):
        for frames in (0, 101):
            s = _desc(samples=0, frames=frames)
            assert B.lib().bhw_istft_cfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, None, None) == OK
            assert "nothing (samples 0)" in B.describe_istft_cfft(p, 400, s, normalize=bool(flags & 1), fftshift=bool(flags & 4))
        s = _desc(samples=0, n_fft=768, col0=184, pad=384)
        assert B.lib().bhw_istft_cfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, None, None) == UNSUPPORTED


def test_the_real_entry_points_keep_their_refusals():
    """bhw_istft_fft_f32_* still answers channels 2 with BHW_ERR_UNSUPPORTED ("real output"), the shift flag with BHW_ERR_BADARG, and
    takes n_fft 4096; bhw.istft still refuses two-sided and real spectra."""
    torch = pytest.importorskip("torch")
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    for call in _calls(_desc(), real=True):
        assert call(ref) == UNSUPPORTED and "real output" in _err()
    for call in _calls(_desc(channels=1), flags=4, real=True):
        assert call(ref) == BADARG and "flags" in _err()
    s = B.make_stft(2, 8192, 5, 2048, 4096, pad=2048, shift=31)
    assert "k_istft_fft_direct" in B.describe_istft_fft(p, 4096, s)
    # the body bhw.istft and bhw.istft_iq share, with istft's defaults (the public functions refuse to start without a HIP device)
    with pytest.raises(ValueError, match="CUDA tensor"):
        S._istft(torch, p, torch.zeros(3, 512, dtype=torch.complex64), 512, 160, None, True, None, True, None, None, None, None)


def test_describe_line_parses():
    p = B.make_params(B.WIN_BH7, 16, 32)
    d = IC.parse(B.describe_istft_cfft(p, 400, _desc(batch=64, samples=159520, frames=998), normalize=True))
    assert d["line"].startswith("istft cfft direct (L = 400, n_fft 512, col0 56, pad 256: t0 = 200), normalised by the window envelope, "
                                "bins in order: k_istft_cfft_direct<2>")
    assert (d["signals"], d["frames"], d["rows"], d["m"], d["schedule"]) == (64, 998, 63872, 512, "4x4x4x4x2")
    assert (d["lpf"], d["fy"], d["cpl"], d["lds"]) == (128, 2, 4, 2 * 2 * 512 * 8 + 256 * 8 + 512 * 4)
    # S: 64 * 998 rows over 1024 groups of 2 slots; halo: ceil(400 / 160) - 1; the repeats: 2 of every 33 transforms
    assert (d["S"], d["halo"], d["spans"], d["trips"], d["repeated"]) == (31, 2, 33, 33, 6)
    assert (d["groups"], d["grid"]) == (1056, 1056) and not d["heavy"] and "(no split)" in d["line"]
    d = IC.parse(B.describe_istft_cfft(p, 2048, B.make_stft(1, 8192, 9, 1024, 2048, pad=1024, channels=2, shift=31), fftshift=True))
    assert (d["schedule"], d["lpf"], d["fy"], d["cpl"], d["lds"]) == ("4x4x4x4x4x2", 256, 1, 8, 48 * 1024) and not d["normalize"] and d["shifted"]
    # heavy overlap and one short signal: the halo sets S, few workgroups run, and the line says so
    d = IC.parse(B.describe_istft_cfft(p, 2048, B.make_stft(1, 34000, 2126, 16, 2048, pad=1024, channels=2, shift=31), normalize=True))
    assert (d["halo"], d["S"], d["groups"]) == (127, 508, 5) and d["heavy"] and "ifft + istft overlap-add" in d["line"]
    with pytest.raises(B.BhwError):
        B.describe_istft_cfft(p, 400, _desc(n_fft=500, col0=50))
    # a short buffer truncates, a missing one is an error
    buf = ctypes.create_string_buffer(16)
    s = _desc()
    assert B.lib().bhw_describe_istft_cfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, buf, 16) == OK and len(buf.value) == 15
    assert B.lib().bhw_describe_istft_cfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, None, 0) == BADARG


def test_python_surface():
    for name in ("istft_iq", "describe_istft_cfft"):
        assert name in bhw.__all__ and hasattr(bhw, name)
    sig = inspect.signature(bhw.istft_iq)
    assert list(sig.parameters) == ["params", "Y", "n_fft", "hop", "win_length", "center", "length", "normalize", "shift", "fftshift", "out"]
    assert sig.parameters["center"].default is True and sig.parameters["normalize"].default is True and sig.parameters["length"].default is None
    assert sig.parameters["fftshift"].default is False
    for name in ("win_length", "center", "length", "normalize", "shift", "fftshift", "out"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(bhw.ResidentTable.istft_iq).parameters)[1:] == list(sig.parameters)
    assert [n for n in sig.parameters if n != "fftshift"] == list(inspect.signature(bhw.istft).parameters)
    doc = bhw.istft_iq.__doc__
    assert "transpose(-1, -2)" in doc and "torch.istft" in doc and "onesided=False" in doc and "does not reroute" in doc


def test_python_value_errors_need_no_device():
    """Every ValueError of istft_iq is raised before the device is looked at: the shared body is called with host tensors here (the
    public functions refuse to start without a HIP device), which reach all of them, and a good host tensor reaches the device check
    last."""
    torch = pytest.importorskip("torch")
    p = B.make_params(B.WIN_BH4, 24, 32)
    Y = torch.zeros(2, 11, 512, dtype=torch.complex64)
    bad = [
        (dict(Y=torch.zeros(2, 11, 512)), "complex64"),
        (dict(Y=torch.zeros(2, 11, 512, dtype=torch.complex128)), "complex64"),
        (dict(Y=[1, 2, 3]), "complex64"),
        (dict(Y=torch.zeros(512, dtype=torch.complex64)), r"\(frames, n_fft\)"),
        (dict(Y=torch.zeros(2, 11, 257, dtype=torch.complex64)), "257 bins"),
        (dict(Y=torch.zeros(2, 0, 512, dtype=torch.complex64)), "zero frames"),
        (dict(n_fft=4096, Y=torch.zeros(2, 3, 4096, dtype=torch.complex64)), "power of two in 16..2048"),
        (dict(n_fft=500, Y=torch.zeros(2, 3, 500, dtype=torch.complex64)), "power of two"),
        (dict(n_fft=8, Y=torch.zeros(2, 3, 8, dtype=torch.complex64)), "power of two"),
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
        a = dict(Y=Y, n_fft=512, hop=160)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            S._istft(torch, p, a["Y"], a["n_fft"], a["hop"], a.get("win_length"), a.get("center", True), a.get("length"), True, None,
                     a.get("out"), None, None, S._icfft_input, torch.complex64, False)
