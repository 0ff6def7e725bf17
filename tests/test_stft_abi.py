"""Batched, centred STFT framing and overlap-add (bhw_stft_frames_f32_* / bhw_istft_ola_f32_* / bhw_describe_stft): the checks that
need no GPU -- exports and declarations, every argument error before any HIP call, the describe lines and the Python surface."""
import ctypes
import os
import re

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = -1, -2
NEW_SYMBOLS = ("bhw_stft_frames_f32_device", "bhw_stft_frames_f32_from_table", "bhw_istft_ola_f32_device", "bhw_istft_ola_f32_from_table",
               "bhw_describe_stft")
A, Z = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000)     # never dereferenced: every call below fails or has nothing to do


def _err():
    return B.lib().bhw_last_error().decode()


def _fwd(**kw):
    """T1's framing: 4 signals of 16000, n_fft 512, L 400, hop 160, centred, reflect."""
    a = dict(batch=4, samples=16000, frames=101, hop=160, n_fft=512, col0=56, pad=256, pad_mode=B.PAD_REFLECT, shift=31)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _inv(**kw):
    return _fwd(**{"pad_mode": 0, **kw})


def _frames_calls(s, L=400):
    lib = B.lib()
    return (lambda p: lib.bhw_stft_frames_f32_device(p, L, 0, None, ctypes.byref(s), A, Z),
            lambda p: lib.bhw_stft_frames_f32_from_table(None, p, L, None, ctypes.byref(s), A, Z))


def _ola_calls(s, flags=1, L=400):
    lib = B.lib()
    return (lambda p: lib.bhw_istft_ola_f32_device(p, L, 0, None, ctypes.byref(s), flags, Z, A),
            lambda p: lib.bhw_istft_ola_f32_from_table(None, p, L, None, ctypes.byref(s), flags, Z, A))


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert re.search(r"#define BHW_PAD_CONSTANT 0u", header) and re.search(r"#define BHW_PAD_REFLECT 1u", header)
    assert ctypes.sizeof(B.BhwStft) == 96 and B.BhwStft.pad_mode.offset == 88


def test_frames_argument_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    cases = [
        (dict(struct_size=8), "struct_size"),
        (dict(channels=3), "channels"),
        (dict(batch=0), "batch is 0"),
        (dict(hop=0), "hop is 0"),
        (dict(n_fft=0), "n_fft"),
        (dict(n_fft=(1 << 31) + 1), "n_fft"),
        (dict(shift=63), "shift"),
        (dict(col0=113), "col0 + L"),
        (dict(pad_mode=2), "pad_mode"),
        (dict(pad=(1 << 40) + 1), "pad"),
        (dict(frames=102), "leaves the padded signal"),
        (dict(samples=0), "samples is 0"),
        (dict(samples=256, frames=2), "reflect padding needs pad"),
        (dict(x_stride=15999), "x_stride"),
        (dict(y_stride=511), "y_stride"),
        (dict(y_batch_stride=100 * 512 + 511), "y_batch_stride"),
        (dict(batch=1 << 20, frames=101), "2^34"),
    ]
    for kw, text in cases:
        s = _fwd(**{k: v for k, v in kw.items() if k != "struct_size"})
        if "struct_size" in kw:
            s.struct_size = kw["struct_size"]
        for call in _frames_calls(s):
            rc = call(ctypes.byref(p))
            assert rc == BADARG and (text in _err() or "table is NULL" in _err()), (kw, rc, _err())
        assert _frames_calls(s)[0](ctypes.byref(p)) == BADARG and text in _err(), (kw, _err())
    # the pad rule of REFLECT is torch's: pad <= T - 1 passes the checks (then fails on the fake pointers' overlap, no HIP call)
    # (d_x = d_y: the overlap check is the last one, so reaching it means every other check passed)
    lib = B.lib()
    s = _fwd(samples=257, frames=1 + (257 + 512 - 512) // 160)
    assert lib.bhw_stft_frames_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), A, A) == BADARG and "overlap" in _err(), _err()
    # constant padding has no such rule
    s = _fwd(samples=20, frames=1, pad_mode=B.PAD_CONSTANT)
    assert lib.bhw_stft_frames_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), A, A) == BADARG and "overlap" in _err(), _err()
    # NULL pointers, overlap, the frames call's flags (through describe), Taylor, length
    s = _fwd()
    assert lib.bhw_stft_frames_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), None, Z) == BADARG and "NULL" in _err()
    assert lib.bhw_stft_frames_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), A, A) == BADARG and "overlap" in _err()
    assert lib.bhw_stft_frames_f32_device(ctypes.byref(p), 400, 0, None, None, A, Z) == BADARG and "descriptor is NULL" in _err()
    assert lib.bhw_stft_frames_f32_device(ctypes.byref(p), 0, 0, None, ctypes.byref(s), A, Z) == BADARG and "length 0" in _err()
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    assert lib.bhw_stft_frames_f32_device(ctypes.byref(taylor), 400, 0, None, ctypes.byref(s), A, Z) == UNSUPPORTED
    buf = ctypes.create_string_buffer(512)
    assert lib.bhw_describe_stft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, 1, buf, 512) == BADARG and "flags" in _err()
    assert lib.bhw_stft_frames_f32_from_table(None, ctypes.byref(p), 400, None, ctypes.byref(s), A, Z) == BADARG and "table is NULL" in _err()
    # frames 0: nothing to do, pointers unchecked
    assert lib.bhw_stft_frames_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(_fwd(frames=0)), None, None) == 0


def test_overlap_add_argument_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    lib = B.lib()
    cases = [
        (dict(pad_mode=1), "pad_mode"),
        (dict(frames=0), "frames is 0"),
        (dict(pad=55), "pad 55 < col0 56"),
        (dict(samples=(1 << 34) + 1, frames=1), "samples"),
        (dict(x_stride=100), "x_stride"),
        (dict(col0=200), "col0 + L"),
    ]
    for kw, text in cases:
        for call in _ola_calls(_inv(**kw)):
            rc = call(ctypes.byref(p))
            assert rc == BADARG and (text in _err() or "table is NULL" in _err()), (kw, rc, _err())
        assert _ola_calls(_inv(**kw))[0](ctypes.byref(p)) == BADARG and text in _err(), (kw, _err())
    s = _inv()
    assert lib.bhw_istft_ola_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), 2, Z, A) == BADARG and "flags" in _err()
    # samples past the frames' extent pass the checks (empty sums are +0.0): the fake pointers' overlap fails next
    s = _inv(samples=50000)
    assert lib.bhw_istft_ola_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), 1, A, A) == BADARG and "overlap" in _err()
    assert lib.bhw_istft_ola_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(_inv(samples=0)), 1, None, None) == 0
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    assert lib.bhw_istft_ola_f32_device(ctypes.byref(taylor), 400, 0, None, ctypes.byref(s), 1, Z, A) == UNSUPPORTED
    assert lib.bhw_istft_ola_f32_from_table(None, ctypes.byref(p), 400, None, ctypes.byref(s), 1, Z, A) == BADARG and "table is NULL" in _err()


def test_describe_names_route_plan_and_kernel():
    p = B.make_params(B.WIN_BH4, 24, 32)
    d = B.describe_stft(p, 400, _fwd())
    assert d.startswith("stft frames direct (L = 400, n_fft 512, col0 56, pad 256 reflect): k_stft_frames_direct<"), d
    assert "4 signals x 101 frames = 404 rows" in d and "G = " in d and "256 along the row" in d
    d = B.describe_stft(p, 400, _fwd(pad_mode=B.PAD_CONSTANT, batch=4096))
    assert "constant" in d and "4096 signals" in d
    d = B.describe_stft(p, 400, _inv(), inverse=True, normalize=True)
    assert d.startswith("istft overlap-add direct (L = 400, n_fft 512, col0 56, pad 256: t0 = 200), normalised by the window envelope"), d
    assert "k_ola_f32_direct_len<" in d and "4 signals (grid z 4)" in d
    p12 = B.make_params(B.WIN_BH7, 12, 32)
    s = B.make_stft(1, 1 << 14, 13, 1024, 4096, pad=2048, pad_mode=B.PAD_REFLECT, shift=31)
    assert "k_ola_f32_direct<" in B.describe_stft(p12, 4096, B.make_stft(1, 1 << 14, 13, 1024, 4096, pad=2048, shift=31), inverse=True)
    assert "k_stft_frames_direct<" in B.describe_stft(p12, 4096, s)
    assert "nothing" in B.describe_stft(p, 400, _fwd(frames=0))


def test_python_surface():
    for name in ("stft_frames", "istft_overlap_add", "describe_stft", "BhwStft", "PAD_REFLECT", "PAD_CONSTANT"):
        assert hasattr(bhw, name), name
    for name in ("stft_frames", "istft_overlap_add"):
        assert hasattr(bhw.ResidentTable, name), name
    import inspect
    sig = inspect.signature(bhw.stft_frames)
    assert list(sig.parameters)[:4] == ["params", "x", "n_fft", "hop"]
    assert sig.parameters["center"].default is True and sig.parameters["pad_mode"].default == "reflect"
    sig = inspect.signature(bhw.istft_overlap_add)
    assert sig.parameters["normalize"].default is True and sig.parameters["length"].default is None
