"""The fused Welch PSD calls for I/Q input at a mixed-radix n_fft (bhw_welch_cmfft_f32_device / _from_table /
bhw_welch_cmfft_workspace_bytes / bhw_describe_welch_cmfft): the checks that need no GPU -- exports and declarations, every refusal of
include/bhw.h with its code and words, in the stated order and before any HIP call, the workspace formula, frames 0, the describe
line, the messages of the existing families, and the Python surface."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import welch_cmfft_cases as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
NEW_SYMBOLS = ("bhw_welch_cmfft_workspace_bytes", "bhw_welch_cmfft_f32_device", "bhw_welch_cmfft_f32_from_table", "bhw_describe_welch_cmfft")
# never dereferenced: every call below fails or has nothing to do
X, P, W = 0x10000000, 0x80000000, 0x40000000
N = 600
DETREND, POWER, SHIFT = 1, 2, 4
POW2 = "n_fft {}: the fused complex FFT takes a power of two in 16..2048"
IS_POW2 = "n_fft {} is a power of two: bhw_stft_cfft_f32_* transforms it (one transform per n_fft)"
NO_SIZE = "n_fft {}: the mixed-radix fused complex FFT takes 2^a 3^b 5^c in 16..2047"
REAL = "channels 1: the mixed-radix fused complex FFT takes interleaved I/Q input (2); real input: bhw_stft_mfft_f32_*"


def _err():
    return B.lib().bhw_last_error().decode()


def _seg(**kw):
    """Welch framing of I/Q input: 4 signals of 16000 complex samples, window 400 in rows of 600, hop 160, no padding: 98 frames, 7
    chunks, one block."""
    a = dict(batch=4, samples=16000, frames=98, hop=160, n_fft=N, channels=2, shift=31)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _need(s):
    return 8 * WM.workspace_doubles(s.batch, s.frames, s.n_fft)


def _calls(s, flags=DETREND, L=400, scale=1.0, x=X, out=P, p_stride=0, ws=W, ws_bytes=None):
    lib = B.lib()
    sr = ctypes.byref(s) if s is not None else None
    nbytes = (_need(s) if s is not None else 0) if ws_bytes is None else ws_bytes
    tail = (sr, flags, scale, ctypes.c_void_p(x), ctypes.c_void_p(out), p_stride, ctypes.c_void_p(ws), nbytes)
    return (lambda p: lib.bhw_welch_cmfft_f32_device(p, L, 0, None, *tail),
            lambda p: lib.bhw_welch_cmfft_f32_from_table(None, p, L, None, *tail))


def _passes(ref, s, **kw):
    """Every check passed: the from-table call with no table stops at 'table is NULL', before any launch."""
    rc = _calls(s, **kw)[1](ref)
    return rc == BADARG and "table is NULL" in _err()


def _header():
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        return fh.read()


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    header = _header()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\b(int|uint64_t) " + name + r"\(", header), name
    assert L.bhw_abi_version() == 4
    assert ctypes.sizeof(B.BhwStft) == 96 and ctypes.sizeof(B.BhwPsd) == 72
    at = header.index("Fused Welch PSD for complex (I/Q) input at a mixed-radix n_fft")
    text = header[at:header.index("uint64_t bhw_welch_cmfft_workspace_bytes")]
    for words in ("not on B, the grid", "bit for bit", "within one float32 ulp", "no float\n *     atomics", "BHW_CFFT_POWER is refused",
                  "no psd_flags", "(k + n_fft / 2) mod n_fft", "integer\n *     division", "torch.fft.fftshift", "ascending f",
                  "Not built: n_fft >= 2048; factors of 7 and above; I/Q cross spectra", "max-hold or median"):
        assert words in text, words
    # the check order is a numbered list
    assert [int(m) for m in re.findall(r"\n \*       (\d)\. ", text)] == list(range(1, 9))


def test_the_prototypes_are_the_power_of_two_calls_word_for_word():
    header = _header()
    for kind, tail in (("int", "_f32_device"), ("int", "_f32_from_table"), ("uint64_t", "_workspace_bytes")):
        new = re.search(kind + r" bhw_welch_cmfft" + tail + r"\(([^;]*)\);", header).group(1)
        old = re.search(kind + r" bhw_welch_cfft" + tail + r"\(([^;]*)\);", header).group(1)
        assert re.sub(r"\s+", " ", new) == re.sub(r"\s+", " ", old), tail
    new = re.search(r"int bhw_describe_welch_cmfft\(([^;]*)\);", header).group(1)
    assert new == re.search(r"int bhw_describe_welch_cfft\(([^;]*)\);", header).group(1)
    L = B.lib()
    for tail in ("_workspace_bytes", "_f32_device", "_f32_from_table"):
        assert getattr(L, "bhw_welch_cmfft" + tail).argtypes == getattr(L, "bhw_welch_cfft" + tail).argtypes
        assert getattr(L, "bhw_welch_cmfft" + tail).restype == getattr(L, "bhw_welch_cfft" + tail).restype
    assert L.bhw_describe_welch_cmfft.argtypes == L.bhw_describe_welch_cfft.argtypes


def test_input_side_errors_are_the_forward_calls():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    cases = [
        (dict(struct_size=8), BADARG, "struct_size"),
        (dict(channels=3), BADARG, "channels"),
        (dict(channels=1), UNSUPPORTED, REAL),
        (dict(batch=0), BADARG, "batch is 0"),
        (dict(hop=0), BADARG, "hop is 0"),
        (dict(n_fft=0), BADARG, "n_fft"),
        (dict(n_fft=256), BADARG, "col0 + L"),
        (dict(n_fft=512), UNSUPPORTED, IS_POW2.format(512)),
        (dict(n_fft=4096), UNSUPPORTED, IS_POW2.format(4096)),
        (dict(n_fft=448), UNSUPPORTED, NO_SIZE.format(448)),
        (dict(n_fft=2160), UNSUPPORTED, NO_SIZE.format(2160)),
        (dict(n_fft=601), UNSUPPORTED, NO_SIZE.format(601)),
        (dict(shift=63), BADARG, "shift"),
        (dict(frames=99), BADARG, "segment 98 leaves the signal"),
        (dict(samples=0), BADARG, "samples is 0"),
        (dict(x_stride=31999), BADARG, "x_stride"),
    ]
    buf = ctypes.create_string_buffer(1280)
    for flags in (0, DETREND, SHIFT, DETREND | SHIFT):
        for kw, code, text in cases:
            s = _seg(**{k: v for k, v in kw.items() if k != "struct_size"})
            if "struct_size" in kw:
                s.struct_size = kw["struct_size"]
            for call in _calls(s, flags=flags):
                assert call(ref) == code and text in _err(), (flags, kw, _err())
            # the same code and the same words as the forward call
            want = _err()
            assert B.lib().bhw_describe_stft_cmfft(None, ref, 400, ctypes.byref(s), flags, buf, 1280) == code and _err() == want, (kw, want, _err())
        assert _passes(ref, _seg(), flags=flags)
    # the small unsupported sizes, with a window that fits
    for n, text in ((14, NO_SIZE), (21, NO_SIZE), (16, IS_POW2), (2048, IS_POW2)):
        for call in _calls(_seg(n_fft=n, samples=100000, hop=7, frames=3), L=8):
            assert call(ref) == UNSUPPORTED and _err() == text.format(n), _err()
    for kw, text in ((dict(pad=300), "pad 300"), (dict(col0=100), "col0 100"), (dict(pad_mode=B.PAD_REFLECT), "pad_mode 1")):
        for call in _calls(_seg(**kw), flags=DETREND):
            assert call(ref) == BADARG and text in _err(), (kw, _err())
    # the padding fields as the forward call accepts them: a centred, reflect-padded descriptor (1 + (16000 + 600 - 600) / 160 = 101)
    assert _passes(ref, _seg(pad=300, col0=100, pad_mode=B.PAD_REFLECT, frames=101), flags=0)
    for call in _calls(_seg(pad=300, col0=100, pad_mode=B.PAD_REFLECT, frames=102), flags=0):
        assert call(ref) == BADARG and "leaves the padded signal" in _err()
    # an unknown flag is the forward call's refusal, in its words
    for call in _calls(_seg(), flags=8):
        assert call(ref) == BADARG and _err() == "flags 0x8 (BHW_WELCH_DETREND_CONSTANT, BHW_CFFT_POWER, BHW_CFFT_SHIFT)"
    for call in _calls(None):
        assert call(ref) == BADARG and "descriptor is NULL" in _err()
    for call in _calls(_seg()):
        assert call(None) == BADARG
    for call in _calls(_seg(), L=0):
        assert call(ref) == BADARG and "length" in _err()
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    for call in _calls(_seg()):
        assert call(ctypes.byref(taylor)) == UNSUPPORTED


def test_power_flag_is_refused():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    for flags in (POWER, POWER | DETREND, POWER | SHIFT, POWER | DETREND | SHIFT):
        for call in _calls(_seg(), flags=flags):
            assert call(ref) == BADARG and _err() == (f"flags 0x{flags:x}: BHW_CFFT_POWER has no meaning here (BHW_WELCH_DETREND_CONSTANT, "
                                                      "BHW_CFFT_SHIFT)"), _err()
        # also with frames 0, and from the describe call
        assert B.lib().bhw_welch_cmfft_f32_device(ref, 400, 0, None, ctypes.byref(_seg(frames=0)), flags, 1.0, None, None, 0, None, 0) == BADARG
        buf = ctypes.create_string_buffer(1280)
        assert B.lib().bhw_describe_welch_cmfft(None, ref, 400, ctypes.byref(_seg()), flags, buf, 1280) == BADARG
    # the forward call still takes it
    buf = ctypes.create_string_buffer(1280)
    assert B.lib().bhw_describe_stft_cmfft(None, ref, 400, ctypes.byref(_seg()), POWER, buf, 1280) == OK


def test_output_side_errors_in_the_stated_order():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    s = _seg()
    # 2. no spectrum is written: non-zero y strides are refused, whatever their value
    for kw in (dict(y_stride=2 * N), dict(y_batch_stride=98 * 2 * N), dict(y_stride=2 * N + 2, y_batch_stride=98 * (2 * N + 2)), dict(y_stride=3)):
        for call in _calls(_seg(**kw)):
            assert call(ref) == BADARG and "no spectrum is written, both must be 0" in _err(), (kw, _err())
    for scale in (float("inf"), float("-inf"), float("nan")):
        for call in _calls(s, scale=scale):
            assert call(ref) == BADARG and _err() == "scale is not finite"
    for scale in (0.0, -1.5, 1e300):
        assert _passes(ref, s, scale=scale)
    # 4.
    for call in _calls(s, p_stride=N - 1):
        assert call(ref) == BADARG and _err() == f"p_stride {N - 1} < n_fft {N}: rows overlap"
    assert _passes(ref, s, p_stride=N) and _passes(ref, s, p_stride=N + 7)
    # The stated limit, batch * ceil(frames / 16) * n_fft above 2^34, cannot be the first to refuse: ceil(F / 16) <= F, and the forward
    # checks, which run first, hold batch * frames * n_fft to 2^34.  What is matched here is THEIR message.
    big = (1 << 34) // (98 * N) + 1
    for call in _calls(_seg(batch=big), ws_bytes=1 << 60):
        assert call(ref) == BADARG and _err() == "batch * frames * n_fft above 2^34 per call", _err()
    # 5.
    for kw in (dict(x=0), dict(out=0)):
        for call in _calls(s, **kw):
            assert call(ref) == BADARG and _err() == "d_x / d_P is NULL"
    for call in _calls(s, out=P + 2):
        assert call(ref) == BADARG and _err() == "d_P is not 4-byte aligned"
    assert _passes(ref, s, out=P + 4)
    for call in _calls(s, x=X + 2):
        assert call(ref) == BADARG and _err() == "d_x is not 4-byte aligned"
    assert _passes(ref, s, x=X + 4)                  # complex samples need no 8-byte alignment: the kernel then loads the parts apart
    # 6. the workspace: NULL, misaligned, short (its own code), and exactly enough
    for call in _calls(s, ws=0):
        assert call(ref) == BADARG and _err() == f"workspace is NULL: the chunk sums need {_need(s)} bytes"
    for call in _calls(s, ws=W + 4):
        assert call(ref) == BADARG and _err() == "workspace is not 8-byte aligned"
    for call in _calls(s, ws_bytes=_need(s) - 1):
        assert call(ref) == WORKSPACE and _err() == f"workspace of {_need(s) - 1} bytes, the chunk and block sums need {_need(s)}"
    for call in _calls(s, ws_bytes=0):
        assert call(ref) == WORKSPACE
    assert _passes(ref, s, ws_bytes=_need(s)) and _passes(ref, s, ws_bytes=_need(s) + 8)
    # 7. overlaps: x holds 4 * 16000 complex = 4 * 32000 floats, P 4 * 600 floats, the workspace _need(s) bytes
    xb, pb, wb = 4 * 32000 * 4, 4 * N * 4, _need(s)
    for kw, bad, text in (
            (dict(x=X, out=X + xb - 4), True, "d_x and d_P overlap"), (dict(x=X, out=X + xb), False, ""),
            (dict(x=P + pb - 4, out=P), True, "d_x and d_P overlap"), (dict(x=P + pb, out=P), False, ""),
            (dict(x=X, ws=X + xb - 8), True, "workspace overlaps d_x or d_P"), (dict(x=X, ws=X + xb), False, ""),
            (dict(x=W + wb - 4, ws=W), True, "workspace overlaps d_x or d_P"), (dict(x=W + wb, ws=W), False, ""),
            (dict(out=P, ws=P + pb - 8), True, "workspace overlaps d_x or d_P"), (dict(out=W + wb - 4, ws=W), True, "workspace overlaps d_x or d_P"),
            (dict(out=W + wb, ws=W), False, "")):
        if bad:
            for call in _calls(s, **kw):
                assert call(ref) == BADARG and _err() == text, (kw, _err())
        else:
            assert _passes(ref, s, **kw), (kw, _err())
    # the order: for each adjacent pair of the header's list a call that breaks both rules; the earlier one wins
    order = [
        (dict(s=_seg(n_fft=512, y_stride=3), flags=POWER, scale=float("nan")), UNSUPPORTED, "is a power of two"),       # 1 before 2
        (dict(s=_seg(n_fft=448, y_stride=3), flags=POWER, scale=float("nan")), UNSUPPORTED, "2^a 3^b 5^c"),
        (dict(s=_seg(channels=1, n_fft=512), flags=POWER), UNSUPPORTED, "channels 1"),                                   #    inside 1
        (dict(s=_seg(y_stride=3), flags=POWER, scale=float("nan")), BADARG, "BHW_CFFT_POWER"),                          # 2: the flag,
        (dict(s=_seg(y_stride=3), scale=float("nan")), BADARG, "no spectrum is written"),                               #    the strides,
        (dict(s=s, scale=float("nan"), p_stride=1), BADARG, "scale is not finite"),                                     #    the scale
        (dict(s=_seg(frames=0), scale=float("nan"), p_stride=1, x=0), BADARG, "scale is not finite"),                   # 2 before 3
        (dict(s=s, p_stride=1, x=0), BADARG, "p_stride"),                                                               # 4 before 5
        (dict(s=s, x=0, ws=0), BADARG, "d_x / d_P is NULL"),                                                            # 5 before 6
        (dict(s=s, out=P + 2, ws=W + 4), BADARG, "d_P is not 4-byte aligned"),
        (dict(s=s, ws=0, ws_bytes=0), BADARG, "workspace is NULL"),                                                     #    inside 6
        (dict(s=s, ws=W + 4, ws_bytes=0), BADARG, "workspace is not 8-byte aligned"),
        (dict(s=s, ws_bytes=8, x=P), WORKSPACE, "workspace of 8 bytes"),                                                # 6 before 7
        (dict(s=s, x=P), BADARG, "d_x and d_P overlap"),                                                                # 7 before 8
    ]
    for kw, code, text in order:
        kw = dict(kw)
        for call in _calls(kw.pop("s"), **kw):
            assert call(ref) == code and text in _err(), (kw, code, _err())
    # 3 before 4: frames 0 is OK whatever p_stride and the pointers are
    assert B.lib().bhw_welch_cmfft_f32_device(ref, 400, 0, None, ctypes.byref(_seg(frames=0)), 0, 1.0, None, None, 1, None, 0) == OK


def test_the_refusals_are_the_power_of_two_calls_words():
    """Steps 2 to 7 are one text for both I/Q Welch families: the same call, at a size each takes, gives the same words."""
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    lib = B.lib()
    for kw in (dict(flags=POWER), dict(scale=float("nan")), dict(p_stride=1), dict(x=0), dict(out=P + 2), dict(x=X + 2), dict(ws=W + 4),
               dict(x=P), dict(ws=X)):
        words = []
        for n, fn in ((600, lib.bhw_welch_cmfft_f32_device), (512, lib.bhw_welch_cfft_f32_device)):
            a = dict(flags=DETREND, scale=1.0, x=X, out=P, p_stride=0, ws=W)
            a.update(kw)
            s = _seg(n_fft=n)
            rc = fn(ref, 400, 0, None, ctypes.byref(s), a["flags"], a["scale"], ctypes.c_void_p(a["x"]), ctypes.c_void_p(a["out"]), a["p_stride"],
                    ctypes.c_void_p(a["ws"]), _need(s))
            words.append((rc, _err().replace(str(n), "N")))
        assert words[0] == words[1] and words[0][0] == BADARG, (kw, words)


@pytest.mark.parametrize("cid", WM.case_ids())
def test_workspace_bytes_equal_the_formula(cid):
    c = WM.case(cid)
    s, _, F, _ = WM.desc(c)
    n = c["n_fft"]
    chunks, blocks = -(-F // 16), -(-F // 256)
    want = 8 * c["B"] * n * (chunks + (blocks if blocks > 1 else 0))
    assert B.welch_cmfft_workspace_bytes(s) == want == WM.parse(WM.line(c))["workspace"]
    p = WM.params(c["setup"])
    for flags in (int(c["detrend"]), int(c["detrend"]) | SHIFT):
        assert _passes(ctypes.byref(p), s, L=c["L"], flags=flags, ws_bytes=want), _err()
        for call in _calls(s, L=c["L"], flags=flags, ws_bytes=want - 8):
            assert call(ctypes.byref(p)) == WORKSPACE, _err()


def test_workspace_bytes_of_nothing():
    assert B.lib().bhw_welch_cmfft_workspace_bytes(None) == 0
    assert B.welch_cmfft_workspace_bytes(_seg(frames=0)) == 0
    s = _seg()
    s.struct_size = 80
    assert B.welch_cmfft_workspace_bytes(s) == 0


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1280)
    ok = []
    for n in list(range(1, 2101)) + [2160, 2187, 2250, 4050, 4096]:
        s = B.make_stft(2, 100000, 3, 7, n, channels=2, shift=31)
        rc = lib.bhw_describe_welch_cmfft(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), DETREND, buf, 1280)
        assert rc == (OK if B.cmfft_supported(n) else UNSUPPORTED), (n, rc, _err())
        if rc == OK:
            ok.append(n)
            assert buf.value.decode().startswith(f"welch cmfft direct (L = 16, n_fft {n}, ")
        elif n >= 1 and n & (n - 1) == 0 and n >= 16:
            assert _err() == IS_POW2.format(n)
    assert ok == WM.SIZES and len(ok) == 91
    # real input is refused with the forward call's words
    s = B.make_stft(2, 100000, 3, 7, 600, channels=1, shift=31)
    assert lib.bhw_describe_welch_cmfft(None, ctypes.byref(p), 16, ctypes.byref(s), DETREND, buf, 1280) == UNSUPPORTED
    assert _err() == REAL


def test_frames_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    for flags in (0, DETREND, SHIFT):
        s = _seg(frames=0)
        assert lib.bhw_welch_cmfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, None, None, 0, None, 0) == OK
        assert lib.bhw_welch_cmfft_f32_from_table(None, ctypes.byref(p), 400, None, ctypes.byref(s), flags, 1.0, None, None, 0, None, 0) == BADARG
        assert "table is NULL" in _err()
        line = B.describe_welch_cmfft(p, 400, s, detrend=bool(flags & DETREND), fftshift=bool(flags & SHIFT))
        assert line.startswith("welch cmfft direct (L = 400, n_fft 600, ") and line.endswith(": nothing (frames 0)")
        # what is checked before frames 0 returns: the descriptor, the flag, the strides, the scale
        assert lib.bhw_welch_cmfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, float("nan"), None, None, 0, None, 0) == BADARG
        assert lib.bhw_welch_cmfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(_seg(frames=0, y_stride=1200)), flags, 1.0, None, None, 0,
                                              None, 0) == BADARG
        # and what is not: p_stride
        assert lib.bhw_welch_cmfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, None, None, 1, None, 0) == OK
        s = _seg(frames=0, n_fft=512)
        assert lib.bhw_welch_cmfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, None, None, 0, None, 0) == UNSUPPORTED


def test_describe_line_parses():
    p = B.make_params(B.WIN_BH7, 16, 32)
    s = _seg(batch=64, samples=160000, frames=998, n_fft=400)
    line = B.describe_welch_cmfft(p, 400, s, detrend=True)
    d = WM.parse(line)
    assert line.startswith("welch cmfft direct (L = 400, n_fft 400, col0 0, pad 0 constant, constant detrend), bins in order: "
                           "k_welch_cmfft_direct<2>, 64 signals x 998 frames = 63872 rows, complex FFT of 400 points in passes 5x5x4x4 "
                           "(no split), 128 lanes per row x 2 rows per workgroup, 4 columns per lane, ")
    assert (d["signals"], d["frames"], d["rows"], d["m"], d["schedule"], d["fold"]) == (64, 998, 63872, 400, "5x5x4x4", 200)
    assert (d["lpf"], d["fy"], d["cpl"], d["lds"]) == (128, 2, 4, 2 * 2 * 400 * 8 + 200 * 8 + 16)
    # 998 frames pad to 1008 = 63 runs of 16 frames per signal, eight groups each
    assert (d["chunk"], d["run"], d["gpr"], d["runs"], d["groups"], d["grid"]) == (16, 16, 8, 64 * 63, 64 * 63 * 8, 2048)
    assert (d["acc"], d["chunks"], d["blocks"], d["joins"], d["workspace"]) == (2, 63, 4, 2, 8 * 64 * 400 * (63 + 4))
    assert line.endswith("14416 bytes of LDS, 200 twiddles; chunk 16 frames, 4032 runs of 16 frames (8 groups per run), 2 accumulators per lane, "
                         f"63 chunks and 4 blocks per signal, then k_welch_fft_join twice (chunks, blocks), workspace {8 * 64 * 400 * 67} bytes")
    assert "spectrum rows" not in line and "power rows" not in line
    assert "bins shifted" in B.describe_welch_cmfft(p, 400, s, detrend=True, fftshift=True)
    # one signal of 2^24 samples at 2000 / hop 500
    t2 = WM.parse(B.describe_welch_cmfft(p, 2000, B.make_stft(1, 1 << 24, 33551, 500, 2000, channels=2, shift=31), detrend=True))
    assert (t2["runs"], t2["chunks"], t2["blocks"], t2["acc"], t2["gpr"], t2["grid"]) == (2097, 2097, 132, 8, 16, 2048)
    with pytest.raises(B.BhwError):
        B.describe_welch_cmfft(p, 400, _seg(n_fft=512))
    buf = ctypes.create_string_buffer(16)
    assert B.lib().bhw_describe_welch_cmfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, buf, 16) == OK and len(buf.value) == 15
    assert B.lib().bhw_describe_welch_cmfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, None, 0) == BADARG


def test_the_existing_families_keep_their_messages():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1280)
    # the power-of-two I/Q Welch call: its refusals of the mixed-radix sizes and of each output-side rule, word for word
    tail = lambda s, **kw: (ctypes.byref(s), kw.get("flags", 1), kw.get("scale", 1.0), ctypes.c_void_p(kw.get("x", X)), ctypes.c_void_p(kw.get("out", P)),
                            kw.get("p_stride", 0), ctypes.c_void_p(kw.get("ws", W)), kw.get("ws_bytes", 1 << 30))
    for n in (500, 400, 600):
        assert lib.bhw_welch_cfft_f32_device(ref, 400, 0, None, *tail(_seg(n_fft=n))) == UNSUPPORTED
        assert _err() == POW2.format(n)
        assert lib.bhw_describe_welch_cfft(None, ref, 400, ctypes.byref(_seg(n_fft=n)), 1, buf, 1280) == UNSUPPORTED and _err() == POW2.format(n)
    s = _seg(n_fft=512)
    need = 8 * 4 * 512 * 7
    assert B.welch_cfft_workspace_bytes(s) == need
    for kw, code, text in (
            (dict(flags=POWER | DETREND), BADARG, "flags 0x3: BHW_CFFT_POWER has no meaning here (BHW_WELCH_DETREND_CONSTANT, BHW_CFFT_SHIFT)"),
            (dict(scale=float("inf")), BADARG, "scale is not finite"),
            (dict(p_stride=511), BADARG, "p_stride 511 < n_fft 512: rows overlap"),
            (dict(x=0), BADARG, "d_x / d_P is NULL"),
            (dict(out=P + 2), BADARG, "d_P is not 4-byte aligned"),
            (dict(x=X + 2), BADARG, "d_x is not 4-byte aligned"),
            (dict(ws=0), BADARG, f"workspace is NULL: the chunk sums need {need} bytes"),
            (dict(ws=W + 4), BADARG, "workspace is not 8-byte aligned"),
            (dict(ws_bytes=8), WORKSPACE, f"workspace of 8 bytes, the chunk and block sums need {need}"),
            (dict(x=P), BADARG, "d_x and d_P overlap"),
            (dict(ws=X), BADARG, "workspace overlaps d_x or d_P")):
        assert lib.bhw_welch_cfft_f32_device(ref, 400, 0, None, *tail(s, **kw)) == code and _err() == text, (kw, _err())
    assert lib.bhw_welch_cfft_f32_device(ref, 400, 0, None, *tail(_seg(n_fft=512, y_stride=3))) == BADARG
    assert _err() == "y_stride 3, y_batch_stride 0: no spectrum is written, both must be 0"
    assert lib.bhw_welch_cfft_f32_from_table(None, ref, 400, None, *tail(s)) == BADARG and _err() == "table is NULL"
    # the forward mixed-radix I/Q call and the real mixed-radix Welch call
    s = _seg(y_stride=2 * N + 1)
    assert lib.bhw_stft_cmfft_f32_device(ref, 400, 0, None, ctypes.byref(s), DETREND, ctypes.c_void_p(X), ctypes.c_void_p(P)) == BADARG
    assert _err() == f"y_stride {2 * N + 1}: at least 2 * n_fft = {2 * N} floats, and even"
    assert lib.bhw_describe_welch_mfft(None, ref, 400, ctypes.byref(_seg(channels=1, n_fft=512)), 1, buf, 1280) == UNSUPPORTED
    assert "power of two" in _err()
    assert lib.bhw_describe_welch_mfft(None, ref, 400, ctypes.byref(_seg()), 1, buf, 1280) == UNSUPPORTED and "channels 2" in _err()
    # the lines are as they were
    big = dict(batch=64, samples=160000, frames=998)
    assert B.describe_stft_cmfft(p, 400, _seg(n_fft=400, **big), detrend=True) == (
        "stft cmfft direct (L = 400, n_fft 400, col0 0, pad 0 constant, constant detrend), spectrum rows, bins in order: k_stft_cmfft_direct<2>, "
        "64 signals x 998 frames = 63872 rows, complex FFT of 400 points in passes 5x5x4x4 (no split), 128 lanes per row x 2 rows per "
        "workgroup, 4 columns per lane, 31936 groups, grid 2048 x 256 lanes, 14416 bytes of LDS, 200 twiddles")
    assert B.describe_welch_cfft(p, 400, _seg(n_fft=512, **big), detrend=True) == (
        "welch cfft direct (L = 400, n_fft 512, col0 0, pad 0 constant, constant detrend), bins in order: k_welch_cfft_direct<2>, "
        "64 signals x 998 frames = 63872 rows, complex FFT of 512 points in passes 4x4x4x4x2 (no split), 128 lanes per row x 2 rows per "
        "workgroup, 4 columns per lane, 32256 groups, grid 2048 x 256 lanes, 18448 bytes of LDS; chunk 16 frames, 4032 runs of 16 frames "
        "(8 groups per run), 2 accumulators per lane, 63 chunks and 4 blocks per signal, then k_welch_fft_join twice (chunks, blocks), "
        f"workspace {8 * 64 * 512 * 67} bytes")


def test_the_python_refusals_name_the_welch_calls():
    """The input wrapper of the two Python calls, on CPU tensors (the dtype and the size are checked before the device)."""
    torch = pytest.importorskip("torch")
    from blackman_harris_win_amd import selector
    z = torch.zeros(4000, dtype=torch.complex64)
    with pytest.raises(ValueError, match=r"n_fft 512 is a power of two: welch_fft_iq / welch_fused_iq transform it"):
        selector._welch_cmfft_input(torch, z, 512, 0)
    with pytest.raises(ValueError, match=r"real input at a mixed-radix n_fft: welch_fft_mixed / welch_fused_mixed"):
        selector._welch_cmfft_input(torch, z.real, 600, 0)
    with pytest.raises(ValueError, match=r"takes complex64 input, got torch.complex128"):
        selector._welch_cmfft_input(torch, z.to(torch.complex128), 600, 0)
    for n in (2048, 14, 21, 448):
        with pytest.raises(ValueError, match="power of two" if n == 2048 else r"2\^a·3\^b·5\^c in 16..2047, got " + str(n)):
            selector._welch_cmfft_input(torch, z, n, 0)
    selector._welch_cmfft_input(torch, z, 600, 0)


def test_python_surface():
    for name in ("welch_fft_iq_mixed", "welch_fused_iq_mixed", "describe_welch_cmfft", "welch_cmfft_workspace_bytes"):
        assert name in bhw.__all__ and hasattr(bhw, name)
    assert B.describe_welch_cmfft is bhw.describe_welch_cmfft and B.welch_cmfft_workspace_bytes is bhw.welch_cmfft_workspace_bytes
    assert inspect.signature(B.describe_welch_cmfft) == inspect.signature(B.describe_welch_cfft)
    for new, old in (("welch_fft_iq_mixed", "welch_fft_iq"), ("welch_fused_iq_mixed", "welch_fused_iq")):
        sig = inspect.signature(getattr(bhw, new))
        assert sig == inspect.signature(getattr(bhw, old)), new          # names, order, defaults and kinds
        assert inspect.signature(getattr(bhw.ResidentTable, new)) == inspect.signature(getattr(bhw.ResidentTable, old))
        assert list(inspect.signature(getattr(bhw.ResidentTable, new)).parameters)[1:] == list(sig.parameters)
    sig = inspect.signature(bhw.welch_fft_iq_mixed)
    assert list(sig.parameters) == ["params", "x", "n_fft", "hop", "scale", "win_length", "center", "pad_mode", "detrend", "shift", "fftshift",
                                    "out", "workspace"]
    sig = inspect.signature(bhw.welch_fused_iq_mixed)
    assert list(sig.parameters) == ["params", "x", "fs", "length", "noverlap", "nfft", "detrend", "scaling", "shift", "fftshift", "out", "workspace"]
    assert "fft" not in sig.parameters and "average" not in sig.parameters
    assert "mean" in bhw.welch_fused_iq_mixed.__doc__ and "fftfreq" in bhw.welch_fused_iq_mixed.__doc__
    from blackman_harris_win_amd import selector
    assert inspect.signature(selector._freq_axis_iq).parameters["kind"].default == "freqs_iq"
    with pytest.raises(ValueError, match="'torch' or 'fused'"):
        selector._fft_check("iq_mixed")
