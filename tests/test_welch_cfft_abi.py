"""The fused Welch PSD calls for I/Q input (bhw_welch_cfft_f32_device / _from_table / bhw_welch_cfft_workspace_bytes /
bhw_describe_welch_cfft): the checks that need no GPU -- exports and declarations, every refusal of include/bhw.h with its code and
words, in the stated order and before any HIP call, the workspace formula, frames 0, the describe line, the messages of the existing
families, and the Python surface."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import welch_cfft_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
NEW_SYMBOLS = ("bhw_welch_cfft_workspace_bytes", "bhw_welch_cfft_f32_device", "bhw_welch_cfft_f32_from_table", "bhw_describe_welch_cfft")
# never dereferenced: every call below fails or has nothing to do
X, P, W = 0x10000000, 0x80000000, 0x40000000
N = 512
DETREND, POWER, SHIFT = 1, 2, 4


def _err():
    return B.lib().bhw_last_error().decode()


def _seg(**kw):
    """Welch framing of I/Q input: 4 signals of 16000 complex samples, window 400 in rows of 512, hop 160, no padding: 98 frames, 7
    chunks, one block."""
    a = dict(batch=4, samples=16000, frames=98, hop=160, n_fft=N, channels=2, shift=31)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _need(s):
    return 8 * WC.workspace_doubles(s.batch, s.frames, s.n_fft)


def _calls(s, flags=DETREND, L=400, scale=1.0, x=X, out=P, p_stride=0, ws=W, ws_bytes=None):
    lib = B.lib()
    sr = ctypes.byref(s) if s is not None else None
    nbytes = (_need(s) if s is not None else 0) if ws_bytes is None else ws_bytes
    tail = (sr, flags, scale, ctypes.c_void_p(x), ctypes.c_void_p(out), p_stride, ctypes.c_void_p(ws), nbytes)
    return (lambda p: lib.bhw_welch_cfft_f32_device(p, L, 0, None, *tail),
            lambda p: lib.bhw_welch_cfft_f32_from_table(None, p, L, None, *tail))


def _passes(ref, s, **kw):
    """Every check passed: the from-table call with no table stops at 'table is NULL', before any launch."""
    rc = _calls(s, **kw)[1](ref)
    return rc == BADARG and "table is NULL" in _err()


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\b(int|uint64_t) " + name + r"\(", header), name
    assert L.bhw_abi_version() == 4
    # the order is the header's: the two constants stand where they stood
    assert re.search(r"#define BHW_WELCH_FFT_CHUNK 16u", header) and re.search(r"#define BHW_WELCH_BLOCK 256u", header)
    at = header.index("Fused Welch PSD for complex (I/Q) input")
    text = header[at:header.index("uint64_t bhw_welch_cfft_workspace_bytes")]
    for words in ("not on B, the grid", "bit for bit", "within one float32 ulp", "no float\n *     atomics", "Not built", "BHW_CFFT_POWER is refused",
                  "no psd_flags", "(j + n_fft / 2) mod"):
        assert words in text, words
    # there is no psd_flags argument: the argument order is bhw_welch_fft_f32_*'s without it
    proto = re.search(r"int bhw_welch_cfft_f32_device\(([^;]*)\);", header).group(1)
    real = re.search(r"int bhw_welch_fft_f32_device\(([^;]*)\);", header).group(1)
    names = lambda t: [a.split()[-1].lstrip("*") for a in re.sub(r"\s+", " ", t).split(",")]
    assert names(proto) == [n for n in names(real) if n != "psd_flags"]
    assert ctypes.sizeof(B.BhwStft) == 96 and ctypes.sizeof(B.BhwPsd) == 72


def test_input_side_errors_are_the_forward_calls():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    cases = [
        (dict(struct_size=8), BADARG, "struct_size"),
        (dict(channels=3), BADARG, "channels"),
        (dict(channels=1), UNSUPPORTED, "real input: bhw_stft_fft_f32_*"),
        (dict(batch=0), BADARG, "batch is 0"),
        (dict(hop=0), BADARG, "hop is 0"),
        (dict(n_fft=0), BADARG, "n_fft"),
        (dict(n_fft=256), BADARG, "col0 + L"),
        (dict(n_fft=500), UNSUPPORTED, "n_fft 500: the fused complex FFT takes a power of two in 16..2048"),
        (dict(n_fft=4096), UNSUPPORTED, "n_fft 4096: the fused complex FFT takes a power of two in 16..2048"),
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
            assert B.lib().bhw_describe_stft_cfft(None, ref, 400, ctypes.byref(s), flags, buf, 1280) == code and _err() == want, (kw, want, _err())
        assert _passes(ref, _seg(), flags=flags)
    # n_fft 400 (mixed radix) with a window that fits: that call's words
    for call in _calls(_seg(n_fft=400)):
        assert call(ref) == UNSUPPORTED and _err() == "n_fft 400: the fused complex FFT takes a power of two in 16..2048"
    for kw, text in ((dict(pad=256), "pad 256"), (dict(col0=56), "col0 56"), (dict(pad_mode=B.PAD_REFLECT), "pad_mode 1")):
        for call in _calls(_seg(**kw), flags=DETREND):
            assert call(ref) == BADARG and text in _err(), (kw, _err())
    # the padding fields as the forward call accepts them: a centred, reflect-padded descriptor
    assert _passes(ref, _seg(pad=256, col0=56, pad_mode=B.PAD_REFLECT, frames=101), flags=0)
    for call in _calls(_seg(pad=256, col0=56, pad_mode=B.PAD_REFLECT, frames=102), flags=0):
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
            assert call(ref) == BADARG and "BHW_CFFT_POWER" in _err() and "no meaning" in _err(), _err()
        # also with frames 0, and from the describe call
        assert B.lib().bhw_welch_cfft_f32_device(ref, 400, 0, None, ctypes.byref(_seg(frames=0)), flags, 1.0, None, None, 0, None, 0) == BADARG
        buf = ctypes.create_string_buffer(1280)
        assert B.lib().bhw_describe_welch_cfft(None, ref, 400, ctypes.byref(_seg()), flags, buf, 1280) == BADARG
    # the forward call still takes it
    buf = ctypes.create_string_buffer(1280)
    assert B.lib().bhw_describe_stft_cfft(None, ref, 400, ctypes.byref(_seg()), POWER, buf, 1280) == OK


def test_output_side_errors_in_the_stated_order():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    s = _seg()
    # 2. no spectrum is written: non-zero y strides are refused, whatever their value
    for kw in (dict(y_stride=2 * N), dict(y_batch_stride=98 * 2 * N), dict(y_stride=2 * N + 2, y_batch_stride=98 * (2 * N + 2)), dict(y_stride=3)):
        for call in _calls(_seg(**kw)):
            assert call(ref) == BADARG and "no spectrum is written" in _err(), (kw, _err())
    for scale in (float("inf"), float("-inf"), float("nan")):
        for call in _calls(s, scale=scale):
            assert call(ref) == BADARG and "scale is not finite" in _err()
    for scale in (0.0, -1.5, 1e300):
        assert _passes(ref, s, scale=scale)
    # 4.
    for call in _calls(s, p_stride=N - 1):
        assert call(ref) == BADARG and "p_stride" in _err()
    assert _passes(ref, s, p_stride=N) and _passes(ref, s, p_stride=N + 7)
    # The stated limit, batch * ceil(frames / 16) * n_fft above 2^34, cannot be the first to refuse: ceil(F / 16) <= F, and the forward
    # checks, which run first, hold batch * frames * n_fft to 2^34.  What is matched here is THEIR message.
    big = (1 << 34) // (98 * N) + 1
    for call in _calls(_seg(batch=big), ws_bytes=1 << 60):
        assert call(ref) == BADARG and _err() == "batch * frames * n_fft above 2^34 per call", _err()
    # 5.
    for kw in (dict(x=0), dict(out=0)):
        for call in _calls(s, **kw):
            assert call(ref) == BADARG and "NULL" in _err()
    for call in _calls(s, out=P + 2):
        assert call(ref) == BADARG and "d_P is not 4-byte aligned" in _err()
    assert _passes(ref, s, out=P + 4)
    for call in _calls(s, x=X + 2):
        assert call(ref) == BADARG and "d_x is not 4-byte aligned" in _err()
    assert _passes(ref, s, x=X + 4)                  # complex samples need no 8-byte alignment: the kernel then loads the parts apart
    # 6. the workspace: NULL, misaligned, short (its own code), and exactly enough
    for call in _calls(s, ws=0):
        assert call(ref) == BADARG and "workspace is NULL" in _err()
    for call in _calls(s, ws=W + 4):
        assert call(ref) == BADARG and "workspace is not 8-byte aligned" in _err()
    for call in _calls(s, ws_bytes=_need(s) - 1):
        assert call(ref) == WORKSPACE and "workspace of" in _err()
    for call in _calls(s, ws_bytes=0):
        assert call(ref) == WORKSPACE
    assert _passes(ref, s, ws_bytes=_need(s)) and _passes(ref, s, ws_bytes=_need(s) + 8)
    # 7. overlaps: x holds 4 * 16000 complex = 4 * 32000 floats, P 4 * 512 floats, the workspace _need(s) bytes
    xb, pb, wb = 4 * 32000 * 4, 4 * N * 4, _need(s)
    for kw, bad, text in (
            (dict(x=X, out=X + xb - 4), True, "d_x and d_P overlap"), (dict(x=X, out=X + xb), False, ""),
            (dict(x=P + pb - 4, out=P), True, "d_x and d_P overlap"), (dict(x=P + pb, out=P), False, ""),
            (dict(x=X, ws=X + xb - 8), True, "workspace overlaps"), (dict(x=X, ws=X + xb), False, ""),
            (dict(x=W + wb - 4, ws=W), True, "workspace overlaps"), (dict(x=W + wb, ws=W), False, ""),
            (dict(out=P, ws=P + pb - 8), True, "workspace overlaps"), (dict(out=W + wb - 4, ws=W), True, "workspace overlaps"),
            (dict(out=W + wb, ws=W), False, "")):
        if bad:
            for call in _calls(s, **kw):
                assert call(ref) == BADARG and text in _err(), (kw, _err())
        else:
            assert _passes(ref, s, **kw), (kw, _err())
    # the order: each refusal wins over everything stated after it
    order = [
        (dict(s=_seg(n_fft=4096, y_stride=3), flags=POWER, scale=float("nan")), UNSUPPORTED, "power of two"),          # 1 before 2
        (dict(s=_seg(y_stride=3), flags=POWER, scale=float("nan")), BADARG, "BHW_CFFT_POWER"),                          # 2: the flag,
        (dict(s=_seg(y_stride=3), scale=float("nan")), BADARG, "no spectrum is written"),                               #    the strides,
        (dict(s=s, scale=float("nan"), p_stride=1), BADARG, "scale is not finite"),                                     #    the scale
        (dict(s=s, p_stride=1, x=0), BADARG, "p_stride"),                                                               # 4 before 5
        (dict(s=s, x=0, ws=0), BADARG, "d_x / d_P is NULL"),                                                            # 5 before 6
        (dict(s=s, out=P + 2, ws=W + 4), BADARG, "d_P is not 4-byte aligned"),
        (dict(s=s, ws=W + 4, ws_bytes=0), BADARG, "workspace is not 8-byte aligned"),
        (dict(s=s, ws_bytes=8, x=P), WORKSPACE, "workspace of 8 bytes"),                                                # 6 before 7
        (dict(s=s, x=P), BADARG, "d_x and d_P overlap"),                                                                # 7 before 8
    ]
    for kw, code, text in order:
        kw = dict(kw)
        for call in _calls(kw.pop("s"), **kw):
            assert call(ref) == code and text in _err(), (kw, code, _err())


@pytest.mark.parametrize("cid", WC.case_ids())
def test_workspace_bytes_equal_the_formula(cid):
    c = WC.case(cid)
    s, _, F, _ = WC.desc(c)
    n = c["n_fft"]
    chunks, blocks = -(-F // 16), -(-F // 256)
    want = 8 * c["B"] * n * (chunks + (blocks if blocks > 1 else 0))
    assert B.welch_cfft_workspace_bytes(s) == want == WC.parse(WC.line(c))["workspace"]
    p = WC.params(c["setup"])
    for flags in (int(c["detrend"]), int(c["detrend"]) | SHIFT):
        assert _passes(ctypes.byref(p), s, L=c["L"], flags=flags, ws_bytes=want), _err()
        for call in _calls(s, L=c["L"], flags=flags, ws_bytes=want - 8):
            assert call(ctypes.byref(p)) == WORKSPACE, _err()


def test_workspace_bytes_of_nothing():
    assert B.lib().bhw_welch_cfft_workspace_bytes(None) == 0
    assert B.welch_cfft_workspace_bytes(_seg(frames=0)) == 0
    s = _seg()
    s.struct_size = 80
    assert B.welch_cfft_workspace_bytes(s) == 0


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1280)
    for n in list(range(1, 300)) + [400, 500, 511, 512, 513, 1024, 2048, 3000, 4096, 4097, 8192]:
        s = B.make_stft(2, 100000, 3, 7, n, channels=2, shift=31)
        rc = lib.bhw_describe_welch_cfft(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), DETREND, buf, 1280)
        assert rc == (OK if B.cfft_supported(n) else UNSUPPORTED), (n, rc, _err())
    # real input is refused with the forward call's words
    s = B.make_stft(2, 100000, 3, 7, 512, channels=1, shift=31)
    assert lib.bhw_describe_welch_cfft(None, ctypes.byref(p), 16, ctypes.byref(s), DETREND, buf, 1280) == UNSUPPORTED
    assert _err() == "channels 1: the fused complex FFT takes interleaved I/Q input (2); real input: bhw_stft_fft_f32_*"


def test_frames_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    for flags in (0, DETREND, SHIFT):
        s = _seg(frames=0)
        assert lib.bhw_welch_cfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, None, None, 0, None, 0) == OK
        assert lib.bhw_welch_cfft_f32_from_table(None, ctypes.byref(p), 400, None, ctypes.byref(s), flags, 1.0, None, None, 0, None, 0) == BADARG
        assert "table is NULL" in _err()
        assert "nothing (frames 0)" in B.describe_welch_cfft(p, 400, s, detrend=bool(flags & DETREND), fftshift=bool(flags & SHIFT))
        # what is checked before frames 0 returns: the descriptor, the flag, the strides, the scale
        assert lib.bhw_welch_cfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, float("nan"), None, None, 0, None, 0) == BADARG
        assert lib.bhw_welch_cfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(_seg(frames=0, y_stride=1024)), flags, 1.0, None, None, 0,
                                             None, 0) == BADARG
        # and what is not: p_stride
        assert lib.bhw_welch_cfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, None, None, 1, None, 0) == OK
        s = _seg(frames=0, n_fft=768)
        assert lib.bhw_welch_cfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, None, None, 0, None, 0) == UNSUPPORTED


def test_describe_line_parses():
    p = B.make_params(B.WIN_BH7, 16, 32)
    s = _seg(batch=64, samples=160000, frames=998)
    d = WC.parse(B.describe_welch_cfft(p, 400, s, detrend=True))
    assert d["line"].startswith("welch cfft direct (L = 400, n_fft 512, col0 0, pad 0 constant, constant detrend), bins in order: "
                                "k_welch_cfft_direct<2>")
    assert (d["signals"], d["frames"], d["rows"], d["m"], d["schedule"]) == (64, 998, 63872, 512, "4x4x4x4x2")
    assert (d["lpf"], d["fy"], d["cpl"], d["lds"]) == (128, 2, 4, 2 * 2 * 512 * 8 + 256 * 8 + 16)
    # 998 frames pad to 1008 = 63 runs of 16 frames per signal, eight groups each
    assert (d["chunk"], d["run"], d["gpr"], d["runs"], d["groups"], d["grid"]) == (16, 16, 8, 64 * 63, 64 * 63 * 8, 2048)
    assert (d["acc"], d["chunks"], d["blocks"], d["joins"], d["workspace"]) == (2, 63, 4, 2, 8 * 64 * 512 * (63 + 4))
    assert "bins shifted" in B.describe_welch_cfft(p, 400, s, detrend=True, fftshift=True)
    # one signal of 2^24 samples at 2048 / hop 512
    t2 = WC.parse(B.describe_welch_cfft(p, 2048, B.make_stft(1, 1 << 24, 32765, 512, 2048, channels=2, shift=31), detrend=True))
    assert (t2["runs"], t2["chunks"], t2["blocks"], t2["acc"], t2["gpr"], t2["grid"]) == (2048, 2048, 128, 8, 16, 2048)
    with pytest.raises(B.BhwError):
        B.describe_welch_cfft(p, 400, _seg(n_fft=500))
    buf = ctypes.create_string_buffer(16)
    assert B.lib().bhw_describe_welch_cfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, buf, 16) == OK and len(buf.value) == 15
    assert B.lib().bhw_describe_welch_cfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, None, 0) == BADARG


def test_the_existing_families_keep_their_messages():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1280)
    s = _seg(y_stride=2 * N + 1)
    assert lib.bhw_stft_cfft_f32_device(ref, 400, 0, None, ctypes.byref(s), DETREND, ctypes.c_void_p(X), ctypes.c_void_p(P)) == BADARG
    assert _err() == f"y_stride {2 * N + 1}: at least 2 * n_fft = {2 * N} floats, and even"
    s = _seg(y_stride=N - 1)
    assert lib.bhw_stft_cfft_f32_device(ref, 400, 0, None, ctypes.byref(s), DETREND | POWER, ctypes.c_void_p(X), ctypes.c_void_p(P)) == BADARG
    assert _err() == f"y_stride {N - 1}: at least n_fft = {N} floats"
    # the real-input Welch call: its words, its workspace of K = 257 bins, its psd_flags
    r = _seg(channels=1)
    K = N // 2 + 1
    tail = (ctypes.byref(r), 1, 1.0, 1, ctypes.c_void_p(X), ctypes.c_void_p(P), 0, ctypes.c_void_p(W))
    assert lib.bhw_welch_fft_f32_device(ref, 400, 0, None, *tail, 8) == WORKSPACE
    assert _err() == f"workspace of 8 bytes, the chunk and block sums need {8 * 4 * K * 7}"
    assert B.welch_fft_workspace_bytes(r) == 8 * 4 * K * 7
    assert lib.bhw_welch_fft_f32_device(ref, 400, 0, None, ctypes.byref(_seg()), 1, 1.0, 1, ctypes.c_void_p(X), ctypes.c_void_p(P), 0,
                                        ctypes.c_void_p(W), 1 << 30) == UNSUPPORTED
    assert "real input" in _err()
    assert lib.bhw_describe_welch_fft(None, ref, 400, ctypes.byref(_seg(channels=1, n_fft=500)), 1, buf, 1280) == UNSUPPORTED
    assert _err() == "n_fft 500: the fused FFT takes a power of two in 16..4096"
    # the forward lines are as they were
    big = dict(batch=64, samples=160000, frames=998)
    assert B.describe_stft_cfft(p, 400, _seg(**big), detrend=True) == (
        "stft cfft direct (L = 400, n_fft 512, col0 0, pad 0 constant, constant detrend), spectrum rows, bins in order: k_stft_cfft_direct<2>, "
        "64 signals x 998 frames = 63872 rows, complex FFT of 512 points in passes 4x4x4x4x2 (no split), 128 lanes per row x 2 rows per "
        "workgroup, 4 columns per lane, 31936 groups, grid 2048 x 256 lanes, 18448 bytes of LDS")
    line = B.describe_welch_fft(p, 400, _seg(channels=1, **big), detrend=True)
    assert line.startswith("welch fft direct (L = 400, n_fft 512, col0 0, pad 0 constant, constant detrend): k_welch_fft_direct<2>")
    assert line.endswith("chunk 16 frames, 4032 runs of 16 frames (4 groups per run), 2 accumulators per lane, 63 chunks and 4 blocks per signal, "
                         f"then k_welch_fft_join twice (chunks, blocks), workspace {8 * 64 * K * 67} bytes")


def test_complex_input_is_refused_or_routed_as_before():
    from blackman_harris_win_amd import selector
    p = B.make_params(B.WIN_HANN, 10, 16)
    with pytest.raises(ValueError, match="'torch' or 'fused'"):
        selector._fft_check("iq")
    for name in ("welch", "welch_fft", "welch_fused"):
        assert "fftshift" not in inspect.signature(getattr(bhw, name)).parameters
    assert "fft" not in inspect.signature(bhw.welch_fused_iq).parameters and "fft" not in inspect.signature(bhw.welch_fft_iq).parameters
    assert list(inspect.signature(bhw.welch).parameters) == ["params", "x", "fs", "length", "noverlap", "nfft", "detrend", "return_onesided",
                                                             "scaling", "shift", "average", "fft"]
    assert list(inspect.signature(bhw.welch_fused).parameters) == ["params", "x", "fs", "length", "noverlap", "nfft", "detrend", "scaling",
                                                                   "shift", "out", "workspace"]


def test_python_surface():
    for name in ("welch_fft_iq", "welch_fused_iq", "describe_welch_cfft", "welch_cfft_workspace_bytes"):
        assert name in bhw.__all__ and hasattr(bhw, name)
    assert B.describe_welch_cfft is bhw.describe_welch_cfft and B.welch_cfft_workspace_bytes is bhw.welch_cfft_workspace_bytes
    sig = inspect.signature(bhw.welch_fft_iq)
    assert list(sig.parameters) == ["params", "x", "n_fft", "hop", "scale", "win_length", "center", "pad_mode", "detrend", "shift", "fftshift",
                                    "out", "workspace"]
    assert sig.parameters["center"].default is False and sig.parameters["pad_mode"].default == "reflect"
    assert sig.parameters["detrend"].default is False and sig.parameters["fftshift"].default is False
    assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for n, q in sig.parameters.items() if n not in ("params", "x", "n_fft", "hop", "scale"))
    assert list(inspect.signature(bhw.ResidentTable.welch_fft_iq).parameters)[1:] == list(sig.parameters)
    sig = inspect.signature(bhw.welch_fused_iq)
    assert list(sig.parameters) == ["params", "x", "fs", "length", "noverlap", "nfft", "detrend", "scaling", "shift", "fftshift", "out", "workspace"]
    assert sig.parameters["fs"].default == 1.0 and sig.parameters["detrend"].default == "constant" and sig.parameters["scaling"].default == "density"
    assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for n, q in sig.parameters.items() if n not in ("params", "x", "fs"))
    assert list(inspect.signature(bhw.ResidentTable.welch_fused_iq).parameters)[1:] == list(sig.parameters)
    assert "average" not in sig.parameters and "mean" in bhw.welch_fused_iq.__doc__ and "fftfreq" in bhw.welch_fused_iq.__doc__
