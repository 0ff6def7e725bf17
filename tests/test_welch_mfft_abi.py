"""The fused Welch PSD calls at a mixed-radix n_fft (bhw_welch_mfft_f32_device / _from_table / bhw_welch_mfft_workspace_bytes /
bhw_describe_welch_mfft): the checks that need no GPU -- exports and declarations, every refusal of include/bhw.h with its code and
words in the stated order before any HIP call (one call that breaks two adjacent rules for each adjacent pair), the workspace formula,
frames 0, the describe line, the messages of the existing families, and the Python surface."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import welch_mfft_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
NEW_SYMBOLS = ("bhw_welch_mfft_workspace_bytes", "bhw_welch_mfft_f32_device", "bhw_welch_mfft_f32_from_table", "bhw_describe_welch_mfft")
DETREND, POWER = B.WELCH_DETREND_CONSTANT, B.MFFT_POWER
# never dereferenced: every call below fails or has nothing to do
X, P, W = 0x10000000, 0x80000000, 0x40000000
K = 201


def _err():
    return B.lib().bhw_last_error().decode()


def _seg(**kw):
    """Welch framing: 4 signals of 16000, window 400 in rows of 400, hop 160, no padding: 98 frames, 7 chunks, one block."""
    a = dict(batch=4, samples=16000, frames=98, hop=160, n_fft=400, shift=31)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _need(s):
    return 8 * WC.workspace_doubles(s.batch, s.frames, s.n_fft // 2 + 1)


def _calls(s, flags=DETREND, L=400, scale=1.0, psd_flags=1, x=X, out=P, p_stride=0, ws=W, ws_bytes=None):
    lib = B.lib()
    sr = ctypes.byref(s) if s is not None else None
    nbytes = (_need(s) if s is not None else 0) if ws_bytes is None else ws_bytes
    tail = (sr, flags, scale, psd_flags, ctypes.c_void_p(x), ctypes.c_void_p(out), p_stride, ctypes.c_void_p(ws), nbytes)
    return (lambda p: lib.bhw_welch_mfft_f32_device(p, L, 0, None, *tail),
            lambda p: lib.bhw_welch_mfft_f32_from_table(None, p, L, None, *tail))


def _passes(ref, s, **kw):
    """Every check passed: the from-table call with no table stops at 'table is NULL', before any launch."""
    rc = _calls(s, **kw)[1](ref)
    return rc == BADARG and "table is NULL" in _err()


def _refused(ref, s, code, text, **kw):
    for call in _calls(s, **kw):
        assert call(ref) == code and text in _err(), (kw, code, text, _err())
    return _err()


def _prototype(header, name):
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\b(int|uint64_t) " + name + r"\(", header), name
    assert L.bhw_abi_version() == 4                                    # additions only
    at = header.index("Fused Welch PSD at a mixed-radix n_fft")
    text = header[at:header.index("uint64_t bhw_welch_mfft_workspace_bytes")]
    for words in ("not on B, the grid", "bit for bit", "within one float32 ulp", "no float atomics", "No call\n *     allocates", "Not built",
                  "8-byte aligned", "BHW_MFFT_POWER is refused", "no filter-bank"):
        assert words in text, words
    assert ctypes.sizeof(B.BhwStft) == 96 and ctypes.sizeof(B.BhwPsd) == 72


def test_the_prototypes_are_bhw_welch_fft_f32s_word_for_word():
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for form in ("device", "from_table"):
        assert _prototype(header, f"bhw_welch_mfft_f32_{form}") == _prototype(header, f"bhw_welch_fft_f32_{form}")
        assert getattr(B.lib(), f"bhw_welch_mfft_f32_{form}").argtypes == getattr(B.lib(), f"bhw_welch_fft_f32_{form}").argtypes
    assert _prototype(header, "bhw_describe_welch_mfft") == _prototype(header, "bhw_describe_welch_fft")
    assert "(p, length, s, flags, scale, psd_flags, d_x, d_P, p_stride, workspace, workspace_bytes)" in \
        re.sub(r"int device, |void \*hip_stream, |const \w+ \*|\w+ \*|double |uint\d+_t |float \*", "",
               "(" + _prototype(header, "bhw_welch_mfft_f32_device") + ")").replace("const ", "")


def test_input_side_errors_are_the_forward_calls():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    cases = [
        (dict(struct_size=8), 400, BADARG, "struct_size"),
        (dict(channels=3), 400, BADARG, "channels"),
        (dict(channels=2), 400, UNSUPPORTED, "channels 2: the mixed-radix fused FFT takes real input (1)"),
        (dict(batch=0), 400, BADARG, "batch is 0"),
        (dict(hop=0), 400, BADARG, "hop is 0"),
        (dict(n_fft=0), 400, BADARG, "n_fft"),
        (dict(n_fft=200), 400, BADARG, "col0 + L"),
        (dict(n_fft=512), 400, UNSUPPORTED, "n_fft 512 is a power of two: bhw_stft_fft_f32_* and bhw_spectrogram_f32_* transform it"),
        (dict(n_fft=4096, frames=50), 400, UNSUPPORTED, "n_fft 4096 is a power of two"),
        (dict(n_fft=14), 14, UNSUPPORTED, "n_fft 14: the mixed-radix fused FFT takes an even 2^a 3^b 5^c in 16..4095"),
        (dict(n_fft=401), 400, UNSUPPORTED, "n_fft 401: the mixed-radix fused FFT"),
        (dict(n_fft=448), 400, UNSUPPORTED, "n_fft 448: the mixed-radix fused FFT"),
        (dict(shift=63), 400, BADARG, "shift"),
        (dict(frames=99), 400, BADARG, "segment 98 leaves the signal"),
        (dict(samples=0), 400, BADARG, "samples is 0"),
        (dict(x_stride=15999), 400, BADARG, "x_stride"),
    ]
    buf = ctypes.create_string_buffer(1280)
    for flags in (0, DETREND):
        for kw, L, code, text in cases:
            s = _seg(**{k: v for k, v in kw.items() if k != "struct_size"})
            if "struct_size" in kw:
                s.struct_size = kw["struct_size"]
            want = _refused(ref, s, code, text, flags=flags, L=L)
            # the same code and the same words as the forward call
            assert B.lib().bhw_describe_stft_mfft(None, ref, L, ctypes.byref(s), flags, None, buf, 1280) == code and _err() == want, (kw, want, _err())
        assert _passes(ref, _seg(), flags=flags)
    # an unknown flag: the forward call's code and words, whatever else is set
    for flags in (4, 8, DETREND | 4, POWER | 16):
        want = _refused(ref, _seg(), BADARG, f"flags 0x{flags:x} (any of BHW_WELCH_DETREND_CONSTANT, BHW_MFFT_POWER)", flags=flags)
        assert B.lib().bhw_describe_stft_mfft(None, ref, 400, ctypes.byref(_seg()), flags, None, buf, 1280) == BADARG and _err() == want
    for kw, text in ((dict(pad=200), "pad 200"), (dict(col0=56), "col0 56"), (dict(pad_mode=B.PAD_REFLECT), "pad_mode 1")):
        _refused(ref, _seg(**kw), BADARG, text, flags=DETREND, L=320)
    # the padding fields as the forward call accepts them: a centred, reflect-padded descriptor
    assert _passes(ref, _seg(pad=200, col0=40, pad_mode=B.PAD_REFLECT, frames=101), flags=0, L=320)
    _refused(ref, _seg(pad=200, col0=40, pad_mode=B.PAD_REFLECT, frames=102), BADARG, "leaves the padded signal", flags=0, L=320)
    _refused(ref, None, BADARG, "descriptor is NULL")
    for call in _calls(_seg()):
        assert call(None) == BADARG
    _refused(ref, _seg(), BADARG, "length", L=0)
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    for call in _calls(_seg()):
        assert call(ctypes.byref(taylor)) == UNSUPPORTED


def test_output_side_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    s = _seg()
    # BHW_MFFT_POWER is a flag the forward call knows: it passes that call's checks and is refused here
    for flags in (POWER, POWER | DETREND):
        _refused(ref, s, BADARG, "BHW_MFFT_POWER has no meaning here", flags=flags)
    # no spectrum is written: non-zero y strides are refused, whatever their value
    for kw in (dict(y_stride=2 * K), dict(y_batch_stride=98 * 2 * K), dict(y_stride=2 * K + 2, y_batch_stride=98 * (2 * K + 2)), dict(y_stride=3)):
        _refused(ref, _seg(**kw), BADARG, "no spectrum is written", flags=0)
    _refused(ref, s, BADARG, "psd_flags 0x2", psd_flags=2)
    for scale in (float("inf"), float("-inf"), float("nan")):
        _refused(ref, s, BADARG, "scale is not finite", scale=scale)
    for scale, fl in ((0.0, 0), (-1.5, 1), (1e300, 0)):
        assert _passes(ref, s, scale=scale, psd_flags=fl)
    _refused(ref, s, BADARG, f"p_stride {K - 1} < bins {K}", p_stride=K - 1)
    assert _passes(ref, s, p_stride=K) and _passes(ref, s, p_stride=K + 7)
    # The stated limit, batch * ceil(frames / 16) * K above 2^34, cannot be the first to refuse: ceil(F / 16) <= F, and the forward
    # checks, which run first, hold batch * frames * n_fft to 2^34.  What is matched here is THEIR message; the branch of
    # bhwp_welch_mfft_checks behind them is not reached by any descriptor.
    big = (1 << 34) // (98 * 400) + 1
    _refused(ref, _seg(batch=big), BADARG, "above 2^34 per call", ws_bytes=1 << 60)
    assert "ceil(frames" not in _err()
    for kw in (dict(x=0), dict(out=0)):
        _refused(ref, s, BADARG, "d_x / d_P is NULL", **kw)
    _refused(ref, s, BADARG, "d_P is not 4-byte aligned", out=P + 2)
    assert _passes(ref, s, out=P + 4)
    _refused(ref, s, BADARG, "d_x is not 4-byte aligned", x=X + 2)
    # the workspace: NULL, misaligned, short (its own code), and exactly enough
    _refused(ref, s, BADARG, "workspace is NULL", ws=0)
    _refused(ref, s, BADARG, "workspace is not 8-byte aligned", ws=W + 4)
    _refused(ref, s, WORKSPACE, "workspace of", ws_bytes=_need(s) - 1)
    _refused(ref, s, WORKSPACE, "workspace of 0 bytes", ws_bytes=0)
    assert _passes(ref, s, ws_bytes=_need(s)) and _passes(ref, s, ws_bytes=_need(s) + 8)
    # overlaps: x holds 4 * 16000 floats, P 4 * 201 floats, the workspace _need(s) bytes
    xb, pb, wb = 4 * 16000 * 4, 4 * K * 4, _need(s)
    for kw, bad, text in (
            (dict(x=X, out=X + xb - 4), True, "d_x and d_P overlap"), (dict(x=X, out=X + xb), False, ""),
            (dict(x=P + pb - 4, out=P), True, "d_x and d_P overlap"), (dict(x=P + pb, out=P), False, ""),
            (dict(x=X, ws=X + xb - 8), True, "workspace overlaps"), (dict(x=X, ws=X + xb), False, ""),
            (dict(x=W + wb - 4, ws=W), True, "workspace overlaps"), (dict(x=W + wb, ws=W), False, ""),
            (dict(out=P, ws=P + pb - 4 - (pb - 4) % 8), True, "workspace overlaps"), (dict(out=W + wb - 4, ws=W), True, "workspace overlaps"),
            (dict(out=W + wb, ws=W), False, "")):
        if bad:
            _refused(ref, s, BADARG, text, **kw)
        else:
            assert _passes(ref, s, **kw), (kw, _err())


def test_the_checks_run_in_the_stated_order():
    """One call that breaks two adjacent rules of include/bhw.h's list for each adjacent pair: the earlier rule's code and words."""
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    s = _seg()
    xb = 4 * 16000 * 4
    lib = B.lib()
    # 1 before 2: the forward call's refusals before BHW_MFFT_POWER
    _refused(ref, _seg(channels=2), UNSUPPORTED, "real input", flags=POWER)
    _refused(ref, _seg(n_fft=512), UNSUPPORTED, "power of two", flags=POWER)
    _refused(ref, s, BADARG, "any of BHW_WELCH_DETREND_CONSTANT", flags=POWER | 4)
    # inside 2: BHW_MFFT_POWER, the y strides, psd_flags, the scale
    _refused(ref, _seg(y_stride=2 * K), BADARG, "BHW_MFFT_POWER", flags=POWER)
    _refused(ref, _seg(y_stride=2 * K), BADARG, "no spectrum is written", flags=0, psd_flags=2)
    _refused(ref, s, BADARG, "psd_flags", psd_flags=2, scale=float("nan"))
    # 2 before 3: a scale that is not finite is refused with frames 0 too
    for call in _calls(_seg(frames=0), scale=float("nan")):
        assert call(ref) == BADARG and "scale is not finite" in _err()
    # 3 before 4, 6, 7 and 8: frames 0 with a p_stride below K, NULL pointers and no workspace is BHW_OK
    z = _seg(frames=0)
    assert lib.bhw_welch_mfft_f32_device(ref, 400, 0, None, ctypes.byref(z), 0, 1.0, 1, None, None, K - 1, None, 0) == OK
    # 4 before 5 and 6
    _refused(ref, _seg(batch=(1 << 34) // (7 * K) + 1, frames=98), BADARG, "above 2^34", p_stride=K - 1, ws_bytes=1 << 60)   # 1 holds it first
    _refused(ref, s, BADARG, "p_stride", p_stride=K - 1, x=0)
    # 6 before 7: a NULL or misaligned pointer before a short workspace
    _refused(ref, s, BADARG, "d_x / d_P is NULL", x=0, ws_bytes=8)
    _refused(ref, s, BADARG, "d_P is not 4-byte aligned", out=P + 1, ws_bytes=8)
    _refused(ref, s, BADARG, "workspace is NULL", ws=0, ws_bytes=0)
    _refused(ref, s, BADARG, "workspace is not 8-byte aligned", ws=W + 4, ws_bytes=8)
    # 7 before 8: a short workspace before an overlap
    _refused(ref, s, WORKSPACE, "workspace of 8 bytes", out=X + xb - 4, ws_bytes=8)
    _refused(ref, s, WORKSPACE, "workspace of 8 bytes", ws=X + 8, ws_bytes=8)
    # 8 before 9: an overlap before the table
    assert _calls(s, out=X + xb - 4)[1](ref) == BADARG and "d_x and d_P overlap" in _err()
    assert _passes(ref, s)


@pytest.mark.parametrize("cid", WC.case_ids())
def test_workspace_bytes_equal_the_formula(cid):
    c = WC.case(cid)
    s, _, F, _ = WC.desc(c)
    Kc = c["n_fft"] // 2 + 1
    chunks, blocks = -(-F // 16), -(-F // 256)
    want = 8 * c["B"] * Kc * (chunks + (blocks if blocks > 1 else 0))
    assert B.welch_mfft_workspace_bytes(s) == want == WC.parse(WC.line(c))["workspace"]
    p = WC.params(c["setup"])
    assert _passes(ctypes.byref(p), s, L=c["L"], flags=int(c["detrend"]), ws_bytes=want), _err()
    _refused(ctypes.byref(p), s, WORKSPACE, "workspace of", L=c["L"], flags=int(c["detrend"]), ws_bytes=want - 8)


def test_workspace_bytes_of_nothing():
    assert B.lib().bhw_welch_mfft_workspace_bytes(None) == 0
    assert B.welch_mfft_workspace_bytes(_seg(frames=0)) == 0
    s = _seg()
    s.struct_size = 80
    assert B.welch_mfft_workspace_bytes(s) == 0


def test_every_supported_size_passes_and_every_other_does_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1280)
    n_ok = 0
    for n in range(1, 4200):
        s = B.make_stft(2, 100000, 3, 7, n, shift=31)
        rc = lib.bhw_describe_welch_mfft(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), 1, buf, 1280)
        assert rc == (OK if B.mfft_supported(n) else UNSUPPORTED), (n, rc, _err())
        n_ok += rc == OK
    assert n_ok == 95


def test_frames_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    for flags in (0, DETREND):
        s = _seg(frames=0)
        assert lib.bhw_welch_mfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, 1, None, None, 0, None, 0) == OK
        assert lib.bhw_welch_mfft_f32_from_table(None, ctypes.byref(p), 400, None, ctypes.byref(s), flags, 1.0, 1, None, None, 0, None, 0) == BADARG
        assert "table is NULL" in _err()
        assert "nothing (frames 0)" in B.describe_welch_mfft(p, 400, s, detrend=bool(flags))
        # what is checked before frames 0 returns: the descriptor, the strides, the flags, the scale
        assert lib.bhw_welch_mfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, float("nan"), 1, None, None, 0, None, 0) == BADARG
        assert lib.bhw_welch_mfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, 4, None, None, 0, None, 0) == BADARG
        assert lib.bhw_welch_mfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags | POWER, 1.0, 1, None, None, 0, None, 0) == BADARG
        s = _seg(frames=0, n_fft=512)
        assert lib.bhw_welch_mfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, 1, None, None, 0, None, 0) == UNSUPPORTED


def test_describe_line_parses():
    p = B.make_params(B.WIN_BH7, 16, 32)
    s = _seg(batch=64, samples=160000, frames=998)
    d = WC.parse(B.describe_welch_mfft(p, 400, s, detrend=True))
    assert d["line"].startswith("welch mfft direct (L = 400, n_fft 400, col0 0, pad 0 constant, constant detrend): k_welch_mfft_direct<2>")
    assert (d["signals"], d["frames"], d["rows"], d["m"], d["schedule"]) == (64, 998, 63872, 200, "5x5x4x2")
    assert (d["lpf"], d["fy"], d["cpl"], d["lds"]) == (64, 4, 7, 2 * 4 * 200 * 8 + 200 * 8 + 16)
    # 998 frames pad to 1008 = 63 runs of 16 frames per signal, four groups each
    assert (d["chunk"], d["run"], d["gpr"], d["runs"], d["groups"], d["grid"]) == (16, 16, 4, 64 * 63, 64 * 63 * 4, 2048)
    assert (d["acc"], d["chunks"], d["blocks"], d["joins"], d["workspace"]) == (1, 63, 4, 2, 8 * 64 * 201 * (63 + 4))
    assert "rows," not in d["line"].split(": k_welch")[0] and d["form"] is None          # no output form
    # one signal of 2^24 samples at 4000 / hop 1000: 1 049 chunk chains
    t2 = WC.parse(B.describe_welch_mfft(p, 4000, B.make_stft(1, 1 << 24, 16774, 1000, 4000, shift=31), detrend=True))
    assert (t2["runs"], t2["chunks"], t2["blocks"], t2["acc"], t2["gpr"], t2["grid"]) == (1049, 1049, 66, 8, 16, 1049)
    with pytest.raises(B.BhwError):
        B.describe_welch_mfft(p, 400, _seg(n_fft=512))
    buf = ctypes.create_string_buffer(16)
    assert B.lib().bhw_describe_welch_mfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, buf, 16) == OK and len(buf.value) == 15
    assert B.lib().bhw_describe_welch_mfft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, None, 0) == BADARG


def test_the_existing_families_keep_their_messages():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1280)
    s = _seg(y_stride=2 * K + 1)
    assert lib.bhw_stft_mfft_f32_device(ref, 400, 0, None, ctypes.byref(s), DETREND, None, ctypes.c_void_p(X), ctypes.c_void_p(P)) == BADARG
    assert _err() == f"y_stride {2 * K + 1}: at least 2 * K = {2 * K} floats, and even"
    s = _seg(y_stride=K - 1)
    assert lib.bhw_stft_mfft_f32_device(ref, 400, 0, None, ctypes.byref(s), DETREND | POWER, None, ctypes.c_void_p(X), ctypes.c_void_p(P)) == BADARG
    assert _err() == f"y_stride {K - 1}: at least W = {K} floats"
    assert lib.bhw_describe_stft_mfft(None, ref, 400, ctypes.byref(_seg(n_fft=512)), DETREND, None, buf, 1280) == UNSUPPORTED
    assert _err() == "n_fft 512 is a power of two: bhw_stft_fft_f32_* and bhw_spectrogram_f32_* transform it (one transform per n_fft)"
    assert lib.bhw_describe_stft_mfft(None, ref, 400, ctypes.byref(_seg(n_fft=448)), DETREND, None, buf, 1280) == UNSUPPORTED
    assert _err() == "n_fft 448: the mixed-radix fused FFT takes an even 2^a 3^b 5^c in 16..4095"
    # the power-of-two Welch calls refuse these sizes with their own words, as before
    s5 = B.make_stft(4, 16000, 97, 160, 500, shift=31)
    assert lib.bhw_describe_welch_fft(None, ref, 400, ctypes.byref(s5), DETREND, buf, 1280) == UNSUPPORTED
    assert _err() == "n_fft 500: the fused FFT takes a power of two in 16..4096"
    s5.channels = 2
    assert lib.bhw_describe_welch_cfft(None, ref, 400, ctypes.byref(s5), DETREND, buf, 1280) == UNSUPPORTED
    assert _err() == "n_fft 500: the fused complex FFT takes a power of two in 16..2048"
    d = B.make_psd(2, 300, K, 400, 1.0, onesided=True)
    assert lib.bhw_welch_psd_f32(0, None, ctypes.byref(d), ctypes.c_void_p(X), ctypes.c_void_p(P), ctypes.c_void_p(W), 8) == WORKSPACE
    assert _err() == f"workspace of 8 bytes, the block sums need {2 * 2 * K * 8}"
    # the forward line is as it was
    line = B.describe_stft_mfft(p, 400, _seg(batch=64, samples=160000, frames=998), detrend=True)
    assert line == ("stft mfft direct (L = 400, n_fft 400, col0 0, pad 0 constant, constant detrend), spectrum rows, K = 201: "
                    "k_stft_mfft_direct<2>, 64 signals x 998 frames = 63872 rows, complex FFT of 200 points in passes 5x5x4x2 + split, 64 lanes "
                    "per row x 4 rows per workgroup, 7 columns per lane, 15968 groups, grid 2048 x 256 lanes, 14416 bytes of LDS")


def test_there_is_no_new_fft_value():
    from blackman_harris_win_amd import selector
    p = B.make_params(B.WIN_HANN, 10, 16)
    for value in ("mixed", "fused_mixed", "mfft"):
        with pytest.raises(ValueError, match="'torch' or 'fused'"):
            selector._fft_check(value)
        with pytest.raises(ValueError, match="fft must be 'torch' or 'fused'"):
            selector._welch(None, p, None, 1.0, 48, None, None, "constant", True, "density", None, "mean", 0, None, {}, value)
    assert "fft" not in inspect.signature(bhw.welch_fused_mixed).parameters and "fft" not in inspect.signature(bhw.welch_fft_mixed).parameters


def test_python_surface():
    for name in ("welch_fft_mixed", "welch_fused_mixed", "describe_welch_mfft", "welch_mfft_workspace_bytes"):
        assert name in bhw.__all__ and hasattr(bhw, name)
    assert B.describe_welch_mfft is bhw.describe_welch_mfft and B.welch_mfft_workspace_bytes is bhw.welch_mfft_workspace_bytes
    # the arguments are welch_fft's and welch_fused's
    for mixed, pow2 in ((bhw.welch_fft_mixed, bhw.welch_fft), (bhw.welch_fused_mixed, bhw.welch_fused)):
        sig, ref = inspect.signature(mixed), inspect.signature(pow2)
        assert list(sig.parameters) == list(ref.parameters)
        assert all(sig.parameters[n].default == ref.parameters[n].default and sig.parameters[n].kind == ref.parameters[n].kind
                   for n in sig.parameters)
        assert list(inspect.signature(getattr(bhw.ResidentTable, mixed.__name__)).parameters)[1:] == list(sig.parameters)
    sig = inspect.signature(bhw.welch_fft_mixed)
    assert sig.parameters["center"].default is False and "fbank" not in sig.parameters
    assert "return_onesided" not in inspect.signature(bhw.welch_fused_mixed).parameters
    # the refusals name the call that takes what this one does not (raised on the GPU: tests/test_gpu_welch_mixed.py)
    src = inspect.getsource(__import__("blackman_harris_win_amd.selector", fromlist=["x"])._welch_mfft_input)
    assert "welch_fft / welch_fused" in src and "welch_fft_iq" in src
    assert "welch_fft" in bhw.welch_fft_mixed.__doc__ and "welch_fft_iq" in bhw.welch_fft_mixed.__doc__
    # the existing fronts keep their signatures
    assert list(inspect.signature(bhw.welch).parameters) == ["params", "x", "fs", "length", "noverlap", "nfft", "detrend", "return_onesided",
                                                             "scaling", "shift", "average", "fft"]
    assert list(inspect.signature(bhw.welch_fft).parameters) == ["params", "x", "n_fft", "hop", "scale", "win_length", "center", "pad_mode",
                                                                 "detrend", "onesided_doubling", "shift", "out", "workspace"]
    assert list(inspect.signature(bhw.stft_mixed).parameters) == ["params", "x", "n_fft", "hop", "win_length", "center", "pad_mode", "detrend",
                                                                  "shift", "out"]
