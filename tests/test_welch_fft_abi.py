"""The fused Welch PSD calls (bhw_welch_fft_f32_device / _from_table / bhw_welch_fft_workspace_bytes / bhw_describe_welch_fft): the
checks that need no GPU -- exports and declarations, every refusal of include/bhw.h with its code before any HIP call, the workspace
formula, frames 0, the describe line, the messages of the existing families, and the Python surface."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import welch_fft_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
NEW_SYMBOLS = ("bhw_welch_fft_workspace_bytes", "bhw_welch_fft_f32_device", "bhw_welch_fft_f32_from_table", "bhw_describe_welch_fft")
# never dereferenced: every call below fails or has nothing to do
X, P, W = 0x10000000, 0x80000000, 0x40000000
K = 257


def _err():
    return B.lib().bhw_last_error().decode()


def _seg(**kw):
    """Welch framing: 4 signals of 16000, window 400 in rows of 512, hop 160, no padding: 98 frames, 7 chunks, one block."""
    a = dict(batch=4, samples=16000, frames=98, hop=160, n_fft=512, shift=31)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _need(s):
    return 8 * WC.workspace_doubles(s.batch, s.frames, s.n_fft // 2 + 1)


def _calls(s, flags=1, L=400, scale=1.0, psd_flags=1, x=X, out=P, p_stride=0, ws=W, ws_bytes=None):
    lib = B.lib()
    sr = ctypes.byref(s) if s is not None else None
    nbytes = (_need(s) if s is not None else 0) if ws_bytes is None else ws_bytes
    tail = (sr, flags, scale, psd_flags, ctypes.c_void_p(x), ctypes.c_void_p(out), p_stride, ctypes.c_void_p(ws), nbytes)
    return (lambda p: lib.bhw_welch_fft_f32_device(p, L, 0, None, *tail),
            lambda p: lib.bhw_welch_fft_f32_from_table(None, p, L, None, *tail))


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
    assert re.search(r"#define BHW_WELCH_FFT_CHUNK 16u", header) and B.WELCH_FFT_CHUNK == 16 and B.WELCH_BLOCK == 256
    # the reason for 16 stands next to the constant, and the consequences of the order are stated
    at = header.index("#define BHW_WELCH_FFT_CHUNK")
    assert "1 024 independent chunk chains" in header[at - 600:at]
    for words in ("not on B, the grid", "bit for bit", "at most one float32 ulp", "no float atomics", "Not built"):
        assert words in header, words
    # bhw_stft and bhw_psd are as they were
    assert ctypes.sizeof(B.BhwStft) == 96 and ctypes.sizeof(B.BhwPsd) == 72


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
    buf = ctypes.create_string_buffer(1280)
    for flags in (0, 1):
        for kw, code, text in cases:
            s = _seg(**{k: v for k, v in kw.items() if k != "struct_size"})
            if "struct_size" in kw:
                s.struct_size = kw["struct_size"]
            for call in _calls(s, flags=flags):
                assert call(ref) == code and text in _err(), (flags, kw, _err())
            # the same code and the same words as the forward call
            want = _err()
            assert B.lib().bhw_describe_stft_fft(None, ref, 400, ctypes.byref(s), flags, buf, 1280) == code and _err() == want, (kw, want, _err())
        assert _passes(ref, _seg(), flags=flags)
    for kw, text in ((dict(pad=256), "pad 256"), (dict(col0=56), "col0 56"), (dict(pad_mode=B.PAD_REFLECT), "pad_mode 1")):
        for call in _calls(_seg(**kw), flags=1):
            assert call(ref) == BADARG and text in _err(), (kw, _err())
    # the padding fields as the forward call accepts them: a centred, reflect-padded descriptor
    assert _passes(ref, _seg(pad=256, col0=56, pad_mode=B.PAD_REFLECT, frames=101), flags=0)
    for call in _calls(_seg(pad=256, col0=56, pad_mode=B.PAD_REFLECT, frames=102), flags=0):
        assert call(ref) == BADARG and "leaves the padded signal" in _err()
    for call in _calls(_seg(), flags=2):
        assert call(ref) == BADARG and "flags" in _err()
    for call in _calls(None):
        assert call(ref) == BADARG and "descriptor is NULL" in _err()
    for call in _calls(_seg()):
        assert call(None) == BADARG
    for call in _calls(_seg(), L=0):
        assert call(ref) == BADARG and "length" in _err()
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    for call in _calls(_seg()):
        assert call(ctypes.byref(taylor)) == UNSUPPORTED


def test_output_side_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    s = _seg()
    # no spectrum is written: non-zero y strides are refused, whatever their value
    for kw in (dict(y_stride=2 * K), dict(y_batch_stride=98 * 2 * K), dict(y_stride=2 * K + 2, y_batch_stride=98 * (2 * K + 2)), dict(y_stride=3)):
        for call in _calls(_seg(**kw)):
            assert call(ref) == BADARG and "no spectrum is written" in _err(), (kw, _err())
    for call in _calls(s, psd_flags=2):
        assert call(ref) == BADARG and "psd_flags" in _err()
    for scale in (float("inf"), float("-inf"), float("nan")):
        for call in _calls(s, scale=scale):
            assert call(ref) == BADARG and "scale is not finite" in _err()
    for scale, fl in ((0.0, 0), (-1.5, 1), (1e300, 0)):
        assert _passes(ref, s, scale=scale, psd_flags=fl)
    for call in _calls(s, p_stride=K - 1):
        assert call(ref) == BADARG and "p_stride" in _err()
    assert _passes(ref, s, p_stride=K) and _passes(ref, s, p_stride=K + 7)
    # The stated limit, batch * ceil(frames / 16) * K above 2^34, cannot be the first to refuse: ceil(F / 16) <= F, and the forward
    # checks, which run first, hold batch * frames * n_fft (and batch * frames * K) to 2^34.  What is matched here is THEIR message;
    # the branch of bhwp_welch_fft_checks behind them is not reached by any descriptor.
    big = (1 << 34) // (98 * K) + 1
    for call in _calls(_seg(batch=big), ws_bytes=1 << 60):
        assert call(ref) == BADARG and _err() == "batch * frames * n_fft above 2^34 per call", _err()
    for kw in (dict(x=0), dict(out=0)):
        for call in _calls(s, **kw):
            assert call(ref) == BADARG and "NULL" in _err()
    for call in _calls(s, out=P + 2):
        assert call(ref) == BADARG and "d_P is not 4-byte aligned" in _err()
    assert _passes(ref, s, out=P + 4)
    for call in _calls(s, x=X + 2):
        assert call(ref) == BADARG and "d_x is not 4-byte aligned" in _err()
    # the workspace: NULL, misaligned, short (its own code), and exactly enough
    for call in _calls(s, ws=0):
        assert call(ref) == BADARG and "workspace is NULL" in _err()
    for call in _calls(s, ws=W + 4):
        assert call(ref) == BADARG and "workspace is not 8-byte aligned" in _err()
    for call in _calls(s, ws_bytes=_need(s) - 1):
        assert call(ref) == WORKSPACE and "workspace of" in _err()
    for call in _calls(s, ws_bytes=0):
        assert call(ref) == WORKSPACE
    assert _passes(ref, s, ws_bytes=_need(s)) and _passes(ref, s, ws_bytes=_need(s) + 8)
    # overlaps: x holds 4 * 16000 floats, P 4 * 257 floats, the workspace _need(s) bytes
    xb, pb, wb = 4 * 16000 * 4, 4 * K * 4, _need(s)
    for kw, bad, text in (
            (dict(x=X, out=X + xb - 4), True, "d_x and d_P overlap"), (dict(x=X, out=X + xb), False, ""),
            (dict(x=P + pb - 4, out=P), True, "d_x and d_P overlap"), (dict(x=P + pb, out=P), False, ""),
            (dict(x=X, ws=X + xb - 8), True, "workspace overlaps"), (dict(x=X, ws=X + xb), False, ""),
            (dict(x=W + wb - 4, ws=W), True, "workspace overlaps"), (dict(x=W + wb, ws=W), False, ""),
            (dict(out=P, ws=P + pb - 4 - (pb - 4) % 8), True, "workspace overlaps"), (dict(out=W + wb - 4, ws=W), True, "workspace overlaps"),
            (dict(out=W + wb, ws=W), False, "")):
        if bad:
            for call in _calls(s, **kw):
                assert call(ref) == BADARG and text in _err(), (kw, _err())
        else:
            assert _passes(ref, s, **kw), (kw, _err())


@pytest.mark.parametrize("cid", WC.case_ids())
def test_workspace_bytes_equal_the_formula(cid):
    c = WC.case(cid)
    s, _, F, _ = WC.desc(c)
    Kc = c["n_fft"] // 2 + 1
    chunks, blocks = -(-F // 16), -(-F // 256)
    want = 8 * c["B"] * Kc * (chunks + (blocks if blocks > 1 else 0))
    assert B.welch_fft_workspace_bytes(s) == want == WC.parse(WC.line(c))["workspace"]
    p = WC.params(c["setup"])
    assert _passes(ctypes.byref(p), s, L=c["L"], flags=int(c["detrend"]), ws_bytes=want), _err()
    for call in _calls(s, L=c["L"], flags=int(c["detrend"]), ws_bytes=want - 8):
        assert call(ctypes.byref(p)) == WORKSPACE, _err()


def test_workspace_bytes_of_nothing():
    assert B.lib().bhw_welch_fft_workspace_bytes(None) == 0
    assert B.welch_fft_workspace_bytes(_seg(frames=0)) == 0
    s = _seg()
    s.struct_size = 80
    assert B.welch_fft_workspace_bytes(s) == 0


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1280)
    for n in list(range(1, 300)) + [400, 500, 511, 512, 513, 1024, 2048, 3000, 4096, 4097, 8192]:
        s = B.make_stft(2, 100000, 3, 7, n, shift=31)
        rc = lib.bhw_describe_welch_fft(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), 1, buf, 1280)
        assert rc == (OK if B.fft_supported(n) else UNSUPPORTED), (n, rc, _err())


def test_frames_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    for flags in (0, 1):
        s = _seg(frames=0)
        assert lib.bhw_welch_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, 1, None, None, 0, None, 0) == OK
        assert lib.bhw_welch_fft_f32_from_table(None, ctypes.byref(p), 400, None, ctypes.byref(s), flags, 1.0, 1, None, None, 0, None, 0) == BADARG
        assert "table is NULL" in _err()
        assert "nothing (frames 0)" in B.describe_welch_fft(p, 400, s, detrend=bool(flags))
        # what is checked before frames 0 returns: the descriptor, the strides, the flags, the scale
        assert lib.bhw_welch_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, float("nan"), 1, None, None, 0, None, 0) == BADARG
        assert lib.bhw_welch_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, 4, None, None, 0, None, 0) == BADARG
        s = _seg(frames=0, n_fft=768)
        assert lib.bhw_welch_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, 1, None, None, 0, None, 0) == UNSUPPORTED


def test_describe_line_parses():
    p = B.make_params(B.WIN_BH7, 16, 32)
    s = _seg(batch=64, samples=160000, frames=998)
    d = WC.parse(B.describe_welch_fft(p, 400, s, detrend=True))
    assert d["line"].startswith("welch fft direct (L = 400, n_fft 512, col0 0, pad 0 constant, constant detrend): k_welch_fft_direct<2>")
    assert (d["signals"], d["frames"], d["rows"], d["m"], d["schedule"]) == (64, 998, 63872, 256, "4x4x4x4")
    assert (d["lpf"], d["fy"], d["cpl"], d["lds"]) == (64, 4, 8, 2 * 4 * 256 * 8 + 256 * 8 + 16)
    # 998 frames pad to 1008 = 63 runs of 16 frames per signal, four groups each
    assert (d["chunk"], d["run"], d["gpr"], d["runs"], d["groups"], d["grid"]) == (16, 16, 4, 64 * 63, 64 * 63 * 4, 2048)
    assert (d["acc"], d["chunks"], d["blocks"], d["joins"], d["workspace"]) == (2, 63, 4, 2, 8 * 64 * 257 * (63 + 4))
    # one signal of 2^24 samples at 4096 / hop 1024: 1 024 chunk chains
    t2 = WC.parse(B.describe_welch_fft(p, 4096, B.make_stft(1, 1 << 24, 16381, 1024, 4096, shift=31), detrend=True))
    assert (t2["runs"], t2["chunks"], t2["blocks"], t2["acc"], t2["gpr"], t2["grid"]) == (1024, 1024, 64, 9, 16, 1024)
    with pytest.raises(B.BhwError):
        B.describe_welch_fft(p, 400, _seg(n_fft=500))
    buf = ctypes.create_string_buffer(16)
    assert B.lib().bhw_describe_welch_fft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, buf, 16) == OK and len(buf.value) == 15
    assert B.lib().bhw_describe_welch_fft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, None, 0) == BADARG


def test_the_existing_families_keep_their_messages():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1280)
    s = _seg(y_stride=2 * K + 1)
    assert lib.bhw_stft_fft_f32_device(ref, 400, 0, None, ctypes.byref(s), 1, ctypes.c_void_p(X), ctypes.c_void_p(P)) == BADARG
    assert _err() == f"y_stride {2 * K + 1}: at least 2 * K = {2 * K} floats, and even"
    s = _seg(y_stride=K - 1)
    assert lib.bhw_spectrogram_f32_device(ref, 400, 0, None, ctypes.byref(s), 1, None, ctypes.c_void_p(X), ctypes.c_void_p(P)) == BADARG
    assert _err() == f"y_stride {K - 1}: at least W = {K} floats"
    assert lib.bhw_describe_stft_fft(None, ref, 400, ctypes.byref(_seg(n_fft=500)), 1, buf, 1280) == UNSUPPORTED
    assert _err() == "n_fft 500: the fused FFT takes a power of two in 16..4096"
    d = B.make_psd(2, 300, K, 512, 1.0, onesided=True)
    assert lib.bhw_welch_psd_f32(0, None, ctypes.byref(d), ctypes.c_void_p(X), ctypes.c_void_p(P), ctypes.c_void_p(W), 8) == WORKSPACE
    assert _err() == f"workspace of 8 bytes, the block sums need {2 * 2 * K * 8}"
    d.scale = float("inf")
    assert lib.bhw_welch_psd_f32(0, None, ctypes.byref(d), ctypes.c_void_p(X), ctypes.c_void_p(P), ctypes.c_void_p(W), 1 << 20) == BADARG
    assert _err() == "scale is not finite"
    # the forward line is as it was
    line = B.describe_stft_fft(p, 400, _seg(batch=64, samples=160000, frames=998), detrend=True)
    assert line == ("stft fft direct (L = 400, n_fft 512, col0 0, pad 0 constant, constant detrend): k_stft_fft_direct<2>, 64 signals x 998 "
                    "frames = 63872 rows, complex FFT of 256 points in passes 4x4x4x4 + split, 64 lanes per row x 4 rows per workgroup, 8 "
                    "columns per lane, 15968 groups, grid 2048 x 256 lanes, 18448 bytes of LDS")


def test_there_is_no_new_fft_value():
    from blackman_harris_win_amd import selector
    p = B.make_params(B.WIN_HANN, 10, 16)
    with pytest.raises(ValueError, match="'torch' or 'fused'"):
        selector._fft_check("accumulate")
    # bhw.welch(..., fft="accumulate") past its device gate: the first thing _welch does
    with pytest.raises(ValueError, match="fft must be 'torch' or 'fused', got 'accumulate'"):
        selector._welch(None, p, None, 1.0, 64, None, None, "constant", True, "density", None, "mean", 0, None, {}, "accumulate")
    assert "fft" not in inspect.signature(bhw.welch_fused).parameters and "fft" not in inspect.signature(bhw.welch_fft).parameters


def test_python_surface():
    for name in ("welch_fft", "welch_fused", "describe_welch_fft", "welch_fft_workspace_bytes", "WELCH_FFT_CHUNK"):
        assert name in bhw.__all__ and hasattr(bhw, name)
    assert B.describe_welch_fft is bhw.describe_welch_fft and B.WELCH_FFT_CHUNK == bhw.WELCH_FFT_CHUNK == 16
    sig = inspect.signature(bhw.welch_fft)
    assert list(sig.parameters) == ["params", "x", "n_fft", "hop", "scale", "win_length", "center", "pad_mode", "detrend", "onesided_doubling",
                                    "shift", "out", "workspace"]
    assert sig.parameters["center"].default is False and sig.parameters["pad_mode"].default == "reflect"
    assert sig.parameters["detrend"].default is False and sig.parameters["onesided_doubling"].default is True
    assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for n, q in sig.parameters.items() if n not in ("params", "x", "n_fft", "hop", "scale"))
    assert list(inspect.signature(bhw.ResidentTable.welch_fft).parameters)[1:] == list(sig.parameters)
    sig = inspect.signature(bhw.welch_fused)
    assert list(sig.parameters) == ["params", "x", "fs", "length", "noverlap", "nfft", "detrend", "scaling", "shift", "out", "workspace"]
    assert sig.parameters["fs"].default == 1.0 and sig.parameters["detrend"].default == "constant" and sig.parameters["scaling"].default == "density"
    assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for n, q in sig.parameters.items() if n not in ("params", "x", "fs"))
    assert list(inspect.signature(bhw.ResidentTable.welch_fused).parameters)[1:] == list(sig.parameters)
    # the two-sided estimate and other averages are welch()'s, and the documents say so
    assert "return_onesided" not in sig.parameters and "average" not in sig.parameters
    assert "return_onesided=False" in bhw.welch_fused.__doc__ and "mean" in bhw.welch_fused.__doc__
    # the existing fronts keep their signatures
    assert list(inspect.signature(bhw.welch).parameters) == ["params", "x", "fs", "length", "noverlap", "nfft", "detrend", "return_onesided",
                                                             "scaling", "shift", "average", "fft"]
    assert list(inspect.signature(bhw.stft).parameters) == ["params", "x", "n_fft", "hop", "win_length", "center", "pad_mode", "detrend", "shift", "out"]
