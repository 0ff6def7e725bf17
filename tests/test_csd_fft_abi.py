"""The fused Welch cross-spectra calls (bhw_csd_fft_f32_device / _from_table / bhw_csd_fft_workspace_bytes / bhw_describe_csd_fft): the
checks that need no GPU -- exports and declarations, every refusal of include/bhw.h with its code before any HIP call, the workspace
formula, frames 0, the describe line, the messages of the existing families, and the Python surface."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import csd_fft_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
NEW_SYMBOLS = ("bhw_csd_fft_workspace_bytes", "bhw_csd_fft_f32_device", "bhw_csd_fft_f32_from_table", "bhw_describe_csd_fft")
NAMES = tuple(B.CSD_OUTPUTS)                     # pxy, pxx, pyy, coherence, h1: the order of the pointers
WIDTH = dict(pxy=8, pxx=4, pyy=4, coherence=4, h1=8)
# never dereferenced: every call below fails or has nothing to do
X, Y, W = 0x10000000, 0x20000000, 0x40000000
OUT = {n: 0x80000000 + i * 0x1000000 for i, n in enumerate(NAMES)}
K = 257
FULL = B.csd_mask(NAMES) | B.CSD_ONESIDED


def _err():
    return B.lib().bhw_last_error().decode()


def _seg(**kw):
    """Welch framing: 4 signals of 16000, window 400 in rows of 512, hop 160, no padding: 98 frames, 7 chunks, one block."""
    a = dict(batch=4, samples=16000, frames=98, hop=160, n_fft=512, shift=31)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _need(s):
    return 8 * CC.workspace_doubles(s.batch, s.frames, s.n_fft // 2 + 1)


def _calls(s, flags=1, L=400, scale=1.0, csd_flags=FULL, x=X, y=Y, outs=None, o_stride=0, ws=W, ws_bytes=None):
    lib = B.lib()
    sr = ctypes.byref(s) if s is not None else None
    nbytes = (_need(s) if s is not None else 0) if ws_bytes is None else ws_bytes
    o = dict(OUT)
    o.update(outs or {})
    tail = (sr, flags, scale, csd_flags, ctypes.c_void_p(x), ctypes.c_void_p(y), *[ctypes.c_void_p(o[n]) for n in NAMES], o_stride,
            ctypes.c_void_p(ws), nbytes)
    return (lambda p: lib.bhw_csd_fft_f32_device(p, L, 0, None, *tail),
            lambda p: lib.bhw_csd_fft_f32_from_table(None, p, L, None, *tail))


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
    at = header.index("Fused Welch cross spectra")
    text = header[at:header.index("uint64_t bhw_csd_fft_workspace_bytes")]
    for words in ("not on B, the grid", "P_xx is bit for bit bhw_welch_fft_f32_*", "For\n *     F <= 16 every output equals", "Cauchy-Schwarz",
                  "2 F * 2^-53", "4 * bhw_welch_fft_workspace_bytes(s)", "no float atomics", "16..2048", "bhw_stft_fft_f32_* + bhw_welch_csd_f32",
                  "bhw_stft_mfft_f32_*", "bhw_stft_cfft_f32_*", "Not built", "d_x and d_y may coincide"):
        assert words in text, words
    # bhw_stft and bhw_csd are as they were
    assert ctypes.sizeof(B.BhwStft) == 96 and ctypes.sizeof(B.BhwCsd) == 96


def test_input_side_errors_are_the_welch_calls():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    cases = [
        (dict(struct_size=8), BADARG, "struct_size"),
        (dict(channels=3), BADARG, "channels"),
        (dict(batch=0), BADARG, "batch is 0"),
        (dict(hop=0), BADARG, "hop is 0"),
        (dict(n_fft=0), BADARG, "n_fft"),
        (dict(n_fft=256), BADARG, "col0 + L"),
        (dict(shift=63), BADARG, "shift"),
        (dict(frames=99), BADARG, "segment 98 leaves the signal"),
        (dict(samples=0), BADARG, "samples is 0"),
        (dict(x_stride=15999), BADARG, "x_stride"),
    ]
    buf = ctypes.create_string_buffer(1600)
    for flags in (0, 1):
        for kw, code, text in cases:
            s = _seg(**{k: v for k, v in kw.items() if k != "struct_size"})
            if "struct_size" in kw:
                s.struct_size = kw["struct_size"]
            for call in _calls(s, flags=flags):
                assert call(ref) == code and text in _err(), (flags, kw, _err())
            # the same code and the same words as the fused Welch PSD call
            want = _err()
            assert B.lib().bhw_describe_welch_fft(None, ref, 400, ctypes.byref(s), flags, buf, 1600) == code and _err() == want, (kw, want, _err())
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


def test_refusals_of_the_params_keep_their_code_and_words():
    """What the params alone are refused for (the Taylor source, a bit-model without a float32 form, a length the window cannot
    have) is refused before the descriptor is looked at, with the code and the words of bhw_describe_welch_fft -- whatever the
    descriptor holds, a NULL one and the ones this call would rename included."""
    lib = B.lib()
    buf = ctypes.create_string_buffer(1600)
    refused = [(B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR), 400), (B.make_params(B.WIN_BH4, 12, 24, model=B.MODEL_DDS48), 400),
               (B.make_params(B.WIN_BH4, 24, 32), 0), (B.make_params(B.WIN_BH4, 8, 32), 400)]
    seen = set()
    for p, L in refused:
        ref = ctypes.byref(p)
        for s in (_seg(), _seg(n_fft=4096), _seg(n_fft=500), _seg(channels=2), _seg(n_fft=8192), _seg(frames=0), None):
            sr = ctypes.byref(s) if s is not None else None
            code = lib.bhw_describe_welch_fft(None, ref, L, ctypes.byref(_seg()), 1, buf, 1600)
            want = _err()
            assert code in (BADARG, UNSUPPORTED) and "descriptor" not in want and "n_fft" not in want and "channels" not in want, (code, want)
            seen.add(code)
            for call in _calls(s, L=L):
                assert call(ref) == code and _err() == want, (L, want, _err())
            assert lib.bhw_describe_csd_fft(None, ref, L, sr, 1, FULL, buf, 1600) == code and _err() == want, (L, want, _err())
    assert UNSUPPORTED in seen
    # and with params the call takes, a NULL descriptor is the forward call's refusal
    ok = B.make_params(B.WIN_BH4, 24, 32)
    assert lib.bhw_describe_csd_fft(None, ctypes.byref(ok), 400, None, 1, FULL, buf, 1600) == BADARG and _err() == "stft descriptor is NULL"


def test_what_this_call_refuses_is_refused_by_name():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    for call in _calls(_seg(n_fft=4096)):
        assert call(ref) == UNSUPPORTED and "n_fft 4096" in _err() and "16..2048" in _err() and "bhw_stft_fft_f32_* + bhw_welch_csd_f32" in _err(), _err()
    for n in (500, 1000, 480):
        for call in _calls(_seg(n_fft=n)):
            assert call(ref) == UNSUPPORTED and f"n_fft {n}" in _err() and "bhw_stft_mfft_f32_* + bhw_welch_csd_f32" in _err(), _err()
    for call in _calls(_seg(channels=2)):
        assert call(ref) == UNSUPPORTED and "real input" in _err() and "bhw_stft_cfft_f32_* + bhw_welch_csd_f32" in _err(), _err()
    for n in (8192, 514):                               # no call transforms these: nothing to name
        for call in _calls(_seg(n_fft=n)):
            assert call(ref) == UNSUPPORTED and "power of two in 16..2048" in _err() and "; " not in _err() and "bhw_" not in _err(), _err()
    assert _passes(ref, _seg(n_fft=2048, samples=160000)) and _passes(ref, _seg(n_fft=1024))


def test_output_side_errors_before_any_hip_call():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    s = _seg()
    # no spectrum is written: non-zero y strides are refused, with the fused Welch PSD's words
    for kw in (dict(y_stride=2 * K), dict(y_batch_stride=98 * 2 * K), dict(y_stride=3)):
        for call in _calls(_seg(**kw)):
            assert call(ref) == BADARG and "no spectrum is written, both must be 0" in _err(), (kw, _err())
    # the mask: bhw_welch_csd_f32's rules and words
    for call in _calls(s, csd_flags=FULL | 4):
        assert call(ref) == BADARG and _err() == f"flags 0x{FULL | 4:x} (BHW_CSD_ONESIDED, BHW_CSD_BROADCAST_X and the output mask 0x1f0)"
    for call in _calls(s, csd_flags=B.CSD_ONESIDED):
        assert call(ref) == BADARG and _err() == "flags 0x1: the output mask is empty"
    for scale in (float("inf"), float("-inf"), float("nan")):
        for call in _calls(s, scale=scale):
            assert call(ref) == BADARG and _err() == "scale is not finite"
    for scale in (0.0, -1.5, 1e300):
        assert _passes(ref, s, scale=scale)
    for call in _calls(s, o_stride=K - 1):
        assert call(ref) == BADARG and _err() == f"o_stride {K - 1} < bins {K}: rows overlap"
    assert _passes(ref, s, o_stride=K) and _passes(ref, s, o_stride=K + 7)
    for kw in (dict(x=0), dict(y=0)):
        for call in _calls(s, **kw):
            assert call(ref) == BADARG and "d_x / d_y is NULL" in _err()
    for kw in (dict(x=X + 2), dict(y=Y + 1)):
        for call in _calls(s, **kw):
            assert call(ref) == BADARG and "d_x / d_y is not 4-byte aligned" in _err()
    assert _passes(ref, s, x=X + 4) and _passes(ref, s, x=Y, y=Y)                    # 4-byte aligned; x and y may coincide
    # any non-empty subset; a pointer is read only where its bit is set
    for i, n in enumerate(NAMES):
        one = B.csd_mask((n,))
        nothing = {m: 0 for m in NAMES if m != n}
        assert _passes(ref, s, csd_flags=one, outs=nothing), (n, _err())
        for call in _calls(s, csd_flags=one, outs={n: 0}):
            assert call(ref) == BADARG and _err() == f"d_{'Cxy' if n == 'coherence' else n.capitalize() if n != 'h1' else 'H1'} is NULL and its output is requested", _err()
        for call in _calls(s, csd_flags=one, outs={n: OUT[n] + WIDTH[n] // 2}):
            assert call(ref) == BADARG and f"is not {WIDTH[n]}-byte aligned" in _err(), _err()
        assert _passes(ref, s, csd_flags=FULL & ~one, outs={n: 2})                  # not asked for: never looked at
    # the workspace: NULL, misaligned, short (its own code), and exactly enough
    for call in _calls(s, ws=0):
        assert call(ref) == BADARG and "workspace is NULL" in _err()
    for call in _calls(s, ws=W + 4):
        assert call(ref) == BADARG and "workspace is not 8-byte aligned" in _err()
    for call in _calls(s, ws_bytes=_need(s) - 1):
        assert call(ref) == WORKSPACE and "workspace of" in _err()
    for call in _calls(s, ws_bytes=4 * B.welch_fft_workspace_bytes(s) - 8):
        assert call(ref) == WORKSPACE
    assert _need(s) == 4 * B.welch_fft_workspace_bytes(s)
    assert _passes(ref, s, ws_bytes=_need(s)) and _passes(ref, s, ws_bytes=_need(s) + 8)
    # overlaps: x and y hold 4 * 16000 floats, an output 4 * 257 elements, the workspace _need(s) bytes
    xb, wb = 4 * 16000 * 4, _need(s)
    for kw, bad, text in (
            (dict(outs=dict(pxx=X + xb - 4)), True, "d_x and d_Pxx overlap"), (dict(outs=dict(pxx=X + xb)), False, ""),
            (dict(outs=dict(h1=Y + xb - 8)), True, "d_y and d_H1 overlap"), (dict(outs=dict(h1=Y + xb)), False, ""),
            (dict(outs=dict(pyy=OUT["pxx"] + 4 * K * 4 - 4)), True, "d_Pxx and d_Pyy overlap"), (dict(outs=dict(pyy=OUT["pxx"] + 4 * K * 4)), False, ""),
            (dict(ws=X + xb - 8), True, "workspace overlaps d_x"), (dict(ws=X + xb), False, ""),
            (dict(outs=dict(pxy=W + wb - 8)), True, "workspace overlaps d_Pxy"), (dict(outs=dict(pxy=W + wb)), False, "")):
        if bad:
            for call in _calls(s, **kw):
                assert call(ref) == BADARG and text in _err(), (kw, _err())
        else:
            assert _passes(ref, s, **kw), (kw, _err())
    # under broadcast x is one signal: an output right behind its 16000 floats is apart from it
    bc = FULL | B.CSD_BROADCAST_X
    assert _passes(ref, s, csd_flags=bc, outs=dict(pxx=X + 16000 * 4))
    for call in _calls(s, csd_flags=bc, outs=dict(pxx=X + 16000 * 4 - 4)):
        assert call(ref) == BADARG and "d_x and d_Pxx overlap" in _err()
    for call in _calls(s, csd_flags=FULL, outs=dict(pxx=X + 16000 * 4)):
        assert call(ref) == BADARG and "d_x and d_Pxx overlap" in _err()


@pytest.mark.parametrize("cid", CC.case_ids())
def test_workspace_bytes_equal_four_times_the_formula(cid):
    c = CC.case(cid)
    s, _, F, _ = CC.desc(c)
    Kc = c["n_fft"] // 2 + 1
    chunks, blocks = -(-F // 16), -(-F // 256)
    want = 4 * 8 * c["B"] * Kc * (chunks + (blocks if blocks > 1 else 0))
    assert B.csd_fft_workspace_bytes(s) == want == CC.parse(CC.line(c))["workspace"] == 4 * B.welch_fft_workspace_bytes(s)
    p = CC.params(c["setup"])
    cf = FULL | (B.CSD_BROADCAST_X if c.get("bcast") else 0)
    # far apart: the long record's x and y take a megabyte each
    far = dict(x=1 << 32, y=1 << 33, ws=1 << 36, outs={n: (1 << 34) + i * (1 << 30) for i, n in enumerate(NAMES)})
    assert _passes(ctypes.byref(p), s, L=c["L"], flags=int(c["detrend"]), csd_flags=cf, ws_bytes=want, **far), _err()
    for call in _calls(s, L=c["L"], flags=int(c["detrend"]), csd_flags=cf, ws_bytes=want - 8, **far):
        assert call(ctypes.byref(p)) == WORKSPACE, _err()


def test_workspace_bytes_of_nothing():
    assert B.lib().bhw_csd_fft_workspace_bytes(None) == 0
    assert B.csd_fft_workspace_bytes(_seg(frames=0)) == 0
    s = _seg()
    s.struct_size = 80
    assert B.csd_fft_workspace_bytes(s) == 0


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1600)
    for n in list(range(1, 300)) + [400, 500, 511, 512, 513, 1024, 2047, 2048, 2049, 3000, 4096, 4097, 8192]:
        s = B.make_stft(2, 100000, 3, 7, n, shift=31)
        rc = lib.bhw_describe_csd_fft(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), 1, FULL, buf, 1600)
        assert rc == (OK if B.fft_supported(n) and n <= 2048 else UNSUPPORTED), (n, rc, _err())


def test_frames_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    nul = (None,) * 7
    for flags in (0, 1):
        s = _seg(frames=0)
        assert lib.bhw_csd_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, FULL, *nul, 0, None, 0) == OK
        assert lib.bhw_csd_fft_f32_from_table(None, ctypes.byref(p), 400, None, ctypes.byref(s), flags, 1.0, FULL, *nul, 0, None, 0) == BADARG
        assert "table is NULL" in _err()
        assert "nothing (frames 0)" in B.describe_csd_fft(p, 400, s, detrend=bool(flags))
        # what is checked before frames 0 returns: the descriptor, the strides, the flags, the mask, the scale
        assert lib.bhw_csd_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, float("nan"), FULL, *nul, 0, None, 0) == BADARG
        assert lib.bhw_csd_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, 1, *nul, 0, None, 0) == BADARG
        assert lib.bhw_csd_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, FULL | 8, *nul, 0, None, 0) == BADARG
        s = _seg(frames=0, n_fft=768)
        assert lib.bhw_csd_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, 1.0, FULL, *nul, 0, None, 0) == UNSUPPORTED


def test_describe_line_parses():
    p = B.make_params(B.WIN_BH7, 16, 32)
    s = _seg(batch=64, samples=160000, frames=998)
    d = CC.parse(B.describe_csd_fft(p, 400, s, detrend=True, outputs=NAMES))
    assert d["line"].startswith("csd fft direct (L = 400, n_fft 512, col0 0, pad 0 constant, constant detrend): k_csd_fft_direct<2>")
    assert (d["signals"], d["frames"], d["rows"], d["m"], d["schedule"]) == (64, 998, 63872, 256, "4x4x4x4")
    assert (d["lpf"], d["fy"], d["cpl"], d["lds"], d["pairs"]) == (64, 4, 8, 2 * 4 * 256 * 8 + 256 * 8 + 16, 2)
    # 998 frames pad to 1008 = 63 runs of 16 frames per signal, eight groups of two frame pairs each
    assert (d["chunk"], d["run"], d["gpr"], d["runs"], d["groups"], d["grid"]) == (16, 16, 8, 64 * 63, 64 * 63 * 8, 2048)
    assert (d["acc"], d["chains"], d["chunks"], d["blocks"], d["joins"], d["workspace"]) == (2, 4, 63, 4, 2, 4 * 8 * 64 * 257 * (63 + 4))
    assert d["outputs"] == NAMES and d["onesided"] and not d["broadcast"]
    b = CC.parse(B.describe_csd_fft(p, 400, s, outputs=("h1",), onesided=False, broadcast_x=True))
    assert b["outputs"] == ("h1",) and not b["onesided"] and b["broadcast"] and b["chains"] == 4
    # one signal of 2^24 samples at 2048 / hop 512: 2 048 chunk chains, the most accumulators
    t2 = CC.parse(B.describe_csd_fft(p, 2048, B.make_stft(1, 1 << 24, 32765, 512, 2048, shift=31), detrend=True))
    assert (t2["runs"], t2["chunks"], t2["blocks"], t2["acc"], t2["gpr"], t2["grid"], t2["lpf"], t2["lds"]) == (2048, 2048, 128, 5, 16, 2048, 128, 40968)
    with pytest.raises(B.BhwError):
        B.describe_csd_fft(p, 400, _seg(n_fft=500))
    buf = ctypes.create_string_buffer(16)
    assert B.lib().bhw_describe_csd_fft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, FULL, buf, 16) == OK and len(buf.value) == 15
    assert B.lib().bhw_describe_csd_fft(None, ctypes.byref(p), 400, ctypes.byref(s), 0, FULL, None, 0) == BADARG


def test_the_existing_families_keep_their_messages():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1280)
    assert lib.bhw_describe_stft_fft(None, ref, 400, ctypes.byref(_seg(n_fft=500)), 1, buf, 1280) == UNSUPPORTED
    assert _err() == "n_fft 500: the fused FFT takes a power of two in 16..4096"
    assert lib.bhw_describe_welch_fft(None, ref, 400, ctypes.byref(_seg(channels=2)), 1, buf, 1280) == UNSUPPORTED
    assert _err() == "channels 2: the fused FFT takes real input (1)"
    assert lib.bhw_describe_welch_fft(None, ref, 400, ctypes.byref(_seg(n_fft=4096, samples=160000)), 1, buf, 1280) == OK
    s = _seg()
    tail = (ctypes.byref(s), 1, 1.0, 1, ctypes.c_void_p(X), ctypes.c_void_p(OUT["pxx"]), 0, ctypes.c_void_p(W), 8)
    assert lib.bhw_welch_fft_f32_device(ref, 400, 0, None, *tail) == WORKSPACE
    assert _err() == f"workspace of 8 bytes, the chunk and block sums need {8 * 4 * K * 7}"
    # bhw_welch_csd_f32: the mask, pointer, alignment, workspace and overlap words are as they were
    d = B.make_csd(2, 300, K, 512, 1.0, outputs=NAMES, onesided=True)
    args = lambda o=OUT, w=W, wb=1 << 20: (0, None, ctypes.byref(d), ctypes.c_void_p(X), ctypes.c_void_p(Y), *[ctypes.c_void_p(o[n]) for n in NAMES],
                                           ctypes.c_void_p(w), wb)
    assert lib.bhw_welch_csd_f32(*args(wb=8)) == WORKSPACE and _err() == f"workspace of 8 bytes, the block sums need {2 * 2 * K * 4 * 8}"
    assert lib.bhw_welch_csd_f32(*args(o=dict(OUT, pyy=0))) == BADARG and _err() == "d_Pyy is NULL and its output is requested"
    assert lib.bhw_welch_csd_f32(*args(o=dict(OUT, h1=OUT["h1"] + 4))) == BADARG and _err() == "d_H1 is not 8-byte aligned"
    assert lib.bhw_welch_csd_f32(*args(o=dict(OUT, pyy=OUT["pxx"] + 4))) == BADARG and _err() == "d_Pxx and d_Pyy overlap"
    assert lib.bhw_welch_csd_f32(*args(o=dict(OUT, pxy=X + 8))) == BADARG and _err() == "d_X and d_Pxy overlap"
    assert lib.bhw_welch_csd_f32(*args(w=OUT["pxx"])) == BADARG and _err() == "workspace overlaps d_Pxx"
    assert lib.bhw_welch_csd_f32(*args(o=dict(OUT, pxy=(1 << 64) - 8))) == BADARG and _err() == "d_Pxy range wraps the address space"
    d.flags = B.CSD_ONESIDED
    assert lib.bhw_welch_csd_f32(*args()) == BADARG and _err() == "flags 0x1: the output mask is empty"
    # the lines of the neighbouring calls are as they were
    line = B.describe_welch_fft(p, 400, _seg(batch=64, samples=160000, frames=998), detrend=True)
    assert line == ("welch fft direct (L = 400, n_fft 512, col0 0, pad 0 constant, constant detrend): k_welch_fft_direct<2>, 64 signals x 998 "
                    "frames = 63872 rows, complex FFT of 256 points in passes 4x4x4x4 + split, 64 lanes per row x 4 rows per workgroup, 8 "
                    "columns per lane, 16128 groups, grid 2048 x 256 lanes, 18448 bytes of LDS; chunk 16 frames, 4032 runs of 16 frames (4 "
                    "groups per run), 2 accumulators per lane, 63 chunks and 4 blocks per signal, then k_welch_fft_join twice (chunks, "
                    f"blocks), workspace {8 * 64 * 257 * 67} bytes")


def test_there_is_no_new_fft_value():
    from blackman_harris_win_amd import selector
    p = B.make_params(B.WIN_HANN, 10, 16)
    with pytest.raises(ValueError, match="'torch' or 'fused'"):
        selector._fft_check("accumulate")
    # bhw.cross_spectra(..., fft="accumulate") past its device gate: the first thing _cross does
    with pytest.raises(ValueError, match="fft must be 'torch' or 'fused', got 'accumulate'"):
        selector._cross(None, p, None, None, 1.0, 64, None, None, "constant", True, "density", None, ("pxy",), None, {}, "accumulate")
    for f in (bhw.csd_fft, bhw.cross_spectra_fused, bhw.csd_fused, bhw.coherence_fused, bhw.transfer_function_fused):
        assert "fft" not in inspect.signature(f).parameters


def test_python_surface():
    """Each new name exists (on the parent none does)."""
    for name in ("csd_fft", "cross_spectra_fused", "csd_fused", "coherence_fused", "transfer_function_fused", "describe_csd_fft",
                 "csd_fft_workspace_bytes"):
        assert name in bhw.__all__ and hasattr(bhw, name), name
    assert B.describe_csd_fft is bhw.describe_csd_fft and B.csd_fft_workspace_bytes is bhw.csd_fft_workspace_bytes
    for name in ("csd_fft", "cross_spectra_fused", "csd_fused", "coherence_fused", "transfer_function_fused"):
        assert list(inspect.signature(getattr(bhw.ResidentTable, name)).parameters)[1:] == list(inspect.signature(getattr(bhw, name)).parameters), name
    sig = inspect.signature(bhw.csd_fft)
    assert list(sig.parameters) == ["params", "x", "y", "n_fft", "hop", "scale", "outputs", "win_length", "center", "pad_mode", "detrend",
                                    "onesided_doubling", "shift", "out", "workspace"]
    assert sig.parameters["center"].default is False and sig.parameters["pad_mode"].default == "reflect" and sig.parameters["outputs"].default == ("pxy",)
    assert sig.parameters["detrend"].default is False and sig.parameters["onesided_doubling"].default is True
    assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for n, q in sig.parameters.items() if n not in ("params", "x", "y", "n_fft", "hop", "scale"))
    sig = inspect.signature(bhw.cross_spectra_fused)
    assert list(sig.parameters) == ["params", "x", "y", "fs", "length", "noverlap", "nfft", "detrend", "scaling", "shift", "outputs", "out", "workspace"]
    assert sig.parameters["fs"].default == 1.0 and sig.parameters["detrend"].default == "constant" and sig.parameters["scaling"].default == "density"
    assert sig.parameters["outputs"].default == ("pxy", "pxx", "pyy", "coherence", "h1")
    assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for n, q in sig.parameters.items() if n not in ("params", "x", "y", "fs"))
    for f in (bhw.csd_fused, bhw.coherence_fused, bhw.transfer_function_fused):
        assert list(inspect.signature(f).parameters) == ["params", "x", "y", "fs", "length", "noverlap", "nfft", "detrend", "scaling", "shift", "out",
                                                         "workspace"]
    assert "return_onesided" not in sig.parameters and "average" not in sig.parameters and "mean" in bhw.cross_spectra_fused.__doc__
    # the existing fronts keep their signatures
    for f in (bhw.csd, bhw.coherence, bhw.transfer_function):
        assert list(inspect.signature(f).parameters) == ["params", "x", "y", "fs", "length", "noverlap", "nfft", "detrend", "return_onesided",
                                                         "scaling", "shift", "fft"]
    assert list(inspect.signature(bhw.cross_spectra).parameters) == ["params", "x", "y", "fs", "length", "noverlap", "nfft", "detrend",
                                                                     "return_onesided", "scaling", "shift", "outputs", "fft"]
    assert list(inspect.signature(bhw.welch_csd).parameters) == ["X", "Y", "scale", "nfft", "onesided", "outputs", "out", "workspace"]
