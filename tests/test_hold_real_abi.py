"""The fused max-hold / min-hold calls for real input, both families (bhw_hold_fft_f32_* and bhw_hold_mfft_f32_*, their
workspace_bytes and describe calls): the checks that need no GPU -- exports and declarations, the header's words, the two families'
prototypes word for word, every input-side refusal with the code and the exact message of the Welch sibling, the output-side refusals
of include/bhw.h in the stated order and before any HIP call, the workspace figure, frames 0, the describe line, the messages of the
older calls, and the Python surface."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import hold_real_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
FAMILIES = ("fft", "mfft")
NEW_SYMBOLS = tuple(f"bhw_hold_{f}{t}" for f in FAMILIES for t in ("_workspace_bytes", "_f32_device", "_f32_from_table")) + \
    ("bhw_describe_hold_fft", "bhw_describe_hold_mfft")
# never dereferenced: every call below fails or has nothing to do
X, PMAX, PMIN, W = 0x10000000, 0x80000000, 0x90000000, 0x40000000
SIZE = {"fft": 512, "mfft": 400}
DETREND, POWER = 1, 2
ONESIDED = 1
BOTH = 3


def _err():
    return B.lib().bhw_last_error().decode()


def _seg(fam, **kw):
    """Welch framing: 4 signals of 16000 samples, window 400 in rows of 512 / 400, hop 160, no padding: 98 frames, 7 chunks, one
    block (the siblings' ABI tests use this descriptor)."""
    a = dict(batch=4, samples=16000, frames=98, hop=160, n_fft=SIZE[fam], shift=31)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _need(s):
    return 8 * H.WF.workspace_doubles(s.batch, s.frames, s.n_fft // 2 + 1)


def _fn(fam, tail):
    return getattr(B.lib(), f"bhw_hold_{fam}{tail}")


def _calls(fam, s, flags=DETREND, L=400, scale=1.0, psd=ONESIDED, x=X, pmax=PMAX, pmin=PMIN, p_stride=0, ws=W, ws_bytes=None):
    sr = ctypes.byref(s) if s is not None else None
    nbytes = (_need(s) if s is not None else 0) if ws_bytes is None else ws_bytes
    tail = (sr, flags, scale, psd, ctypes.c_void_p(x), ctypes.c_void_p(pmax), ctypes.c_void_p(pmin), p_stride, ctypes.c_void_p(ws), nbytes)
    return (lambda p: _fn(fam, "_f32_device")(p, L, 0, None, *tail),
            lambda p: _fn(fam, "_f32_from_table")(None, p, L, None, *tail))


def _welch_call(fam, s, flags=DETREND, L=400, scale=1.0, psd=ONESIDED):
    """The Welch sibling's device call with good pointers: it stops at 'table is NULL' in the from-table form when every check passes."""
    fn = getattr(B.lib(), f"bhw_welch_{fam}_f32_from_table")
    sr = ctypes.byref(s) if s is not None else None
    return lambda p: fn(None, p, L, None, sr, flags, scale, psd, ctypes.c_void_p(X), ctypes.c_void_p(PMAX), 0, ctypes.c_void_p(W), 1 << 40)


def _passes(fam, ref, s, **kw):
    """Every check passed: the from-table call with no table stops at 'table is NULL', before any launch."""
    rc = _calls(fam, s, **kw)[1](ref)
    return rc == BADARG and "table is NULL" in _err()


def _header():
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        return fh.read()


def test_exports_declarations_and_header_words():
    L = B.lib()
    header = _header()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\b(int|uint64_t) " + name + r"\(", header), name
    # additions only
    assert L.bhw_abi_version() == 4
    assert ctypes.sizeof(B.BhwStft) == 96 and ctypes.sizeof(B.BhwPsd) == 72
    # the new section stands after bhw_describe_hold_cmfft and before the cross spectra
    at = header.index("Fused max-hold and min-hold traces for real input")
    assert header.index("int bhw_describe_hold_cmfft(") < at < header.index("/* Fused Welch cross spectra")
    end = header.index("int bhw_describe_hold_mfft(")
    assert end < header.index("/* Fused Welch cross spectra")
    text = header[at:end]
    for words in ("Either may be NULL", "Both NULL is BHW_ERR_BADARG", "over the live frames f < F only",
                  "fl32((double) max_f h_f * s_k)", "fl32((double) min_f h_f * s_k)", "fl32((double) re * re +", "(double) im * im)",
                  "s_k = scale * 2.0 where", "K = n_fft / 2 + 1", "both traces of that bin are NaN", "unsigned integers", "not on B,",
                  "the order of the reduction", "library versus table", "At EVERY F", "bit for bit", "there is no ulp clause",
                  "no float atomics", "bhw_hold_fft_workspace_bytes(s) = bhw_welch_fft_workspace_bytes(s)",
                  "bhw_hold_mfft_workspace_bytes(s) = bhw_welch_mfft_workspace_bytes(s)", "The layout inside is not part of the contract",
                  "BHW_ERR_WORKSPACE", "with the pointers unchecked", "Both traces are always computed", "the same check function",
                  "Not built: median or percentile traces; the mean in the same launch", "BHW_MFFT_POWER is refused", "the traces asked for"):
        assert words in text, words
    # the older "Not built" sentences stand word for word and once, each followed by a pointer to the new calls
    for old, new in (
            ("Not built: max-hold or median averaging; a filter bank on the averaged powers.", "bhw_hold_fft_f32_* below"),
            ("Not built: odd n_fft and factors >= 7; cross spectra at these lengths in one kernel; max-hold or median traces.",
             "bhw_hold_mfft_f32_* below"),
            ("Not built: median or percentile traces; the mean in the same launch (call bhw_welch_cfft_f32_* beside this one); real input;",
             "bhw_hold_fft_f32_*")):
        i = header.index(old)
        section = header[i:header.index("\n *   - bhw_describe_", i)]
        assert new in section, old
        assert header.count(old) == 1


def test_the_two_families_have_one_prototype():
    header = _header()
    flat = lambda t: re.sub(r"\s+", " ", t)                          # noqa: E731
    for kind, tail in (("int", "_f32_device"), ("int", "_f32_from_table"), ("uint64_t", "_workspace_bytes")):
        a = re.search(kind + r" bhw_hold_fft" + tail + r"\(([^;]*)\);", header).group(1)
        b = re.search(kind + r" bhw_hold_mfft" + tail + r"\(([^;]*)\);", header).group(1)
        assert flat(a) == flat(b), tail
    a = re.search(r"int bhw_describe_hold_fft\(([^;]*)\);", header).group(1)
    assert flat(a) == flat(re.search(r"int bhw_describe_hold_mfft\(([^;]*)\);", header).group(1))
    assert flat(a) == flat(re.search(r"int bhw_describe_hold_cfft\(([^;]*)\);", header).group(1))
    # the issue's prototype, word for word
    want = ("const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags, double scale, "
            "uint32_t psd_flags, const float *d_x, float *d_max, float *d_min, uint64_t p_stride, void *workspace, uint64_t workspace_bytes")
    assert flat(re.search(r"int bhw_hold_fft_f32_device\(([^;]*)\);", header).group(1)) == want
    # the Welch siblings', with the two outputs in d_P's place
    for fam in FAMILIES:
        for tail in ("_f32_device", "_f32_from_table"):
            old = flat(re.search(r"int bhw_welch_" + fam + tail + r"\(([^;]*)\);", header).group(1))
            new = flat(re.search(r"int bhw_hold_" + fam + tail + r"\(([^;]*)\);", header).group(1))
            assert old.replace("float *d_P,", "float *d_max, float *d_min,") == new, (fam, tail)
    L = B.lib()
    for tail in ("_workspace_bytes", "_f32_device", "_f32_from_table"):
        assert _fn("fft", tail).argtypes == _fn("mfft", tail).argtypes and _fn("fft", tail).restype == _fn("mfft", tail).restype
    assert L.bhw_describe_hold_fft.argtypes == L.bhw_describe_hold_mfft.argtypes
    a = list(L.bhw_welch_fft_f32_device.argtypes)
    assert list(L.bhw_hold_fft_f32_device.argtypes) == a[:9] + [a[9]] + a[9:]


# the refusal cases of tests/test_welch_fft_abi.py and tests/test_welch_mfft_abi.py, and the sizes of the other family
_CASES = [dict(struct_size=8), dict(channels=3), dict(channels=2), dict(batch=0), dict(hop=0), dict(n_fft=0), dict(n_fft=256), dict(n_fft=200),
          dict(n_fft=500), dict(n_fft=512), dict(n_fft=400), dict(n_fft=8192), dict(n_fft=4096, frames=50), dict(n_fft=14), dict(n_fft=401),
          dict(n_fft=448), dict(shift=63), dict(frames=99), dict(samples=0), dict(x_stride=15999), dict(pad=256), dict(pad=200), dict(col0=56),
          dict(pad_mode=B.PAD_REFLECT), dict(y_stride=3), dict(y_batch_stride=7), dict(pad=256, col0=56, pad_mode=B.PAD_REFLECT, frames=101),
          dict(pad=256, col0=56, pad_mode=B.PAD_REFLECT, frames=102)]


@pytest.mark.parametrize("fam", FAMILIES)
def test_input_side_refusals_are_the_welch_siblings_word_for_word(fam):
    """Every input-side refusal carries the code and the exact message of the Welch sibling: one check function.  The sibling is asked
    through its from-table call with no table and good pointers (its describe call takes neither a scale nor psd_flags)."""
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    hold = getattr(B.lib(), f"bhw_describe_hold_{fam}")
    welch_describe = getattr(B.lib(), f"bhw_describe_welch_{fam}")
    buf = ctypes.create_string_buffer(1280)
    refused = 0
    for flags in (0, DETREND, POWER, POWER | DETREND, 4, 8):
        for scale, psd in ((1.0, 0), (1.0, ONESIDED), (float("nan"), ONESIDED), (1.0, 2), (float("inf"), 6)):
            for L in (400, 14):
                for kw in _CASES + [dict()]:
                    s = _seg(fam, **{k: v for k, v in kw.items() if k != "struct_size"})
                    if "struct_size" in kw:
                        s.struct_size = kw["struct_size"]
                    code = _welch_call(fam, s, flags=flags, L=L, scale=scale, psd=psd)(ref)
                    want = _err()
                    if code == BADARG and want == "table is NULL":
                        assert _passes(fam, ref, s, flags=flags, L=L, scale=scale, psd=psd), (kw, flags, _err())
                        continue
                    refused += 1
                    for call in _calls(fam, s, flags=flags, L=L, scale=scale, psd=psd):
                        assert call(ref) == code and _err() == want, (fam, kw, flags, want, _err())
                    # the describe call has neither scale nor psd_flags: with good ones it is the sibling's describe call
                    if scale == 1.0 and psd == ONESIDED:
                        assert hold(None, ref, L, ctypes.byref(s), flags, BOTH, buf, 1280) == code and _err() == want
                        assert welch_describe(None, ref, L, ctypes.byref(s), flags, buf, 1280) == code and _err() == want
    assert refused > 200
    # the words the siblings use today, spelled out
    words = {"fft": ((400, "n_fft 400"), (8192, "power of two")),
             "mfft": ((512, "n_fft 512 is a power of two: bhw_stft_fft_f32_* and bhw_spectrogram_f32_* transform it"),
                      (448, "n_fft 448: the mixed-radix fused FFT takes an even 2^a 3^b 5^c in 16..4095"))}[fam]
    for n, text in words:
        for call in _calls(fam, _seg(fam, n_fft=n)):
            assert call(ref) == UNSUPPORTED and text in _err(), _err()
    for call in _calls(fam, _seg(fam, channels=2)):
        assert call(ref) == UNSUPPORTED and "channels 2" in _err() and "real input" in _err()
    for call in _calls(fam, _seg(fam), psd=2):
        assert call(ref) == BADARG and _err() == "psd_flags 0x2 (0 or BHW_PSD_ONESIDED)"
    for call in _calls(fam, _seg(fam), scale=float("inf")):
        assert call(ref) == BADARG and _err() == "scale is not finite"
    if fam == "mfft":
        for call in _calls(fam, _seg(fam), flags=POWER | DETREND):
            assert call(ref) == BADARG and _err() == "flags 0x3: BHW_MFFT_POWER has no meaning here (BHW_WELCH_DETREND_CONSTANT)"
    for call in _calls(fam, None):
        assert call(ref) == BADARG and "descriptor is NULL" in _err()
    for call in _calls(fam, _seg(fam)):
        assert call(None) == BADARG
    for call in _calls(fam, _seg(fam), L=0):
        assert call(ref) == BADARG and "length" in _err()
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    for call in _calls(fam, _seg(fam)):
        assert call(ctypes.byref(taylor)) == UNSUPPORTED


@pytest.mark.parametrize("fam", FAMILIES)
def test_output_side_refusals_in_the_stated_order(fam):
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    K = SIZE[fam] // 2 + 1
    s = _seg(fam)
    for scale in (0.0, -1.5, 1e300):
        for psd in (0, ONESIDED):
            assert _passes(fam, ref, s, scale=scale, psd=psd)
    # p_stride is d_P's rule
    for call in _calls(fam, s, p_stride=K - 1):
        assert call(ref) == BADARG and _err() == f"p_stride {K - 1} < bins {K}: rows overlap"
    assert _passes(fam, ref, s, p_stride=K) and _passes(fam, ref, s, p_stride=K + 7)
    # 5. the pointers: d_x, both outputs NULL, each alone, alignment
    for call in _calls(fam, s, x=0):
        assert call(ref) == BADARG and _err() == "d_x is NULL"
    for call in _calls(fam, s, pmax=0, pmin=0):
        assert call(ref) == BADARG and _err() == "d_max and d_min are both NULL: no trace is asked for"
    assert _passes(fam, ref, s, pmax=0) and _passes(fam, ref, s, pmin=0)
    for kw, text in ((dict(pmax=PMAX + 2), "d_max is not 4-byte aligned"), (dict(pmin=PMIN + 2), "d_min is not 4-byte aligned"),
                     (dict(pmax=0, pmin=PMIN + 1), "d_min is not 4-byte aligned"), (dict(x=X + 2), "d_x is not 4-byte aligned")):
        for call in _calls(fam, s, **kw):
            assert call(ref) == BADARG and _err() == text, (kw, _err())
    assert _passes(fam, ref, s, pmax=PMAX + 4, pmin=PMIN + 4, x=X + 4)
    # 6. the workspace: NULL, misaligned, short (its own code), and exactly enough
    for call in _calls(fam, s, ws=0):
        assert call(ref) == BADARG and _err() == f"workspace is NULL: the chunk pairs need {_need(s)} bytes"
    for call in _calls(fam, s, ws=W + 4):
        assert call(ref) == BADARG and _err() == "workspace is not 8-byte aligned"
    for call in _calls(fam, s, ws_bytes=_need(s) - 1):
        assert call(ref) == WORKSPACE and _err() == f"workspace of {_need(s) - 1} bytes, the chunk and block pairs need {_need(s)}"
    for call in _calls(fam, s, ws_bytes=0):
        assert call(ref) == WORKSPACE
    assert _passes(fam, ref, s, ws_bytes=_need(s)) and _passes(fam, ref, s, ws_bytes=_need(s) + 8)
    # 7. overlaps: x holds 4 * 16000 floats, a trace 4 * K floats, the workspace _need(s) bytes
    xb, pb, wb = 4 * 16000 * 4, 4 * K * 4, _need(s)
    for kw, text in (
            (dict(pmax=X + xb - 4), "d_x and d_max overlap"), (dict(pmax=X + xb), None),
            (dict(pmin=X + xb - 4), "d_x and d_min overlap"), (dict(pmin=X + xb), None),
            (dict(x=PMAX + pb - 4), "d_x and d_max overlap"), (dict(x=PMAX + pb), None),
            (dict(x=PMIN + pb - 4), "d_x and d_min overlap"),
            (dict(pmin=PMAX + pb - 4), "d_max and d_min overlap"), (dict(pmin=PMAX + pb), None),
            (dict(pmin=PMAX), "d_max and d_min overlap"), (dict(pmax=PMIN + pb - 4), "d_max and d_min overlap"),
            (dict(pmax=0, pmin=PMAX), None),                                                # a trace that is not written overlaps nothing
            (dict(ws=X + xb - 8), "workspace overlaps d_x"), (dict(ws=X + xb), None),
            (dict(x=W + wb - 4), "workspace overlaps d_x"), (dict(x=W + wb), None),
            (dict(ws=PMAX + pb - 8), "workspace overlaps d_max"), (dict(pmax=W + wb - 4), "workspace overlaps d_max"), (dict(pmax=W + wb), None),
            (dict(ws=PMIN + pb - 8), "workspace overlaps d_min"), (dict(pmin=W + wb - 4), "workspace overlaps d_min"), (dict(pmin=W + wb), None),
            (dict(pmax=0, ws=PMAX), None)):
        if text:
            for call in _calls(fam, s, **kw):
                assert call(ref) == BADARG and _err() == text, (kw, _err())
        else:
            assert _passes(fam, ref, s, **kw), (kw, _err())
    # with a padded p_stride the extent of a trace grows with it
    assert _passes(fam, ref, s, p_stride=K + 8, pmin=PMAX + 4 * (3 * (K + 8) + K))
    for call in _calls(fam, s, p_stride=K + 8, pmin=PMAX + 4 * (3 * (K + 8) + K) - 4):
        assert call(ref) == BADARG and _err() == "d_max and d_min overlap"
    # the order: for each adjacent pair a call that breaks both rules; the earlier one wins
    other = 400 if fam == "fft" else 512
    order = [
        (dict(s=_seg(fam, n_fft=other, y_stride=3), psd=2, scale=float("nan")), UNSUPPORTED, "n_fft"),                 # the descriptor first
        (dict(s=_seg(fam, y_stride=3), psd=2, scale=float("nan")), BADARG, "no spectrum is written"),                  # the strides,
        (dict(s=s, psd=2, scale=float("nan")), BADARG, "psd_flags"),                                                   # psd_flags,
        (dict(s=s, scale=float("nan"), p_stride=1), BADARG, "scale is not finite"),                                    # the scale
        (dict(s=_seg(fam, frames=0), scale=float("nan"), p_stride=1, x=0), BADARG, "scale is not finite"),             # before frames 0
        (dict(s=s, p_stride=1, x=0), BADARG, "p_stride"),                                                              # before 5
        (dict(s=s, x=0, pmax=0, pmin=0, ws=0), BADARG, "d_x is NULL"),                                                 #    inside 5
        (dict(s=s, pmax=0, pmin=0, ws=0), BADARG, "both NULL"),                                                        # 5 before 6
        (dict(s=s, pmax=PMAX + 2, ws=W + 4), BADARG, "d_max is not 4-byte aligned"),
        (dict(s=s, ws=0, ws_bytes=0), BADARG, "workspace is NULL"),                                                    #    inside 6
        (dict(s=s, ws=W + 4, ws_bytes=0), BADARG, "workspace is not 8-byte aligned"),
        (dict(s=s, ws_bytes=8, x=PMAX), WORKSPACE, "workspace of 8 bytes"),                                            # 6 before 7
        (dict(s=s, x=PMAX), BADARG, "d_x and d_max overlap"),                                                          # 7 before 8
    ]
    for kw, code, text in order:
        kw = dict(kw)
        for call in _calls(fam, kw.pop("s"), **kw):
            assert call(ref) == code and text in _err(), (kw, code, _err())
    # frames 0 is OK whatever p_stride and the pointers are
    assert _fn(fam, "_f32_device")(ref, 400, 0, None, ctypes.byref(_seg(fam, frames=0)), 0, 1.0, 1, None, None, None, 1, None, 0) == OK
    assert _fn(fam, "_f32_from_table")(None, ref, 400, None, ctypes.byref(_seg(fam, frames=0)), 0, 1.0, 1, None, None, None, 0, None, 0) == BADARG
    assert "table is NULL" in _err()


def test_the_output_side_words_are_one_text_for_all_four_families():
    """hold_pointer_checks is one function: the words of the real-input calls are those of the I/Q calls."""
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    iq = B.make_stft(4, 16000, 98, 160, 512, channels=2, shift=31)
    iq_need = 8 * H.WF.workspace_doubles(4, 98, 512)
    for kw in (dict(x=0), dict(pmax=0, pmin=0), dict(pmax=PMAX + 2), dict(pmin=PMIN + 2), dict(x=X + 2), dict(ws=W + 4), dict(ws=0),
               dict(x=PMAX), dict(pmin=PMAX), dict(ws=X), dict(ws=PMIN)):
        a = dict(x=X, pmax=PMAX, pmin=PMIN, ws=W)
        a.update(kw)
        rc = B.lib().bhw_hold_cfft_f32_device(ref, 400, 0, None, ctypes.byref(iq), DETREND, 1.0, ctypes.c_void_p(a["x"]), ctypes.c_void_p(a["pmax"]),
                                              ctypes.c_void_p(a["pmin"]), 0, ctypes.c_void_p(a["ws"]), iq_need)
        words = [(rc, _err().replace(str(iq_need), "NEED"))]
        for fam in FAMILIES:
            rc = _calls(fam, _seg(fam), **kw)[0](ref)
            words.append((rc, _err().replace(str(_need(_seg(fam))), "NEED")))
        assert words[0] == words[1] == words[2] and words[0][0] == BADARG, (kw, words)


@pytest.mark.parametrize("cid", H.case_ids())
def test_workspace_bytes_are_the_siblings(cid):
    c = H.case(cid)
    fam = c["family"]
    s, _, F, _ = H.desc(fam, c)
    want = 8 * H.WF.workspace_doubles(c["B"], F, c["n_fft"] // 2 + 1)
    assert H.HOLD_WS[fam](s) == H.WELCH_WS[fam](s) == want == H.parse(fam, H.line(fam, c))["workspace"]
    p = H.params(c["setup"])
    assert _passes(fam, ctypes.byref(p), s, L=c["L"], flags=int(c["detrend"]), ws_bytes=want), _err()
    for call in _calls(fam, s, L=c["L"], flags=int(c["detrend"]), ws_bytes=want - 8):
        assert call(ctypes.byref(p)) == WORKSPACE, _err()


def test_workspace_bytes_sweep_and_of_nothing():
    for fam in FAMILIES:
        for n in H.SIZES[fam]:
            for nb in (1, 5, 64):
                for F in (1, 15, 16, 17, 256, 257, 998, 4097, 131142):
                    s = B.make_stft(nb, (F - 1) * 3 + n, F, 3, n, shift=31)
                    assert H.HOLD_WS[fam](s) == H.WELCH_WS[fam](s) == 8 * H.WF.workspace_doubles(nb, F, n // 2 + 1) > 0
        assert _fn(fam, "_workspace_bytes")(None) == 0
        assert H.HOLD_WS[fam](_seg(fam, frames=0)) == 0
        s = _seg(fam)
        s.struct_size = 80
        assert H.HOLD_WS[fam](s) == 0


@pytest.mark.parametrize("fam", FAMILIES)
def test_every_supported_size_passes_and_its_neighbours_do_not(fam):
    p = B.make_params(B.WIN_BH7, 16, 32)
    hold = getattr(B.lib(), f"bhw_describe_hold_{fam}")
    welch = getattr(B.lib(), f"bhw_describe_welch_{fam}")
    buf = ctypes.create_string_buffer(1280)
    ok = []
    for n in list(range(1, 4200)) + [4320, 4374, 4500, 8192]:
        s = B.make_stft(2, 100000, 3, 7, n, shift=31)
        rc = hold(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), DETREND, BOTH, buf, 1280)
        got = _err() if rc else None
        assert rc == welch(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), DETREND, buf, 1280), n
        if rc:
            assert got == _err(), n
        else:
            ok.append(n)
    assert ok == H.SIZES[fam]


@pytest.mark.parametrize("fam", FAMILIES)
def test_frames_zero_and_the_describe_line(fam):
    p = B.make_params(B.WIN_BH7, 16, 32)
    ref = ctypes.byref(p)
    N = SIZE[fam]
    K = N // 2 + 1
    describe = H._DESCRIBE[fam]
    for flags in (0, DETREND):
        s = _seg(fam, frames=0)
        assert _fn(fam, "_f32_device")(ref, 400, 0, None, ctypes.byref(s), flags, 1.0, 1, None, None, None, 0, None, 0) == OK
        line = describe(p, 400, s, detrend=bool(flags & DETREND), traces="min")
        assert line.startswith(f"hold {fam} direct (L = 400, n_fft {N}, ") and line.endswith(": nothing (frames 0); traces: min")
        assert _fn(fam, "_f32_device")(ref, 400, 0, None, ctypes.byref(s), flags, float("nan"), 1, None, None, None, 0, None, 0) == BADARG
    s = _seg(fam, batch=64, samples=160000, frames=998)
    line = describe(p, 400, s, detrend=True)
    assert line.startswith(f"hold {fam} direct (L = 400, n_fft {N}, col0 0, pad 0 constant, constant detrend): "
                           f"k_hold_{fam}_direct<2>, 64 signals x 998 frames = 63872 rows, complex FFT of {N // 2} points in passes ")
    assert line.endswith("chunk 16 frames, 4032 runs of 16 frames (4 groups per run), "
                         f"{-(-K // 256)} accumulator{'s' if K > 256 else ''} per lane, 63 chunks and 4 blocks per signal, then k_hold_join "
                         f"twice (chunks, blocks), workspace {8 * 64 * K * 67} bytes; traces: max, min")
    assert H.to_welch(fam, line) == H._WELCH[fam](p, 400, s, detrend=True)
    assert describe(p, 400, s, traces="max").endswith("; traces: max")
    # the traces of the describe call: a non-empty subset of the two bits
    fn = getattr(B.lib(), f"bhw_describe_hold_{fam}")
    buf = ctypes.create_string_buffer(1280)
    for t in (0, 4, 7):
        assert fn(None, ref, 400, ctypes.byref(s), 0, t, buf, 1280) == BADARG and "BHW_HOLD_MAX | BHW_HOLD_MIN" in _err()
    with pytest.raises(ValueError, match="traces must be 'both', 'max' or 'min'"):
        describe(p, 400, s, traces="median")
    small = ctypes.create_string_buffer(16)
    assert fn(None, ref, 400, ctypes.byref(s), 0, BOTH, small, 16) == OK and len(small.value) == 15
    assert fn(None, ref, 400, ctypes.byref(s), 0, BOTH, None, 0) == BADARG


def test_the_older_calls_keep_their_messages():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    lib = B.lib()
    P = PMAX
    tail = lambda s, **kw: (ctypes.byref(s), kw.get("flags", 1), kw.get("scale", 1.0), kw.get("psd", 1), ctypes.c_void_p(kw.get("x", X)),   # noqa: E731
                            ctypes.c_void_p(kw.get("out", P)), kw.get("p_stride", 0), ctypes.c_void_p(kw.get("ws", W)), kw.get("ws_bytes", 1 << 30))
    for fam, fn in (("fft", lib.bhw_welch_fft_f32_device), ("mfft", lib.bhw_welch_mfft_f32_device)):
        s = _seg(fam)
        K, need = SIZE[fam] // 2 + 1, _need(s)
        for kw, code, text in (
                (dict(scale=float("inf")), BADARG, "scale is not finite"),
                (dict(psd=2), BADARG, "psd_flags 0x2 (0 or BHW_PSD_ONESIDED)"),
                (dict(p_stride=K - 1), BADARG, f"p_stride {K - 1} < bins {K}: rows overlap"),
                (dict(x=0), BADARG, "d_x / d_P is NULL"),
                (dict(out=P + 2), BADARG, "d_P is not 4-byte aligned"),
                (dict(x=X + 2), BADARG, "d_x is not 4-byte aligned"),
                (dict(ws=0), BADARG, f"workspace is NULL: the chunk sums need {need} bytes"),
                (dict(ws=W + 4), BADARG, "workspace is not 8-byte aligned"),
                (dict(ws_bytes=8), WORKSPACE, f"workspace of 8 bytes, the chunk and block sums need {need}"),
                (dict(x=P), BADARG, "d_x and d_P overlap"),
                (dict(ws=X), BADARG, "workspace overlaps d_x or d_P")):
            assert fn(ref, 400, 0, None, *tail(s, **kw)) == code and _err() == text, (kw, _err())
    # the I/Q hold calls keep theirs too, now that hold_pointer_checks takes the bins and the floats of a signal
    iq = B.make_stft(4, 16000, 98, 160, 512, channels=2, shift=31)
    need = 8 * H.WF.workspace_doubles(4, 98, 512)
    call = lambda **kw: lib.bhw_hold_cfft_f32_device(ref, 400, 0, None, ctypes.byref(iq), 1, 1.0, ctypes.c_void_p(kw.get("x", X)),   # noqa: E731
                                                     ctypes.c_void_p(PMAX), ctypes.c_void_p(kw.get("pmin", PMIN)), kw.get("p_stride", 0),
                                                     ctypes.c_void_p(kw.get("ws", W)), kw.get("ws_bytes", need))
    assert call(p_stride=511) == BADARG and _err() == "p_stride 511 < n_fft 512: rows overlap"
    assert call(ws=0) == BADARG and _err() == f"workspace is NULL: the chunk pairs need {need} bytes"
    assert call(ws_bytes=need - 1) == WORKSPACE and _err() == f"workspace of {need - 1} bytes, the chunk and block pairs need {need}"
    assert call(pmin=X + 4 * 32000 * 4 - 4) == BADARG and _err() == "d_x and d_min overlap"
    assert call(pmin=PMAX + 4 * 512 * 4 - 4) == BADARG and _err() == "d_max and d_min overlap"
    # the describe lines of the siblings are as they were, now that they share their text with the hold lines
    big = dict(batch=64, samples=160000, frames=998)
    assert B.describe_welch_fft(p, 400, _seg("fft", **big), detrend=True) == (
        "welch fft direct (L = 400, n_fft 512, col0 0, pad 0 constant, constant detrend): k_welch_fft_direct<2>, "
        "64 signals x 998 frames = 63872 rows, complex FFT of 256 points in passes 4x4x4x4 + split, 64 lanes per row x 4 rows per "
        "workgroup, 8 columns per lane, 16128 groups, grid 2048 x 256 lanes, 18448 bytes of LDS; chunk 16 frames, 4032 runs of 16 frames "
        "(4 groups per run), 2 accumulators per lane, 63 chunks and 4 blocks per signal, then k_welch_fft_join twice (chunks, blocks), "
        f"workspace {8 * 64 * 257 * 67} bytes")
    assert B.describe_welch_fft(p, 400, _seg("fft", frames=0)) == "welch fft direct (L = 400, n_fft 512, no detrending): nothing (frames 0)"
    assert B.describe_welch_mfft(p, 400, _seg("mfft", frames=0)) == "welch mfft direct (L = 400, n_fft 400, no detrending): nothing (frames 0)"
    w = B.describe_welch_mfft(p, 400, _seg("mfft", **big), detrend=True)
    assert w.startswith("welch mfft direct (L = 400, n_fft 400, col0 0, pad 0 constant, constant detrend): k_welch_mfft_direct<2>, 64 signals x "
                        "998 frames = 63872 rows, complex FFT of 200 points in passes ")
    assert w.endswith("chunk 16 frames, 4032 runs of 16 frames (4 groups per run), 1 accumulator per lane, 63 chunks and 4 blocks per signal, "
                      f"then k_welch_fft_join twice (chunks, blocks), workspace {8 * 64 * 201 * 67} bytes")


def test_python_surface_and_signatures():
    names = ("hold_fft", "hold_fft_mixed", "hold_fused", "hold_fused_mixed", "describe_hold_fft", "describe_hold_mfft",
             "hold_fft_workspace_bytes", "hold_mfft_workspace_bytes")
    for name in names:
        assert name in bhw.__all__ and hasattr(bhw, name), name
    for name in names[4:]:
        assert getattr(B, name) is getattr(bhw, name)
    assert inspect.signature(B.describe_hold_fft) == inspect.signature(B.describe_hold_mfft)
    assert list(inspect.signature(B.describe_hold_fft).parameters) == ["params", "length", "stft", "detrend", "traces", "table"]
    sig = inspect.signature(bhw.hold_fft)
    assert str(sig) == ("(params, x, n_fft, hop, scale=1.0, *, win_length=None, center=False, pad_mode='reflect', detrend=False, "
                        "onesided_doubling=True, shift=None, traces='both', out_max=None, out_min=None, workspace=None)")
    assert inspect.signature(bhw.hold_fft_mixed) == sig
    fsig = inspect.signature(bhw.hold_fused)
    assert str(fsig) == ("(params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend='constant', scaling='density', shift=None, "
                         "traces='both', out_max=None, out_min=None, workspace=None)")
    assert inspect.signature(bhw.hold_fused_mixed) == fsig
    for name, want in (("hold_fft", sig), ("hold_fft_mixed", sig), ("hold_fused", fsig), ("hold_fused_mixed", fsig)):
        got = inspect.signature(getattr(bhw.ResidentTable, name))
        assert list(got.parameters)[1:] == list(want.parameters), name
        assert [q.default for q in got.parameters.values()][1:] == [q.default for q in want.parameters.values()], name
        assert [q.kind for q in got.parameters.values()][1:] == [q.kind for q in want.parameters.values()], name
    # the arguments are the Welch siblings' but for the outputs and the default of scale
    for new, old in (("hold_fft", "welch_fft"), ("hold_fft_mixed", "welch_fft_mixed"), ("hold_fused", "welch_fused"),
                     ("hold_fused_mixed", "welch_fused_mixed")):
        a, b = list(inspect.signature(getattr(bhw, new)).parameters), list(inspect.signature(getattr(bhw, old)).parameters)
        assert [q for q in a if q not in ("traces", "out_max", "out_min")] == [q for q in b if q != "out"], new
    # existing signatures do not change
    assert list(inspect.signature(bhw.welch_fft).parameters) == ["params", "x", "n_fft", "hop", "scale", "win_length", "center", "pad_mode",
                                                                "detrend", "onesided_doubling", "shift", "out", "workspace"]
    assert list(inspect.signature(bhw.welch_fused_mixed).parameters) == ["params", "x", "fs", "length", "noverlap", "nfft", "detrend", "scaling",
                                                                        "shift", "out", "workspace"]
    assert str(inspect.signature(bhw.hold_fft_iq)) == (
        "(params, x, n_fft, hop, scale=1.0, *, win_length=None, center=False, pad_mode='reflect', detrend=False, shift=None, "
        "fftshift=False, traces='both', out_max=None, out_min=None, workspace=None)")


def test_every_value_error_is_raised_before_the_device_is_looked_at():
    """On CPU tensors, with no GPU: the fronts hand their arguments to the Welch siblings' two functions, whose checks -- and the check
    of `traces` and the hold calls' own refusals before them -- raise before any device call."""
    torch = pytest.importorskip("torch")
    from blackman_harris_win_amd import selector
    p = B.make_params(B.WIN_BH4, 24, 32)
    z = torch.zeros(4000, dtype=torch.float32)

    def fft(x, n, fam, hold, scale=1.0):
        return selector._welch_fft_psd(torch, p, x, n, 160, scale, None, False, "reflect", False, True, None, None, None, 0, None, fam, hold)

    def fused(x, n, fam, hold, **kw):
        a = dict(noverlap=None, detrend="constant", scaling="density")
        a.update(kw)
        return selector._welch_fused(torch, p, x, 1.0, 400, a["noverlap"], n, a["detrend"], a["scaling"], None, None, None, 0, None, {}, fam,
                                     hold)

    both = ("both", None, None)
    for fam, n in (("fft", 512), ("mfft", 400)):
        for bad in ("median", None, "MAX", 3):
            with pytest.raises(ValueError, match="traces must be 'both', 'max' or 'min'"):
                fft(z, n, fam, (bad, None, None))
            with pytest.raises(ValueError, match="traces must be 'both', 'max' or 'min'"):
                fused(z, n, fam, (bad, None, None))
        # what both the hold call and its Welch sibling refuse in the same words: a float64 x, an unsupported n_fft, a CPU tensor
        for x, size in ((z.double(), n), (z, 448), (z, 4374), (z, n)):
            words = []
            for hold in (both, None):
                with pytest.raises(ValueError) as e:
                    fft(x, size, fam, hold)
                words.append(str(e.value))
                with pytest.raises(ValueError) as e:
                    fused(x, size, fam, hold)
                words.append(str(e.value))
            assert words[0] == words[2] and words[1] == words[3], words
        for kw, text in ((dict(detrend="linear"), "detrend must be"), (dict(scaling="power"), "scaling must be"),
                         (dict(noverlap=400), "noverlap must be less than length")):
            with pytest.raises(ValueError, match=text):
                fused(z, n, fam, both, **kw)
    # the hold calls' own words: each names the hold call that takes what it refuses
    zc = torch.zeros(4000, dtype=torch.complex64)
    for call in (fft, fused):
        with pytest.raises(ValueError, match="n_fft 400 is mixed-radix: hold_fft_mixed / hold_fused_mixed transform it"):
            call(z, 400, "fft", both)
        with pytest.raises(ValueError, match="n_fft 512 is a power of two: hold_fft / hold_fused transform it"):
            call(z, 512, "mfft", both)
        with pytest.raises(ValueError, match="hold_fft_iq / hold_fused_iq"):
            call(zc, 512, "fft", both)
        with pytest.raises(ValueError, match="hold_fft_iq_mixed / hold_fused_iq_mixed"):
            call(zc, 400, "mfft", both)
    # hold_fft_iq still refuses real input with today's message
    with pytest.raises(ValueError) as e:
        selector._welch_cfft_psd(torch, p, z, 512, 160, 1.0, None, False, "reflect", False, None, False, None, None, 0, None, "cfft", both)
    with pytest.raises(ValueError) as w:
        selector._welch_cfft_psd(torch, p, z, 512, 160, 1.0, None, False, "reflect", False, None, False, None, None, 0, None, "cfft", None)
    assert str(e.value) == str(w.value) and "complex64" in str(e.value)
    # the fronts pass these two functions their arguments and nothing else
    src = inspect.getsource(selector.hold_fft) + inspect.getsource(selector.hold_fft_mixed)
    assert src.count("return _welch_fft_psd(") == 2 and "(traces, out_max, out_min)" in src
    src = inspect.getsource(selector.hold_fused) + inspect.getsource(selector.hold_fused_mixed)
    assert src.count("return _welch_fused(") == 2 and "_SUMS_CACHE" in src
