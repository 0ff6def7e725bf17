"""The fused max-hold / min-hold calls for I/Q input, both families (bhw_hold_cfft_f32_* and bhw_hold_cmfft_f32_*, their
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

import hold_iq_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
FAMILIES = ("cfft", "cmfft")
NEW_SYMBOLS = tuple(f"bhw_hold_{f}{t}" for f in FAMILIES for t in ("_workspace_bytes", "_f32_device", "_f32_from_table")) + \
    ("bhw_describe_hold_cfft", "bhw_describe_hold_cmfft")
# never dereferenced: every call below fails or has nothing to do
X, PMAX, PMIN, W = 0x10000000, 0x80000000, 0x90000000, 0x40000000
SIZE = {"cfft": 512, "cmfft": 600}
DETREND, POWER, SHIFT = 1, 2, 4
BOTH = 3


def _err():
    return B.lib().bhw_last_error().decode()


def _seg(fam, **kw):
    """Welch framing of I/Q input: 4 signals of 16000 complex samples, window 400 in rows of 512 / 600, hop 160, no padding: 98
    frames, 7 chunks, one block."""
    a = dict(batch=4, samples=16000, frames=98, hop=160, n_fft=SIZE[fam], channels=2, shift=31)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _need(s):
    return 8 * H.WC.workspace_doubles(s.batch, s.frames, s.n_fft)


def _fn(fam, tail):
    return getattr(B.lib(), f"bhw_hold_{fam}{tail}")


def _calls(fam, s, flags=DETREND, L=400, scale=1.0, x=X, pmax=PMAX, pmin=PMIN, p_stride=0, ws=W, ws_bytes=None):
    sr = ctypes.byref(s) if s is not None else None
    nbytes = (_need(s) if s is not None else 0) if ws_bytes is None else ws_bytes
    tail = (sr, flags, scale, ctypes.c_void_p(x), ctypes.c_void_p(pmax), ctypes.c_void_p(pmin), p_stride, ctypes.c_void_p(ws), nbytes)
    return (lambda p: _fn(fam, "_f32_device")(p, L, 0, None, *tail),
            lambda p: _fn(fam, "_f32_from_table")(None, p, L, None, *tail))


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
    assert re.search(r"#define BHW_HOLD_MAX 1u\n#define BHW_HOLD_MIN 2u\n", header) and (B.HOLD_MAX, B.HOLD_MIN) == (1, 2)
    # the new sections stand after bhw_describe_welch_cmfft, outside every existing section
    at = header.index("Fused max-hold and min-hold traces for complex (I/Q) input")
    assert at > header.index("int bhw_describe_welch_cmfft(") and at < header.index("/* Fused Welch cross spectra")
    end = header.index("int bhw_describe_hold_cmfft(")
    text = header[at:end]
    for words in ("Either may be NULL", "Both NULL is BHW_ERR_BADARG", "BHW_CFFT_POWER is refused", "over the live frames f < F only",
                  "fl32((double) max_f h_f * scale)", "fl32((double) min_f h_f * scale)", "(j + n_fft / 2) mod n_fft", "integer division",
                  "torch.fft.fftshift", "both traces of that bin are NaN", "unsigned integers", "not on B,", "the order of the reduction",
                  "library versus table", "At EVERY F", "bit for bit", "there is no ulp clause", "no float atomics",
                  "bhw_hold_cfft_workspace_bytes(s) = bhw_welch_cfft_workspace_bytes(s)",
                  "bhw_hold_cmfft_workspace_bytes(s) = bhw_welch_cmfft_workspace_bytes(s)", "The layout inside is not part of the contract",
                  "BHW_ERR_WORKSPACE", "with the pointers unchecked", "Both traces are always computed", "the same check function",
                  "Not built: median or percentile traces; the mean in the same launch", "real input", "the traces asked for"):
        assert words in text, words
    assert [int(m) for m in re.findall(r"\n \*       (\d)\. ", text)] == [1, 5, 6, 7, 8]
    # the four older "Not built" sentences stand word for word, each followed by a pointer to the new calls
    for old, new in (
            ("Not built: max-hold or median averaging; a filter bank on the averaged powers.", "bhw_hold_cfft_f32_* and bhw_hold_cmfft_f32_* below"),
            ("Not built: max-hold or median traces; n_fft 4096; I/Q cross spectra accumulated in the kernel (real input:", "bhw_hold_cfft_f32_* below"),
            ("Not built: odd n_fft and factors >= 7; cross spectra at these lengths in one kernel; max-hold or median traces.",
             "bhw_hold_cmfft_f32_* below"),
            ("Not built: n_fft >= 2048; factors of 7 and above; I/Q cross spectra accumulated in the kernel; max-hold or median traces.",
             "bhw_hold_cmfft_f32_* below")):
        i = header.index(old)
        section = header[i:header.index("\n *   - bhw_describe_", i)]
        assert new in section and section.count("(") >= 1, old
        assert header.count(old) == 1


def test_the_two_families_have_one_prototype():
    header = _header()
    flat = lambda t: re.sub(r"\s+", " ", t)
    for kind, tail in (("int", "_f32_device"), ("int", "_f32_from_table"), ("uint64_t", "_workspace_bytes")):
        a = re.search(kind + r" bhw_hold_cfft" + tail + r"\(([^;]*)\);", header).group(1)
        b = re.search(kind + r" bhw_hold_cmfft" + tail + r"\(([^;]*)\);", header).group(1)
        assert flat(a) == flat(b), tail
    a = re.search(r"int bhw_describe_hold_cfft\(([^;]*)\);", header).group(1)
    assert flat(a) == flat(re.search(r"int bhw_describe_hold_cmfft\(([^;]*)\);", header).group(1))
    # the issue's prototype, word for word
    want = ("const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags, double scale, "
            "const float *d_x, float *d_max, float *d_min, uint64_t p_stride, void *workspace, uint64_t workspace_bytes")
    assert flat(re.search(r"int bhw_hold_cfft_f32_device\(([^;]*)\);", header).group(1)) == want
    # the Welch sibling's, with the two outputs in d_P's place
    old = flat(re.search(r"int bhw_welch_cfft_f32_device\(([^;]*)\);", header).group(1))
    assert old.replace("float *d_P,", "float *d_max, float *d_min,") == want
    L = B.lib()
    for tail in ("_workspace_bytes", "_f32_device", "_f32_from_table"):
        assert _fn("cfft", tail).argtypes == _fn("cmfft", tail).argtypes and _fn("cfft", tail).restype == _fn("cmfft", tail).restype
    assert L.bhw_describe_hold_cfft.argtypes == L.bhw_describe_hold_cmfft.argtypes


@pytest.mark.parametrize("fam", FAMILIES)
def test_input_side_refusals_are_the_welch_siblings_word_for_word(fam):
    """Every input-side refusal carries the code and the exact message of the Welch sibling's describe call: one check function."""
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    welch = getattr(B.lib(), f"bhw_describe_welch_{fam}")
    hold = getattr(B.lib(), f"bhw_describe_hold_{fam}")
    cases = [dict(struct_size=8), dict(channels=3), dict(channels=1), dict(batch=0), dict(hop=0), dict(n_fft=0), dict(n_fft=256),
             dict(n_fft=512), dict(n_fft=600), dict(n_fft=400), dict(n_fft=4096), dict(n_fft=448), dict(n_fft=2160), dict(n_fft=601),
             dict(n_fft=2048), dict(shift=63), dict(frames=99), dict(samples=0), dict(x_stride=31999), dict(pad=300), dict(col0=100),
             dict(pad_mode=B.PAD_REFLECT), dict(y_stride=3), dict(y_batch_stride=7), dict(channels=1, n_fft=448)]
    buf = ctypes.create_string_buffer(1280)
    refused = 0
    for flags in (0, DETREND, SHIFT, DETREND | SHIFT, POWER, POWER | DETREND | SHIFT, 8):
        for scale in (1.0, float("nan")):
            for kw in cases + [dict()]:
                s = _seg(fam, **{k: v for k, v in kw.items() if k != "struct_size"})
                if "struct_size" in kw:
                    s.struct_size = kw["struct_size"]
                # the sibling's describe call has no scale: its check function is reached through the call itself for the scale
                code = welch(None, ref, 400, ctypes.byref(s), flags, buf, 1280)
                want = _err() if code else None
                if code == OK and scale != scale:
                    code, want = BADARG, "scale is not finite"
                if code == OK:
                    assert _passes(fam, ref, s, flags=flags, scale=scale), (kw, flags, _err())
                    continue
                refused += 1
                for call in _calls(fam, s, flags=flags, scale=scale):
                    assert call(ref) == code and _err() == want, (fam, kw, flags, want, _err())
                if scale == scale:
                    assert hold(None, ref, 400, ctypes.byref(s), flags, BOTH, buf, 1280) == code and _err() == want
    assert refused > 200
    # the words the siblings use today, spelled out for the sizes the issue names
    pow2 = "n_fft {}: the fused complex FFT takes a power of two in 16..2048"
    is_pow2 = "n_fft {} is a power of two: bhw_stft_cfft_f32_* transforms it (one transform per n_fft)"
    no_size = "n_fft {}: the mixed-radix fused complex FFT takes 2^a 3^b 5^c in 16..2047"
    words = {"cfft": ((448, pow2), (2160, pow2), (600, pow2), (4096, pow2)),
             "cmfft": ((448, no_size), (2160, no_size), (512, is_pow2), (2048, is_pow2))}[fam]
    for n, text in words:
        for call in _calls(fam, _seg(fam, n_fft=n)):
            assert call(ref) == UNSUPPORTED and _err() == text.format(n), _err()
    for call in _calls(fam, _seg(fam, channels=1)):
        assert call(ref) == UNSUPPORTED and "channels 1" in _err() and "real input" in _err()
    for flags in (POWER, POWER | DETREND | SHIFT):
        for call in _calls(fam, _seg(fam), flags=flags):
            assert call(ref) == BADARG and _err() == (f"flags 0x{flags:x}: BHW_CFFT_POWER has no meaning here (BHW_WELCH_DETREND_CONSTANT, "
                                                      "BHW_CFFT_SHIFT)")
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
    N = SIZE[fam]
    s = _seg(fam)
    for scale in (0.0, -1.5, 1e300):
        assert _passes(fam, ref, s, scale=scale)
    # 4. p_stride is d_P's rule
    for call in _calls(fam, s, p_stride=N - 1):
        assert call(ref) == BADARG and _err() == f"p_stride {N - 1} < n_fft {N}: rows overlap"
    assert _passes(fam, ref, s, p_stride=N) and _passes(fam, ref, s, p_stride=N + 7)
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
    # 7. overlaps: x holds 4 * 32000 floats, a trace 4 * N floats, the workspace _need(s) bytes
    xb, pb, wb = 4 * 32000 * 4, 4 * N * 4, _need(s)
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
    assert _passes(fam, ref, s, p_stride=N + 8, pmin=PMAX + 4 * (3 * (N + 8) + N))
    for call in _calls(fam, s, p_stride=N + 8, pmin=PMAX + 4 * (3 * (N + 8) + N) - 4):
        assert call(ref) == BADARG and _err() == "d_max and d_min overlap"
    # the order: for each adjacent pair of the header's list a call that breaks both rules; the earlier one wins
    other = 600 if fam == "cfft" else 512
    order = [
        (dict(s=_seg(fam, n_fft=other, y_stride=3), flags=POWER, scale=float("nan")), UNSUPPORTED, "n_fft"),           # 1 before 2
        (dict(s=_seg(fam, y_stride=3), flags=POWER, scale=float("nan")), BADARG, "BHW_CFFT_POWER"),                    # 2: the flag,
        (dict(s=_seg(fam, y_stride=3), scale=float("nan")), BADARG, "no spectrum is written"),                         #    the strides,
        (dict(s=s, scale=float("nan"), p_stride=1), BADARG, "scale is not finite"),                                    #    the scale
        (dict(s=_seg(fam, frames=0), scale=float("nan"), p_stride=1, x=0), BADARG, "scale is not finite"),             # 2 before 3
        (dict(s=s, p_stride=1, x=0), BADARG, "p_stride"),                                                              # 4 before 5
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
    # 3 before 4 and 5: frames 0 is OK whatever p_stride and the pointers are
    assert _fn(fam, "_f32_device")(ref, 400, 0, None, ctypes.byref(_seg(fam, frames=0)), 0, 1.0, None, None, None, 1, None, 0) == OK
    assert _fn(fam, "_f32_from_table")(None, ref, 400, None, ctypes.byref(_seg(fam, frames=0)), 0, 1.0, None, None, None, 0, None, 0) == BADARG
    assert "table is NULL" in _err()


def test_the_output_side_words_are_one_text_for_both_families():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    for kw in (dict(flags=POWER), dict(scale=float("nan")), dict(p_stride=1), dict(x=0), dict(pmax=0, pmin=0), dict(pmax=PMAX + 2),
               dict(pmin=PMIN + 2), dict(x=X + 2), dict(ws=W + 4), dict(ws=0), dict(x=PMAX), dict(pmin=PMAX), dict(ws=X), dict(ws=PMIN)):
        words = []
        for fam in FAMILIES:
            rc = _calls(fam, _seg(fam), **kw)[0](ref)
            words.append((rc, _err().replace(str(SIZE[fam]), "N").replace(str(_need(_seg(fam))), "NEED")))
        assert words[0] == words[1] and words[0][0] == BADARG, (kw, words)


@pytest.mark.parametrize("cid", H.case_ids())
def test_workspace_bytes_are_the_siblings(cid):
    c = H.case(cid)
    fam = c["family"]
    s, _, F, _ = H.desc(c)
    welch = {"cfft": B.welch_cfft_workspace_bytes, "cmfft": B.welch_cmfft_workspace_bytes}[fam]
    hold = {"cfft": B.hold_cfft_workspace_bytes, "cmfft": B.hold_cmfft_workspace_bytes}[fam]
    want = 8 * H.WC.workspace_doubles(c["B"], F, c["n_fft"])
    assert hold(s) == welch(s) == want == H.parse(fam, H.line(fam, c))["workspace"]
    p = H.params(c["setup"])
    for flags in (int(c["detrend"]), int(c["detrend"]) | SHIFT):
        assert _passes(fam, ctypes.byref(p), s, L=c["L"], flags=flags, ws_bytes=want), _err()
        for call in _calls(fam, s, L=c["L"], flags=flags, ws_bytes=want - 8):
            assert call(ctypes.byref(p)) == WORKSPACE, _err()


def test_workspace_bytes_sweep_and_of_nothing():
    for fam in FAMILIES:
        welch = {"cfft": B.welch_cfft_workspace_bytes, "cmfft": B.welch_cmfft_workspace_bytes}[fam]
        hold = {"cfft": B.hold_cfft_workspace_bytes, "cmfft": B.hold_cmfft_workspace_bytes}[fam]
        for n in H.SIZES[fam]:
            for nb in (1, 5, 64):
                for F in (1, 15, 16, 17, 256, 257, 998, 4097, 131142):
                    s = B.make_stft(nb, (F - 1) * 3 + n, F, 3, n, channels=2, shift=31)
                    assert hold(s) == welch(s) == 8 * H.WC.workspace_doubles(nb, F, n) > 0
        assert _fn(fam, "_workspace_bytes")(None) == 0
        assert hold(_seg(fam, frames=0)) == 0
        s = _seg(fam)
        s.struct_size = 80
        assert hold(s) == 0


@pytest.mark.parametrize("fam", FAMILIES)
def test_every_supported_size_passes_and_its_neighbours_do_not(fam):
    p = B.make_params(B.WIN_BH7, 16, 32)
    hold = getattr(B.lib(), f"bhw_describe_hold_{fam}")
    welch = getattr(B.lib(), f"bhw_describe_welch_{fam}")
    buf = ctypes.create_string_buffer(1280)
    ok = []
    for n in list(range(1, 2101)) + [2160, 2187, 2250, 4050, 4096]:
        s = B.make_stft(2, 100000, 3, 7, n, channels=2, shift=31)
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
    describe = {"cfft": B.describe_hold_cfft, "cmfft": B.describe_hold_cmfft}[fam]
    for flags in (0, DETREND, SHIFT):
        s = _seg(fam, frames=0)
        assert _fn(fam, "_f32_device")(ref, 400, 0, None, ctypes.byref(s), flags, 1.0, None, None, None, 0, None, 0) == OK
        line = describe(p, 400, s, detrend=bool(flags & DETREND), fftshift=bool(flags & SHIFT), traces="min")
        assert line.startswith(f"hold {fam} direct (L = 400, n_fft {N}, ") and line.endswith(": nothing (frames 0); traces: min")
        assert _fn(fam, "_f32_device")(ref, 400, 0, None, ctypes.byref(s), flags, float("nan"), None, None, None, 0, None, 0) == BADARG
    s = _seg(fam, batch=64, samples=160000, frames=998)
    line = describe(p, 400, s, detrend=True)
    assert line.startswith(f"hold {fam} direct (L = 400, n_fft {N}, col0 0, pad 0 constant, constant detrend), bins in order: "
                           f"k_hold_{fam}_direct<2>, 64 signals x 998 frames = 63872 rows, complex FFT of {N} points in passes ")
    gpr = {"cfft": 8, "cmfft": 16}[fam]                           # 512: two rows side by side; 600: one
    assert line.endswith(f"chunk 16 frames, 4032 runs of 16 frames ({gpr} groups per run), "
                         f"{-(-N // 256)} accumulators per lane, 63 chunks and 4 blocks per signal, then k_hold_join twice (chunks, blocks), "
                         f"workspace {8 * 64 * N * 67} bytes; traces: max, min")
    assert "bins shifted" in describe(p, 400, s, detrend=True, fftshift=True)
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
    tail = lambda s, **kw: (ctypes.byref(s), kw.get("flags", 1), kw.get("scale", 1.0), ctypes.c_void_p(kw.get("x", X)), ctypes.c_void_p(kw.get("out", P)),
                            kw.get("p_stride", 0), ctypes.c_void_p(kw.get("ws", W)), kw.get("ws_bytes", 1 << 30))
    for fam, fn in (("cfft", lib.bhw_welch_cfft_f32_device), ("cmfft", lib.bhw_welch_cmfft_f32_device)):
        s = _seg(fam)
        N, need = SIZE[fam], _need(s)
        for kw, code, text in (
                (dict(flags=POWER | DETREND), BADARG, "flags 0x3: BHW_CFFT_POWER has no meaning here (BHW_WELCH_DETREND_CONSTANT, BHW_CFFT_SHIFT)"),
                (dict(scale=float("inf")), BADARG, "scale is not finite"),
                (dict(p_stride=N - 1), BADARG, f"p_stride {N - 1} < n_fft {N}: rows overlap"),
                (dict(x=0), BADARG, "d_x / d_P is NULL"),
                (dict(out=P + 2), BADARG, "d_P is not 4-byte aligned"),
                (dict(x=X + 2), BADARG, "d_x is not 4-byte aligned"),
                (dict(ws=0), BADARG, f"workspace is NULL: the chunk sums need {need} bytes"),
                (dict(ws=W + 4), BADARG, "workspace is not 8-byte aligned"),
                (dict(ws_bytes=8), WORKSPACE, f"workspace of 8 bytes, the chunk and block sums need {need}"),
                (dict(x=P), BADARG, "d_x and d_P overlap"),
                (dict(ws=X), BADARG, "workspace overlaps d_x or d_P")):
            assert fn(ref, 400, 0, None, *tail(s, **kw)) == code and _err() == text, (kw, _err())
    # the describe lines of the siblings are as they were, now that they share their text with the hold lines
    big = dict(batch=64, samples=160000, frames=998)
    assert B.describe_welch_cfft(p, 400, _seg("cfft", **big), detrend=True) == (
        "welch cfft direct (L = 400, n_fft 512, col0 0, pad 0 constant, constant detrend), bins in order: k_welch_cfft_direct<2>, "
        "64 signals x 998 frames = 63872 rows, complex FFT of 512 points in passes 4x4x4x4x2 (no split), 128 lanes per row x 2 rows per "
        "workgroup, 4 columns per lane, 32256 groups, grid 2048 x 256 lanes, 18448 bytes of LDS; chunk 16 frames, 4032 runs of 16 frames "
        "(8 groups per run), 2 accumulators per lane, 63 chunks and 4 blocks per signal, then k_welch_fft_join twice (chunks, blocks), "
        f"workspace {8 * 64 * 512 * 67} bytes")
    assert B.describe_welch_cmfft(p, 400, _seg("cmfft", n_fft=400, **big), detrend=True) == (
        "welch cmfft direct (L = 400, n_fft 400, col0 0, pad 0 constant, constant detrend), bins in order: k_welch_cmfft_direct<2>, "
        "64 signals x 998 frames = 63872 rows, complex FFT of 400 points in passes 5x5x4x4 (no split), 128 lanes per row x 2 rows per "
        "workgroup, 4 columns per lane, 32256 groups, grid 2048 x 256 lanes, 14416 bytes of LDS, 200 twiddles; chunk 16 frames, 4032 runs of "
        "16 frames (8 groups per run), 2 accumulators per lane, 63 chunks and 4 blocks per signal, then k_welch_fft_join twice (chunks, "
        f"blocks), workspace {8 * 64 * 400 * 67} bytes")
    assert B.describe_welch_cfft(p, 400, _seg("cfft", frames=0)) == "welch cfft direct (L = 400, n_fft 512, no detrending), bins in order: nothing (frames 0)"
    assert B.describe_welch_cmfft(p, 400, _seg("cmfft", frames=0)) == "welch cmfft direct (L = 400, n_fft 600, no detrending), bins in order: nothing (frames 0)"


def test_python_surface_and_signatures():
    names = ("hold_fft_iq", "hold_fft_iq_mixed", "hold_fused_iq", "hold_fused_iq_mixed", "describe_hold_cfft", "describe_hold_cmfft",
             "hold_cfft_workspace_bytes", "hold_cmfft_workspace_bytes")
    for name in names:
        assert name in bhw.__all__ and hasattr(bhw, name), name
    for name in names[4:]:
        assert getattr(B, name) is getattr(bhw, name)
    assert inspect.signature(B.describe_hold_cfft) == inspect.signature(B.describe_hold_cmfft)
    assert list(inspect.signature(B.describe_hold_cfft).parameters) == ["params", "length", "stft", "detrend", "fftshift", "traces", "table"]
    sig = inspect.signature(bhw.hold_fft_iq)
    assert str(sig) == ("(params, x, n_fft, hop, scale=1.0, *, win_length=None, center=False, pad_mode='reflect', detrend=False, shift=None, "
                        "fftshift=False, traces='both', out_max=None, out_min=None, workspace=None)")
    assert inspect.signature(bhw.hold_fft_iq_mixed) == sig
    fsig = inspect.signature(bhw.hold_fused_iq)
    assert str(fsig) == ("(params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend='constant', scaling='density', shift=None, "
                         "fftshift=False, traces='both', out_max=None, out_min=None, workspace=None)")
    assert inspect.signature(bhw.hold_fused_iq_mixed) == fsig
    for name, want in (("hold_fft_iq", sig), ("hold_fft_iq_mixed", sig), ("hold_fused_iq", fsig), ("hold_fused_iq_mixed", fsig)):
        got = inspect.signature(getattr(bhw.ResidentTable, name))
        assert list(got.parameters)[1:] == list(want.parameters), name
        assert [q.default for q in got.parameters.values()][1:] == [q.default for q in want.parameters.values()], name
        assert [q.kind for q in got.parameters.values()][1:] == [q.kind for q in want.parameters.values()], name
    # the arguments are the Welch siblings' but for the outputs and the default of scale
    for new, old in (("hold_fft_iq", "welch_fft_iq"), ("hold_fft_iq_mixed", "welch_fft_iq_mixed"), ("hold_fused_iq", "welch_fused_iq"),
                     ("hold_fused_iq_mixed", "welch_fused_iq_mixed")):
        a, b = list(inspect.signature(getattr(bhw, new)).parameters), list(inspect.signature(getattr(bhw, old)).parameters)
        assert [q for q in a if q not in ("traces", "out_max", "out_min")] == [q for q in b if q != "out"], new
    # existing signatures do not change
    assert list(inspect.signature(bhw.welch_fft_iq).parameters) == ["params", "x", "n_fft", "hop", "scale", "win_length", "center", "pad_mode",
                                                                   "detrend", "shift", "fftshift", "out", "workspace"]
    assert list(inspect.signature(bhw.welch_fused_iq_mixed).parameters) == ["params", "x", "fs", "length", "noverlap", "nfft", "detrend", "scaling",
                                                                           "shift", "fftshift", "out", "workspace"]


def test_every_value_error_is_raised_before_the_device_is_looked_at():
    """On CPU tensors, with no GPU: the fronts hand their arguments to the Welch siblings' two functions, whose checks -- and the check
    of `traces` before them -- raise before any device call.  (The public names look for a HIP device first, as every front does.)"""
    torch = pytest.importorskip("torch")
    from blackman_harris_win_amd import selector
    p = B.make_params(B.WIN_BH4, 24, 32)
    z = torch.zeros(4000, dtype=torch.complex64)

    def fft(x, n, fam, hold, scale=1.0):
        return selector._welch_cfft_psd(torch, p, x, n, 160, scale, None, False, "reflect", False, None, False, None, None, 0, None, fam, hold)

    def fused(x, n, fam, hold, **kw):
        a = dict(noverlap=None, detrend="constant", scaling="density")
        a.update(kw)
        return selector._welch_fused_iq(torch, p, x, 1.0, 400, a["noverlap"], n, a["detrend"], a["scaling"], None, False, None, None, 0, None,
                                        {}, fam, hold)

    both = ("both", None, None)
    for fam, n in (("cfft", 512), ("cmfft", 600)):
        for bad in ("median", None, "MAX", 3):
            with pytest.raises(ValueError, match="traces must be 'both', 'max' or 'min'"):
                fft(z, n, fam, (bad, None, None))
            with pytest.raises(ValueError, match="traces must be 'both', 'max' or 'min'"):
                fused(z, n, fam, (bad, None, None))
        for x, size in ((z.real, n), (z.to(torch.complex128), n), (z, 448), (z, 2160), (z, n)):     # the last: a CPU tensor
            words = []
            for hold in (both, None):                                # the hold call and the Welch sibling: the same words
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
    with pytest.raises(ValueError, match="n_fft 512 is a power of two: welch_fft_iq / welch_fused_iq transform it"):
        fft(z, 512, "cmfft", both)
    with pytest.raises(ValueError):
        fft(z, 600, "cfft", both)
    # the fronts pass these two functions their arguments and nothing else
    src = inspect.getsource(selector.hold_fft_iq) + inspect.getsource(selector.hold_fft_iq_mixed)
    assert src.count("return _welch_cfft_psd(") == 2 and "(traces, out_max, out_min)" in src
    src = inspect.getsource(selector.hold_fused_iq) + inspect.getsource(selector.hold_fused_iq_mixed)
    assert src.count("return _welch_fused_iq(") == 2 and "_SUMS_CACHE" in src
