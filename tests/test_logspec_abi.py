"""The fused log spectrogram / MFCC calls (bhw_logspec_f32_*, bhw_logspec_mfft_f32_*, bhw_describe_logspec, bhw_describe_logspec_mfft):
the checks that need no GPU -- exports and declarations, every refusal of include/bhw.h before any HIP call and in its order, for both
families and both forms, frames 0, the describe line and the Python surface."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import logspec_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED = 0, -1, -2
NEW_SYMBOLS = ("bhw_logspec_f32_device", "bhw_logspec_f32_from_table", "bhw_describe_logspec",
               "bhw_logspec_mfft_f32_device", "bhw_logspec_mfft_f32_from_table", "bhw_describe_logspec_mfft")
# never dereferenced: every call below fails or has nothing to do
A, Z = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000)
FIRST, OFFSET, WEIGHT, DCT = 0x20000000, 0x20100000, 0x20200000, 0x20300000
FAMILIES = {"pow2": dict(n_fft=512, stem="bhw_logspec", other=400, other_name="bhw_logspec_mfft_f32"),
            "mixed": dict(n_fft=400, stem="bhw_logspec_mfft", other=512, other_name="bhw_logspec_f32")}


def _err():
    return B.lib().bhw_last_error().decode()


def _seg(fam, **kw):
    """Welch framing: 4 signals of 16000, window 400 in rows of n_fft, hop 160, no padding: 98 frames."""
    a = dict(batch=4, samples=16000, frames=98, hop=160, n_fft=FAMILIES[fam]["n_fft"], shift=31)
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _bank(fam, **kw):
    a = dict(filters=80, bins=FAMILIES[fam]["n_fft"] // 2 + 1, weights=1000, d_first=FIRST, d_offset=OFFSET, d_weight=WEIGHT)
    a.update(kw)
    fb = B.make_fbank(a["filters"], a["bins"], a["weights"], a["d_first"], a["d_offset"], a["d_weight"])
    fb.reserved = a.get("reserved", 0)
    if "struct_size" in a:
        fb.struct_size = a["struct_size"]
    return fb


def _ls(**kw):
    a = dict(floor=1e-10, mult=1.0, add=False, coeffs=0, dct_rows=0, d_dct=None)
    a.update(kw)
    ls = B.make_logspec(a["floor"], a["mult"], add=a["add"], coeffs=a["coeffs"], dct_rows=a["dct_rows"], d_dct=a["d_dct"])
    ls.reserved = a.get("reserved", 0)
    if "struct_size" in a:
        ls.struct_size = a["struct_size"]
    if "mode" in a:
        ls.mode = a["mode"]
    return ls


def _mfcc(**kw):
    a = dict(coeffs=13, dct_rows=80, d_dct=DCT)
    a.update(kw)
    return _ls(**a)


def _calls(fam, s, fb, ls, flags=1, L=400, x=A, out=Z):
    lib, stem = B.lib(), FAMILIES[fam]["stem"]
    sr = ctypes.byref(s) if s is not None else None
    fr = ctypes.byref(fb) if fb is not None else None
    lr = ctypes.byref(ls) if ls is not None else None
    return (lambda p: getattr(lib, stem + "_f32_device")(p, L, 0, None, sr, flags, fr, lr, x, out),
            lambda p: getattr(lib, stem + "_f32_from_table")(None, p, L, None, sr, flags, fr, lr, x, out))


def _passes(fam, ref, s, fb, ls, flags=1, L=400, x=A, out=Z):
    """Every check passed: the from-table call with no table stops at 'table is NULL', before any launch."""
    rc = _calls(fam, s, fb, ls, flags, L, x, out)[1](ref)
    return rc == BADARG and "table is NULL" in _err()


def _refused(fam, ref, code, text, s, fb, ls, **kw):
    for call in _calls(fam, s, fb, ls, **kw):
        assert call(ref) == code and text in _err(), (fam, text, _err())
    return True


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert L.bhw_abi_version() == 4 and ctypes.sizeof(B.BhwLogspec) == 48 and "} bhw_logspec;" in header
    assert "#define BHW_LOG_CLAMP 0u" in header and "#define BHW_LOG_ADD 1u" in header and (B.LOG_CLAMP, B.LOG_ADD) == (0, 1)
    assert "A wrong bank or matrix gives wrong numbers, never a stray access" in header
    for word in ("Not built", "magnitude", "log", "complex input", "top_db", "liftering", "a DCT without a bank"):
        assert word in header


@pytest.mark.parametrize("fam", FAMILIES)
def test_input_side_errors_are_the_parents(fam):
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    n = FAMILIES[fam]["n_fft"]
    cases = [
        (dict(struct_size=8), BADARG, "struct_size"),
        (dict(channels=3), BADARG, "channels"),
        (dict(channels=2), UNSUPPORTED, "real input"),
        (dict(batch=0), BADARG, "batch is 0"),
        (dict(hop=0), BADARG, "hop is 0"),
        (dict(n_fft=0), BADARG, "n_fft"),
        (dict(n_fft=256), BADARG, "col0 + L"),
        (dict(n_fft=FAMILIES[fam]["other"]), UNSUPPORTED, FAMILIES[fam]["other_name"]),
        (dict(n_fft=8192), UNSUPPORTED, "n_fft 8192"),
        (dict(n_fft=442), UNSUPPORTED, "n_fft 442"),
        (dict(shift=63), BADARG, "shift"),
        (dict(frames=99), BADARG, "segment 98 leaves the signal"),
        (dict(samples=0), BADARG, "samples is 0"),
        (dict(x_stride=15999), BADARG, "x_stride"),
    ]
    for fb, ls in ((None, _ls()), (_bank(fam), _ls()), (_bank(fam), _mfcc()), (None, None)):
        for flags in (0, 1):
            for kw, code, text in cases:
                s = _seg(fam, **{k: v for k, v in kw.items() if k != "struct_size"})
                if "struct_size" in kw:
                    s.struct_size = kw["struct_size"]
                assert _refused(fam, ref, code, text, s, fb, ls, flags=flags)
            if ls is not None:
                assert _passes(fam, ref, _seg(fam), fb, ls, flags=flags), _err()
        for flags in (2, 3, 4):                                      # BHW_MFFT_POWER is not a flag here
            assert _refused(fam, ref, BADARG, "flags", _seg(fam), fb, ls, flags=flags)
        assert _refused(fam, ref, BADARG, "descriptor is NULL", None, fb, ls)
        for call in _calls(fam, _seg(fam), fb, ls):
            assert call(None) == BADARG
        assert _refused(fam, ref, BADARG, "length", _seg(fam), fb, ls, L=0)
    # the fields of fb, in the parent's words, before anything of ls
    for kw, text in ((dict(struct_size=40), "bhw_fbank.struct_size"), (dict(reserved=1), "bhw_fbank.reserved"), (dict(filters=0), "bhw_fbank.filters"),
                     (dict(filters=4097), "bhw_fbank.filters"), (dict(bins=n // 2), "bhw_fbank.bins"), (dict(weights=(1 << 24) + 1), "bhw_fbank.weights")):
        assert _refused(fam, ref, BADARG, text, _seg(fam), _bank(fam, **kw), None)


@pytest.mark.parametrize("fam", FAMILIES)
def test_log_descriptor_errors_in_order(fam):
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    n = FAMILIES[fam]["n_fft"]
    s, fb = _seg(fam), _bank(fam)
    # each entry fails at its own check although every LATER check would fail too
    later = dict(floor=-1.0, mult=0.0, coeffs=5000)
    chain = [
        (None, "log descriptor is NULL"),
        (dict(struct_size=40, reserved=1, mode=7, **later), "bhw_logspec.struct_size"),
        (dict(reserved=1, mode=7, **later), "bhw_logspec.reserved"),
        (dict(mode=2, **later), "bhw_logspec.mode"),
        (dict(floor=0.0, mult=0.0, coeffs=5000), "bhw_logspec.floor"),
        (dict(floor=-1e-3, mult=0.0), "bhw_logspec.floor"),
        (dict(floor=math.inf, mult=0.0), "bhw_logspec.floor"),
        (dict(floor=math.nan, mult=0.0), "bhw_logspec.floor"),
        (dict(mult=0.0, coeffs=5000), "bhw_logspec.mult"),
        (dict(mult=math.inf, coeffs=5000), "bhw_logspec.mult"),
        (dict(mult=math.nan, coeffs=5000), "bhw_logspec.mult"),
        (dict(coeffs=4097, dct_rows=3), "bhw_logspec.coeffs 4097 above 4096"),
    ]
    for kw, text in chain:
        for bank in (fb, None):
            assert _refused(fam, ref, BADARG, text, s, bank, None if kw is None else _ls(**kw))
    assert _refused(fam, ref, BADARG, "without a filter bank", s, None, _mfcc(dct_rows=81, d_dct=None))
    assert _refused(fam, ref, BADARG, "bhw_logspec.dct_rows 81", s, _bank(fam, filters=n + 1), _mfcc(dct_rows=81, coeffs=4096, d_dct=None))
    assert _refused(fam, ref, BADARG, "above n_fft", s, _bank(fam, filters=n + 1), _mfcc(dct_rows=n + 1, d_dct=None))
    assert _passes(fam, ref, s, _bank(fam, filters=n), _mfcc(dct_rows=n)), _err()
    # dct_rows * coeffs above 2^24 cannot be reached while filters and coeffs are both capped at 4096 = 2^12: the largest matrix passes
    # that check and stops at the one before it here (4096 filters above this n_fft)
    assert _refused(fam, ref, BADARG, "above n_fft", s, _bank(fam, filters=4096), _mfcc(dct_rows=4096, coeffs=4096, d_dct=None))
    # the pointers of the matrix come last, behind those of the bank
    assert _refused(fam, ref, BADARG, "d_first / d_offset is NULL", s, _bank(fam, d_first=None), _mfcc(d_dct=None))
    assert _refused(fam, ref, BADARG, "bhw_logspec.d_dct is NULL", s, fb, _mfcc(d_dct=None))
    assert _refused(fam, ref, BADARG, "bhw_logspec.d_dct is not 4-byte aligned", s, fb, _mfcc(d_dct=DCT + 2))
    ob = 4 * 98 * 13 * 4                                              # the bytes of the output at 0x80000000
    assert _refused(fam, ref, BADARG, "d_dct and d_out overlap", s, fb, _mfcc(d_dct=0x80000000 + ob - 4))
    assert _refused(fam, ref, BADARG, "d_dct and d_out overlap", s, fb, _mfcc(d_dct=0x80000000 - 80 * 13 * 4 + 4))
    assert _passes(fam, ref, s, fb, _mfcc(d_dct=0x80000000 + ob)) and _passes(fam, ref, s, fb, _mfcc(d_dct=0x80000000 - 80 * 13 * 4))
    assert _refused(fam, ref, BADARG, "d_dct and bhw_fbank.d_weight overlap", s, fb, _mfcc(d_dct=WEIGHT + 4000 - 4))
    assert _refused(fam, ref, BADARG, "d_dct and bhw_fbank.d_first overlap", s, fb, _mfcc(d_dct=FIRST - 80 * 13 * 4 + 4))
    assert _refused(fam, ref, BADARG, "d_dct and bhw_fbank.d_offset overlap", s, fb, _mfcc(d_dct=OFFSET + 80 * 4))
    assert _passes(fam, ref, s, fb, _mfcc(d_dct=WEIGHT + 4000)) and _passes(fam, ref, s, fb, _mfcc(d_dct=OFFSET + 81 * 4))
    # without a DCT the matrix fields are not looked at; both modes, any sign of mult
    for ls in (_ls(), _ls(add=True, mult=-3.5, floor=1e300), _ls(dct_rows=7, d_dct=3)):
        assert _passes(fam, ref, s, fb, ls) and _passes(fam, ref, s, None, ls), _err()
    # the describe call checks the fields but no pointer
    buf = ctypes.create_string_buffer(1280)
    fn = getattr(B.lib(), "bhw_describe_" + FAMILIES[fam]["stem"][4:])
    nofb = _bank(fam, d_first=None, d_offset=None, d_weight=None)
    assert fn(None, ref, 400, ctypes.byref(s), 1, ctypes.byref(nofb), ctypes.byref(_mfcc(d_dct=None)), buf, 1280) == OK, _err()
    assert fn(None, ref, 400, ctypes.byref(s), 1, ctypes.byref(nofb), ctypes.byref(_mfcc(dct_rows=79)), buf, 1280) == BADARG and "dct_rows" in _err()
    assert fn(None, ref, 400, ctypes.byref(s), 1, ctypes.byref(nofb), None, buf, 1280) == BADARG and "NULL" in _err()


@pytest.mark.parametrize("fam", FAMILIES)
def test_output_side_errors_with_the_new_w(fam):
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    K = FAMILIES[fam]["n_fft"] // 2 + 1
    for fb, ls, W in ((None, _ls(), K), (_bank(fam), _ls(add=True), 80), (_bank(fam), _mfcc(), 13), (_bank(fam), _mfcc(coeffs=1, d_dct=DCT), 1)):
        for kw, text in ((dict(y_stride=W - 1), "y_stride"), (dict(y_batch_stride=97 * W + W - 1), "y_batch_stride"),
                         (dict(y_stride=W + 3, y_batch_stride=97 * (W + 3) + W - 1), "y_batch_stride")):
            if kw.get("y_stride", 1) == 0 or kw.get("y_batch_stride", 1) == 0:
                continue                                               # 0 means packed
            assert _refused(fam, ref, BADARG, text, _seg(fam, **kw), fb, ls)
        assert _passes(fam, ref, _seg(fam, y_stride=W + 3, y_batch_stride=97 * (W + 3) + W), fb, ls)
        assert _passes(fam, ref, _seg(fam, y_stride=W, y_batch_stride=98 * W + 1), fb, ls)
        s = _seg(fam)
        assert _refused(fam, ref, BADARG, "NULL", s, fb, ls, x=None) and _refused(fam, ref, BADARG, "NULL", s, fb, ls, out=None)
        assert _refused(fam, ref, BADARG, "d_out is not 4-byte aligned", s, fb, ls, out=ctypes.c_void_p(0x80000002))
        assert _passes(fam, ref, s, fb, ls, out=ctypes.c_void_p(0x80000004))
        assert _refused(fam, ref, BADARG, "d_x is not 4-byte aligned", s, fb, ls, x=ctypes.c_void_p(0x10000002))
        xb, ob = 4 * 16000 * 4, 4 * 98 * W * 4
        for x, out, bad in ((0x10000000, 0x10000000 + xb - 4, True), (0x10000000, 0x10000000 + xb, False), (0x80000000 + ob - 4, 0x80000000, True),
                            (0x80000000 + ob, 0x80000000, False)):
            if bad:
                assert _refused(fam, ref, BADARG, "d_x and d_out overlap", s, fb, ls, x=ctypes.c_void_p(x), out=ctypes.c_void_p(out))
            else:
                assert _passes(fam, ref, s, fb, ls, x=ctypes.c_void_p(x), out=ctypes.c_void_p(out)), _err()
        if fb is not None:
            assert _refused(fam, ref, BADARG, "d_first and d_out overlap", s, _bank(fam, d_first=0x80000000 - 80 * 4 + 4), ls)
            assert _refused(fam, ref, BADARG, "d_weight and d_out overlap", s, _bank(fam, d_weight=0x80000000 + 8), ls)
    # the 2^34 cap counts the W of this call: a batch whose bank rows pass it is fine as 13 coefficients only if the parent's rows fit
    big = -(-(1 << 34) // (98 * K)) + 1
    assert _refused(fam, ref, BADARG, "2^34", _seg(fam, batch=big), None, _ls())


@pytest.mark.parametrize("fam", FAMILIES)
def test_frames_zero_is_ok_with_the_pointers_unchecked(fam):
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib, stem = B.lib(), FAMILIES[fam]["stem"]
    describe = B.describe_logspec if fam == "pow2" else B.describe_logspec_mfft
    for fb, ls in ((None, _ls()), (_bank(fam, d_first=None, d_offset=None, d_weight=None), _mfcc(d_dct=None))):
        fr = ctypes.byref(fb) if fb is not None else None
        for flags in (0, 1):
            s = _seg(fam, frames=0)
            assert getattr(lib, stem + "_f32_device")(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, fr, ctypes.byref(ls), None, None) == OK
            assert getattr(lib, stem + "_f32_from_table")(None, ctypes.byref(p), 400, None, ctypes.byref(s), flags, fr, ctypes.byref(ls), None, None) == BADARG
            assert "table is NULL" in _err()
            assert "nothing (frames 0)" in describe(p, 400, s, ls, detrend=bool(flags), fbank=fb)
            bad = _ls(floor=0.0)                                       # the descriptor is still checked
            assert getattr(lib, stem + "_f32_device")(ctypes.byref(p), 400, 0, None, ctypes.byref(s), flags, fr, ctypes.byref(bad), None, None) == BADARG


def test_every_supported_size_passes_in_one_family_only():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1280)
    ls = _ls()
    for n in list(range(1, 300)) + [400, 500, 511, 512, 513, 1000, 1024, 2048, 3000, 4000, 4050, 4095, 4096, 4097, 8192]:
        s = B.make_stft(2, 100000, 3, 7, n, shift=31)
        a = lib.bhw_describe_logspec(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), 1, None, ctypes.byref(ls), buf, 1280)
        ea = _err()
        b = lib.bhw_describe_logspec_mfft(None, ctypes.byref(p), min(n, 16), ctypes.byref(s), 1, None, ctypes.byref(ls), buf, 1280)
        eb = _err()
        assert a == (OK if B.fft_supported(n) else UNSUPPORTED), (n, a, ea)
        assert b == (OK if B.mfft_supported(n) else UNSUPPORTED), (n, b, eb)
        if B.mfft_supported(n):
            assert "bhw_logspec_mfft_f32_*" in ea
        if B.fft_supported(n):
            assert "bhw_logspec_f32_*" in eb


def test_describe_line_parses():
    p = B.make_params(B.WIN_BH7, 16, 32)
    s = _seg("pow2", batch=64, samples=160000, frames=998)
    d = LC.parse(B.describe_logspec(p, 400, s, _ls(mult=10 / math.log(10)), detrend=True))
    assert d["line"].startswith("logspec direct (L = 400, n_fft 512, col0 0, pad 0 constant, constant detrend), power rows, log clamp floor 1e-10, "
                                "mult 4.3429448190325175, W = 257: k_logspec_direct<2>, 64 signals x 998 frames = 63872 rows, ")
    assert (d["lpf"], d["fy"], d["cpl"], d["groups"], d["grid"], d["lds"]) == (64, 4, 8, 15968, 2048, 2 * 4 * 256 * 8 + 256 * 8 + 16)
    s = _seg("mixed", batch=64, samples=160000, frames=998)
    d = LC.parse(B.describe_logspec_mfft(p, 400, s, _mfcc(add=True, floor=1e-6, d_dct=None), fbank=_bank("mixed")))
    assert d["line"].startswith("logspec mfft direct (L = 400, n_fft 400, col0 0, pad 0 constant, no detrending), bank rows (80 filters, 1000 weights), "
                                "log add floor 1e-06, mult 1, DCT 80 x 13, W = 13: k_logspec_mfft_direct<2>, 64 signals x 998 frames")
    assert (d["schedule"], d["dct"], d["W"], d["mode"]) == ("5x5x4x2", (80, 13), 13, "add")
    buf = ctypes.create_string_buffer(16)
    ls = _ls()
    assert B.lib().bhw_describe_logspec(None, ctypes.byref(p), 400, ctypes.byref(_seg("pow2")), 0, None, ctypes.byref(ls), buf, 16) == OK
    assert len(buf.value) == 15
    assert B.lib().bhw_describe_logspec(None, ctypes.byref(p), 400, ctypes.byref(_seg("pow2")), 0, None, ctypes.byref(ls), None, 0) == BADARG


def test_python_surface():
    for name in ("log_spectrogram", "log_spectrogram_mixed", "mfcc", "mfcc_mixed", "DctMatrix", "dct_weights", "describe_logspec",
                 "describe_logspec_mfft", "make_logspec"):
        assert name in bhw.__all__ and hasattr(bhw, name)
    want = ["params", "x", "n_fft", "hop", "fbank", "log", "floor", "add", "dct", "win_length", "center", "pad_mode", "detrend", "shift", "out", "table"]
    for fn in (bhw.log_spectrogram, bhw.log_spectrogram_mixed):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == want
        assert (sig.parameters["log"].default, sig.parameters["floor"].default, sig.parameters["add"].default) == ("db", 1e-10, False)
        assert sig.parameters["fbank"].default is None and sig.parameters["dct"].default is None and sig.parameters["center"].default is True
        assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for n, q in sig.parameters.items() if n not in ("params", "x", "n_fft", "hop"))
        assert sig.parameters["table"].default is None                 # the ResidentTable form: table=<a ResidentTable>
    for fn in (bhw.mfcc, bhw.mfcc_mixed):
        sig = inspect.signature(fn)
        assert sorted(sig.parameters) == sorted(want)
        assert sig.parameters["fbank"].default is inspect.Parameter.empty and sig.parameters["dct"].default is inspect.Parameter.empty
        assert sig.parameters["table"].default is None
    assert list(inspect.signature(bhw.dct_weights).parameters) == ["n_coeffs", "n_mels", "norm"]
    assert inspect.signature(bhw.dct_weights).parameters["norm"].default == "ortho"
    # the table form is a keyword, not a method: ResidentTable's methods are the fronts of tests/table_source_cases.py
    assert not any(hasattr(bhw.ResidentTable, n) for n in ("log_spectrogram", "log_spectrogram_mixed", "mfcc", "mfcc_mixed"))
    # the existing fronts keep their signatures
    assert list(inspect.signature(bhw.spectrogram).parameters) == ["params", "x", "n_fft", "hop", "win_length", "center", "pad_mode", "detrend", "fbank", "shift", "out"]


def test_python_errors_that_need_no_device():
    from blackman_harris_win_amd.selector import log_multiplier
    assert log_multiplier("ln") == 1.0 and log_multiplier("log10") == 1 / math.log(10) and log_multiplier("db") == 10 / math.log(10)
    assert log_multiplier(-2.5) == -2.5 and log_multiplier(3) == 3.0
    for bad in ("log2", 0, 0.0, math.inf, math.nan, None, True):
        with pytest.raises(ValueError, match="log must be"):
            log_multiplier(bad)
    p = B.make_params(B.WIN_HANN, 10, 16)
    for fn in (bhw.mfcc, bhw.mfcc_mixed):
        with pytest.raises(TypeError):
            fn(p, np.zeros(4000, dtype=np.float32), 64, 16)            # fbank and dct are required
        with pytest.raises(ValueError, match="fbank .* and dct"):
            fn(p, None, 64, 16, fbank=None, dct=None)
