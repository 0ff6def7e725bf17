"""The fused STFT + mask + inverse STFT calls (bhw_mask_fft_f32_device / _from_table / bhw_describe_mask_fft): the checks that need no
GPU -- exports and declarations, every refusal of include/bhw.h before any HIP call, the parents' refusals in the parents' own words,
the rules that tie the two descriptors, the gain strides, the overlaps, samples 0, and the Python surface."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from blackman_harris_win_amd import selector as S

import mask_fft_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED, HIP = 0, -1, -2, -3
NEW_SYMBOLS = ("bhw_mask_fft_f32_device", "bhw_mask_fft_f32_from_table", "bhw_describe_mask_fft")
# never dereferenced: every call below fails or has nothing to do
X, G, O = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x40000000), ctypes.c_void_p(0x80000000)
K, F, NB, T = 257, 101, 4, 16000


def _err():
    return B.lib().bhw_last_error().decode()


def _desc(analysis, **kw):
    """4 signals of 16000 samples, 101 frames of 512 at hop 160, window 400, centred; the analysis side padded by reflection."""
    a = dict(batch=NB, samples=T, frames=F, hop=160, n_fft=512, col0=56, pad=256, shift=31)
    if analysis:
        a["pad_mode"] = B.PAD_REFLECT
    a.update(kw)
    size = a.pop("struct_size", None)
    s = B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)
    if size is not None:
        s.struct_size = size
    return s


def _ref(s):
    return ctypes.byref(s) if s is not None else None


def _calls(sa, ss, flags=1, L=400, x=X, g=G, out=O, gs=K, gbs=F * K):
    lib = B.lib()
    return (lambda p: lib.bhw_mask_fft_f32_device(p, L, 0, None, _ref(sa), _ref(ss), flags, x, g, gs, gbs, out),
            lambda p: lib.bhw_mask_fft_f32_from_table(None, p, L, None, _ref(sa), _ref(ss), flags, x, g, gs, gbs, out))


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert L.bhw_abi_version() == 4 and ctypes.sizeof(B.BhwStft) == 96
    assert "WORD FOR WORD" in header and "one float32 rounding per part" in header
    assert L.bhw_mask_fft_f32_from_table.argtypes[1:3] + L.bhw_mask_fft_f32_from_table.argtypes[4:] == \
        L.bhw_mask_fft_f32_device.argtypes[:2] + L.bhw_mask_fft_f32_device.argtypes[4:]


def test_the_parents_refusals_come_back_in_the_parents_words():
    """The same bad descriptor through bhw_stft_fft_f32_device (analysis side) or bhw_istft_fft_f32_device (synthesis side) and through
    the mask call, both sides given the same bad field where they must agree: the code and the whole message."""
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    lib = B.lib()
    analysis = [dict(struct_size=8), dict(channels=3), dict(batch=0), dict(hop=0), dict(n_fft=0), dict(n_fft=256), dict(n_fft=8192),
                dict(n_fft=22, col0=0, pad=11), dict(shift=63), dict(pad_mode=2), dict(samples=0), dict(frames=102), dict(x_stride=T - 1),
                dict(pad=T, frames=1), dict(batch=1 << 20)]
    for kw in analysis:
        sa = _desc(True, **kw)
        both = {k: v for k, v in kw.items() if k in ("batch", "frames", "hop", "n_fft", "col0", "shift", "channels")}
        ss = _desc(False, **both)
        L = 16 if kw.get("n_fft") == 22 else 400
        rc = lib.bhw_stft_fft_f32_device(ref, L, 0, None, ctypes.byref(sa), 0, X, O)
        want = _err()
        assert rc in (BADARG, UNSUPPORTED), (kw, rc)
        for call in _calls(sa, ss, L=L):
            assert call(ref) == rc and _err() == want, (kw, want, _err())
    synthesis = [dict(struct_size=8), dict(pad=55), dict(pad_mode=B.PAD_REFLECT), dict(samples=(1 << 34) + 1), dict(x_stride=T - 1)]
    for kw in synthesis:
        ss = _desc(False, **kw)
        rc = lib.bhw_istft_fft_f32_device(ref, 400, 0, None, ctypes.byref(ss), 1, G, O)
        want = _err()
        assert rc == BADARG, (kw, rc)
        for call in _calls(_desc(True), ss):
            assert call(ref) == rc and _err() == want, (kw, want, _err())
    # frames 0 on both sides with samples to write: the inverse call's refusal (the forward call has nothing to do at frames 0)
    ss = _desc(False, frames=0)
    assert lib.bhw_istft_fft_f32_device(ref, 400, 0, None, ctypes.byref(ss), 1, G, O) == BADARG
    want = _err()
    for call in _calls(_desc(True, frames=0), ss):
        assert call(ref) == BADARG and _err() == want and "frames is 0 with samples" in want


def test_refusals_that_name_the_route_that_takes_the_input():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    cases = [
        (dict(n_fft=4096, col0=0, pad=2048), 4096, ("bhw_stft_fft_f32_*", "bhw_istft_fft_f32_*")),
        (dict(n_fft=400, col0=0, pad=200), 400, ("bhw_stft_mfft_f32_*", "bhw_istft_mfft_f32_*")),
        (dict(n_fft=1000, col0=300, pad=500), 400, ("bhw_stft_mfft_f32_*", "bhw_istft_mfft_f32_*")),
        (dict(channels=2), 400, ("bhw_stft_cfft_f32_*", "bhw_istft_cfft_f32_*")),
    ]
    for kw, L, names in cases:
        for sa, ss in ((_desc(True, **kw), _desc(False, **kw)), (_desc(True, **kw), _desc(False)), (_desc(True), _desc(False, **kw))):
            for call in _calls(sa, ss, L=L):
                assert call(ref) == UNSUPPORTED and all(n in _err() for n in names), (kw, _err())
            buf = ctypes.create_string_buffer(1280)
            assert B.lib().bhw_describe_mask_fft(None, ref, L, ctypes.byref(sa), ctypes.byref(ss), 1, K, F * K, buf, 1280) == UNSUPPORTED


def test_the_descriptors_must_agree_and_have_no_row_strides():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    differ = [("batch", dict(batch=5)), ("frames", dict(frames=100)), ("hop", dict(hop=161)), ("n_fft", dict(n_fft=1024, pad=512)),
              ("col0", dict(col0=50)), ("shift", dict(shift=30))]
    for field, kw in differ:
        for call in _calls(_desc(True), _desc(False, **kw)):
            assert call(ref) == BADARG and _err().startswith(field + ":") and "must agree" in _err(), (field, _err())
    for kw, side in ((dict(y_stride=514), "analysis"), (dict(y_batch_stride=F * 514), "analysis")):
        for call in _calls(_desc(True, **kw), _desc(False)):
            assert call(ref) == BADARG and "no spectrum rows" in _err() and side in _err(), _err()
    for kw in (dict(y_stride=514), dict(y_batch_stride=F * 514)):
        for call in _calls(_desc(True), _desc(False, **kw)):
            assert call(ref) == BADARG and "no spectrum rows" in _err() and "synthesis" in _err(), _err()


def test_argument_gain_stride_and_overlap_errors():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    sa, ss = _desc(True), _desc(False)
    for flags in (2, 4, 3, 1 << 31):                                     # 0 or BHW_OLA_NORMALIZE: no detrending, no foreign bit
        for call in _calls(sa, ss, flags=flags):
            assert call(ref) == BADARG and "flags" in _err()
    for call in _calls(None, ss) + _calls(sa, None):
        assert call(ref) == BADARG and "descriptor is NULL" in _err()
    for call in _calls(sa, ss):
        assert call(None) == BADARG
    for call in _calls(sa, ss, L=0):
        assert call(ref) == BADARG and "length" in _err()
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    for call in _calls(sa, ss):
        assert call(ctypes.byref(taylor)) == UNSUPPORTED
    # the gain strides: 0 or at least K; 0 or at least (frames - 1) * g_stride + K
    for gs, gbs, text in ((K - 1, F * K, "g_stride 256"), (1, 0, "g_stride 1"), (K, (F - 1) * K + K - 1, "g_batch_stride"), (0, K - 1, "g_batch_stride"),
                          (K + 7, (F - 1) * (K + 7) + K - 1, "g_batch_stride")):
        for call in _calls(sa, ss, gs=gs, gbs=gbs):
            assert call(ref) == BADARG and text in _err(), (gs, gbs, _err())
        with pytest.raises(B.BhwError, match=text):
            B.describe_mask_fft(p, 400, sa, ss, g_stride=gs, g_batch_stride=gbs)
    for gs, gbs in ((0, 0), (K, 0), (0, K), (K, F * K), (K + 7, (F - 1) * (K + 7) + K)):
        assert B.lib().bhw_mask_fft_f32_from_table(None, ref, 400, None, ctypes.byref(sa), ctypes.byref(ss), 1, X, G, gs, gbs, O) == BADARG
        assert "table is NULL" in _err(), (gs, gbs, _err())
    # the pointers
    for kw in (dict(x=None), dict(g=None), dict(out=None)):
        for call in _calls(sa, ss, **kw):
            assert call(ref) == BADARG and "NULL" in _err()
    for kw, name in ((dict(x=ctypes.c_void_p(0x10000002)), "d_x"), (dict(g=ctypes.c_void_p(0x40000001)), "d_g"),
                     (dict(out=ctypes.c_void_p(0x80000003)), "d_out")):
        for call in _calls(sa, ss, **kw):
            assert call(ref) == BADARG and name + " is not 4-byte aligned" in _err()
    # d_out against d_x and against d_g: inside, and the first byte behind each.  x and out hold 4 * 16000 floats, g 4 * 101 * 257
    xb, gb = NB * T * 4, NB * F * K * 4
    lib = B.lib()
    for x, g, out, bad in ((0x10000000, 0x40000000, 0x10000000 + xb - 4, "d_x and d_out"), (0x10000000, 0x40000000, 0x10000000 + xb, None),
                           (0x10000000 + xb - 4, 0x40000000, 0x10000000, "d_x and d_out"), (0x10000000, 0x40000000, 0x10000000, "d_x and d_out"),
                           (0x10000000, 0x40000000, 0x40000000 + gb - 4, "d_g and d_out"), (0x10000000, 0x40000000, 0x40000000 + gb, None),
                           (0x10000000, 0x80000000 + xb - 4, 0x80000000, "d_g and d_out"), (0x10000000, 0x10000000, 0x80000000, None)):
        rc = lib.bhw_mask_fft_f32_from_table(None, ref, 400, None, ctypes.byref(sa), ctypes.byref(ss), 1, ctypes.c_void_p(x),
                                             ctypes.c_void_p(g), K, F * K, ctypes.c_void_p(out))
        assert rc == BADARG and (bad + " overlap" if bad else "table is NULL") in _err(), (hex(x), hex(g), hex(out), _err())
        if bad:
            assert lib.bhw_mask_fft_f32_device(ref, 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), 1, ctypes.c_void_p(x), ctypes.c_void_p(g),
                                               K, F * K, ctypes.c_void_p(out)) == BADARG
    # a broadcast gain row is K floats however many signals there are: out right behind it does not overlap
    rc = lib.bhw_mask_fft_f32_from_table(None, ref, 400, None, ctypes.byref(sa), ctypes.byref(ss), 1, X, G, 0, 0,
                                         ctypes.c_void_p(0x40000000 + K * 4))
    assert rc == BADARG and "table is NULL" in _err()


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1280)
    for n in range(1, 4200):
        sa = B.make_stft(2, 10000, 3, 7, n, pad=n // 2, pad_mode=0, shift=31)
        ss = B.make_stft(2, 1000, 3, 7, n, pad=n // 2, shift=31)
        rc = lib.bhw_describe_mask_fft(None, ctypes.byref(p), min(n, 16), ctypes.byref(sa), ctypes.byref(ss), 1, 0, 0, buf, 1280)
        assert rc == (OK if B.mask_fft_supported(n) else UNSUPPORTED), (n, rc, _err())
        assert B.mask_fft_supported(n) == (n in (16, 32, 64, 128, 256, 512, 1024, 2048))


def test_samples_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    for flags in (0, 1):
        sa, ss = _desc(True), _desc(False, samples=0)
        assert B.lib().bhw_mask_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), flags, None, None, 3, 5, None) == OK
        assert "nothing (samples 0)" in B.describe_mask_fft(p, 400, sa, ss, normalize=bool(flags))
        sa, ss = _desc(True, frames=0), _desc(False, samples=0, frames=0)
        assert B.lib().bhw_mask_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), flags, None, None, 0, 0, None) == OK


def test_compute_entry_point_fails_loudly_without_a_gpu():
    """No CPU fallback: with every check passed and no HIP device the library call returns BHW_ERR_HIP."""
    import torch
    if torch.cuda.is_available():
        return
    p = B.make_params(B.WIN_BH7, 16, 32)
    sa, ss = _desc(True), _desc(False)
    rc = B.lib().bhw_mask_fft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), 1, X, G, K, F * K, O)
    assert rc == HIP, (rc, _err())
    with pytest.raises(RuntimeError):
        bhw.stft_mask_istft(p, torch.zeros(1000), torch.ones(257), 512, 160)


def test_describe_line_parses_and_names_the_gain_layout():
    p = B.make_params(B.WIN_BH7, 16, 32)
    sa, ss = _desc(True, batch=64, samples=159520, frames=998), _desc(False, batch=64, samples=159520, frames=998)
    d = MC.parse(B.describe_mask_fft(p, 400, sa, ss, normalize=True, g_stride=K, g_batch_stride=998 * K))
    assert (d["signals"], d["frames"], d["n_fft"], d["L"], d["fy"], d["lds"]) == (64, 998, 512, 400, 4, 22528)
    assert d["both_ffts"] and d["pad_mode"] == "reflect" and d["T_in"] == 159520 and d["kernels"] == {"k_mask_fft_direct": ("2",)}
    assert (d["g_stride"], d["g_batch_stride"]) == (K, 998 * K)
    line = B.describe_mask_fft(p, 400, sa, ss)
    assert "one gain row for every frame and every signal" in line and "not normalised" in line
    assert "one gain row for every frame, g_batch_stride 257" in B.describe_mask_fft(p, 400, sa, ss, g_batch_stride=K)
    assert "g_stride 257, one set of gain rows for every signal" in B.describe_mask_fft(p, 400, sa, ss, g_stride=K)
    assert "pad 256 constant" in B.describe_mask_fft(p, 400, _desc(True, batch=64, samples=159520, frames=998, pad_mode=0), ss)


def test_python_surface():
    assert "stft_mask_istft" in bhw.__all__ and "describe_mask_fft" in bhw.__all__
    sig = inspect.signature(bhw.stft_mask_istft)
    assert list(sig.parameters) == ["params", "x", "mask", "n_fft", "hop", "win_length", "center", "pad_mode", "length", "normalize", "shift",
                                    "out", "table"]
    for name in ("win_length", "center", "pad_mode", "length", "normalize", "shift", "out", "table"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert not hasattr(bhw.ResidentTable, "stft_mask_istft")
    doc = bhw.stft_mask_istft.__doc__
    assert "BIT FOR BIT" in doc and "expand()" in doc and "stft_mixed" in doc and "stft_iq" in doc


def test_python_refusals_name_the_routes_and_need_no_device():
    """The refusals come before anything looks at a device: the helper the public function starts with, on host tensors."""
    import torch
    x, m = torch.zeros(2, 1000), torch.ones(257)
    for args, text in (((x, m.to(torch.complex64), 512), r"bhw\.stft, a complex multiply and bhw\.istft"),
                       ((x, torch.ones(201), 400), r"bhw\.stft_mixed, a multiply and bhw\.istft_mixed"),
                       ((x.to(torch.complex64), m, 512), r"bhw\.stft_iq, a multiply and bhw\.istft_iq"),
                       ((torch.zeros(2, 9000), torch.ones(2049), 4096), r"got 4096 \(bhw\.stft, a multiply and bhw\.istft take it\)")):
        with pytest.raises(ValueError, match=text):
            S._mask_fft_refusals(torch, *args)
    S._mask_fft_refusals(torch, x, m, 512)
    # the gains: layouts and strides, on host tensors up to the device check
    with pytest.raises(ValueError, match="float32 CUDA tensor"):
        S._mask_gains(torch, m, 2, 7, 257, 0)
