"""The mixed-radix fused STFT + mask + inverse STFT calls (bhw_mask_mfft_f32_device / _from_table / bhw_describe_mask_mfft): the checks
that need no GPU -- exports and declarations, every refusal of include/bhw.h before any HIP call with the route it names, the parents'
refusals in the parents' own words, the rules that tie the two descriptors, the gain strides, the overlaps, samples 0, and the Python
surface with its four ValueErrors."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from blackman_harris_win_amd import selector as S

import mask_mfft_cases as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED, HIP = 0, -1, -2, -3
NEW_SYMBOLS = ("bhw_mask_mfft_f32_device", "bhw_mask_mfft_f32_from_table", "bhw_describe_mask_mfft")
# never dereferenced: every call below fails or has nothing to do
X, G, O = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x40000000), ctypes.c_void_p(0x80000000)
K, F, NB, T = 201, 101, 4, 16000


def _err():
    return B.lib().bhw_last_error().decode()


def _desc(analysis, **kw):
    """4 signals of 16000 samples, 101 frames of 400 at hop 160, window 400, centred; the analysis side padded by reflection."""
    a = dict(batch=NB, samples=T, frames=F, hop=160, n_fft=400, col0=0, pad=200, shift=31)
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
    return (lambda p: lib.bhw_mask_mfft_f32_device(p, L, 0, None, _ref(sa), _ref(ss), flags, x, g, gs, gbs, out),
            lambda p: lib.bhw_mask_mfft_f32_from_table(None, p, L, None, _ref(sa), _ref(ss), flags, x, g, gs, gbs, out))


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert L.bhw_abi_version() == 4 and ctypes.sizeof(B.BhwStft) == 96
    # the arguments of the power-of-two calls, word for word
    assert L.bhw_mask_mfft_f32_device.argtypes == L.bhw_mask_fft_f32_device.argtypes
    assert L.bhw_mask_mfft_f32_from_table.argtypes == L.bhw_mask_fft_f32_from_table.argtypes
    assert L.bhw_describe_mask_mfft.argtypes == L.bhw_describe_mask_fft.argtypes
    for name in NEW_SYMBOLS:
        new = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
        old = re.search(r"\bint " + name.replace("mfft", "fft") + r"\(([^;]*)\);", header).group(1)
        assert " ".join(new.split()) == " ".join(old.split()), name


def test_the_parents_refusals_come_back_in_the_parents_words():
    """The same bad descriptor through bhw_stft_mfft_f32_device (analysis side) or bhw_istft_mfft_f32_device (synthesis side) and
    through the mask call, both sides given the same bad field where they must agree: the code and the whole message."""
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    lib = B.lib()
    analysis = [dict(struct_size=8), dict(channels=3), dict(batch=0), dict(hop=0), dict(n_fft=0), dict(n_fft=8192), dict(n_fft=4374),
                dict(n_fft=22, col0=0, pad=11), dict(n_fft=401), dict(n_fft=14, col0=0, pad=7), dict(shift=63), dict(pad_mode=2), dict(samples=0),
                dict(frames=102), dict(x_stride=T - 1), dict(pad=T, frames=1), dict(batch=1 << 20)]
    for kw in analysis:
        sa = _desc(True, **kw)
        both = {k: v for k, v in kw.items() if k in ("batch", "frames", "hop", "n_fft", "col0", "shift", "channels")}
        ss = _desc(False, **both)
        L = 8 if kw.get("n_fft") in (22, 14) else 400
        rc = lib.bhw_stft_mfft_f32_device(ref, L, 0, None, ctypes.byref(sa), 0, None, X, O)
        want = _err()
        assert rc in (BADARG, UNSUPPORTED), (kw, rc)
        for call in _calls(sa, ss, L=L):
            assert call(ref) == rc and _err() == want, (kw, want, _err())
    synthesis = [dict(struct_size=8), dict(col0=60, pad=55), dict(col0=60, pad=260), dict(pad_mode=B.PAD_REFLECT), dict(samples=(1 << 34) + 1), dict(x_stride=T - 1)]
    for kw in synthesis:
        ss = _desc(False, **kw)
        rc = lib.bhw_istft_mfft_f32_device(ref, 400, 0, None, ctypes.byref(ss), 1, G, O)
        want = _err()
        assert rc == BADARG, (kw, rc)
        for call in _calls(_desc(True), ss):
            assert call(ref) == rc and _err() == want, (kw, want, _err())
    # frames 0 on both sides with samples to write: the inverse call's refusal (the forward call has nothing to do at frames 0)
    ss = _desc(False, frames=0)
    assert lib.bhw_istft_mfft_f32_device(ref, 400, 0, None, ctypes.byref(ss), 1, G, O) == BADARG
    want = _err()
    for call in _calls(_desc(True, frames=0), ss):
        assert call(ref) == BADARG and _err() == want and "frames is 0 with samples" in want


def test_refusals_that_name_the_route_that_takes_the_input():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    cases = [
        (dict(channels=2), 400, ("bhw_stft_cmfft_f32_*", "bhw_istft_cmfft_f32_*")),
        (dict(n_fft=16, col0=0, pad=8), 16, ("bhw_mask_fft_f32_*",)),
        (dict(n_fft=512, col0=56, pad=256), 400, ("bhw_mask_fft_f32_*",)),
        (dict(n_fft=2048, col0=0, pad=1024), 2048, ("bhw_mask_fft_f32_*",)),
        (dict(n_fft=4096, col0=0, pad=2048), 4096, ("bhw_stft_fft_f32_*", "bhw_istft_fft_f32_*")),
        (dict(n_fft=2160, col0=0, pad=1080), 2160, ("bhw_stft_mfft_f32_*", "bhw_istft_mfft_f32_*")),
        (dict(n_fft=2560, col0=0, pad=1280), 2560, ("bhw_stft_mfft_f32_*", "bhw_istft_mfft_f32_*")),
        (dict(n_fft=4050, col0=0, pad=2025), 4050, ("bhw_stft_mfft_f32_*", "bhw_istft_mfft_f32_*")),
    ]
    for kw, L, names in cases:
        for sa, ss in ((_desc(True, **kw), _desc(False, **kw)), (_desc(True, **kw), _desc(False)), (_desc(True), _desc(False, **kw))):
            for call in _calls(sa, ss, L=L):
                assert call(ref) == UNSUPPORTED and all(n in _err() for n in names), (kw, _err())
            # a route is named before the parents refuse the same input in other words
            assert "bhw_mask_fft_f32_*" in _err() or "bhw_mask_fft" not in _err()
            buf = ctypes.create_string_buffer(1280)
            assert B.lib().bhw_describe_mask_mfft(None, ref, L, ctypes.byref(sa), ctypes.byref(ss), 1, K, F * K, buf, 1280) == UNSUPPORTED
    # the power-of-two call keeps its own refusal of these sizes, in the words it had
    sa, ss = _desc(True), _desc(False)
    assert B.lib().bhw_mask_fft_f32_device(ref, 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), 1, X, G, K, F * K, O) == UNSUPPORTED
    assert "bhw_stft_mfft_f32_* + bhw_istft_mfft_f32_* take the mixed-radix lengths" in _err()


def test_the_descriptors_must_agree_and_have_no_row_strides():
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    # (the seventh field, channels, can only be 1 on both sides once the parents have passed: they agree by then)
    differ = [("batch", dict(batch=5)), ("frames", dict(frames=100)), ("hop", dict(hop=161)), ("n_fft", dict(n_fft=480, col0=40, pad=240)),
              ("col0", dict(n_fft=480, col0=40, pad=240)), ("shift", dict(shift=30))]
    for field, kw in differ:
        sa = _desc(True, n_fft=480, col0=30, pad=240) if field == "col0" else _desc(True)
        for call in _calls(sa, _desc(False, **kw)):
            assert call(ref) == BADARG and _err().startswith(field + ":") and "must agree" in _err(), (field, _err())
    for kw in (dict(y_stride=402), dict(y_batch_stride=F * 402)):
        for call in _calls(_desc(True, **kw), _desc(False)):
            assert call(ref) == BADARG and "no spectrum rows" in _err() and "analysis" in _err(), _err()
        for call in _calls(_desc(True), _desc(False, **kw)):
            assert call(ref) == BADARG and "no spectrum rows" in _err() and "synthesis" in _err(), _err()


def test_the_shared_tail_speaks_the_power_of_two_calls_words():
    """The checks after the parents are one function for both fronts: the same mistake gives the same message through either."""
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    lib = B.lib()

    def pow2(analysis, **kw):
        a = dict(n_fft=512, col0=56, pad=256)
        a.update(kw)
        return _desc(analysis, **a)

    def both(kwa, kws, gs_of, gbs_of, x=X, g=G, out=O):
        msgs = []
        for mk, call, k in ((_desc, lib.bhw_mask_mfft_f32_device, 201), (pow2, lib.bhw_mask_fft_f32_device, 257)):
            sa, ss = mk(True, **kwa), mk(False, **kws)
            rc = call(ref, 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), 1, x, g, gs_of(k), gbs_of(k), out)
            msgs.append((rc, re.sub(r"\d+", "#", _err())))
        assert msgs[0] == msgs[1] and msgs[0][0] == BADARG, msgs
        return msgs[0][1]

    full = (lambda k: k, lambda k: F * k)
    assert "must agree" in both({}, dict(hop=161), *full)
    assert "must agree" in both({}, dict(shift=30), *full)
    assert "no spectrum rows" in both(dict(y_stride=600), {}, *full)
    assert "g_stride" in both({}, {}, lambda k: k - 1, lambda k: F * k)
    assert "g_batch_stride" in both({}, {}, lambda k: 0, lambda k: k - 1)
    assert "NULL" in both({}, {}, *full, x=None)
    assert "d_g is not #-byte aligned" in both({}, {}, *full, g=ctypes.c_void_p(0x40000002))
    assert "d_x and d_out overlap" in both({}, {}, *full, out=X)
    assert "d_g and d_out overlap" in both({}, {}, *full, out=G)


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
    for gs, gbs, text in ((K - 1, F * K, "g_stride 200"), (1, 0, "g_stride 1"), (K, (F - 1) * K + K - 1, "g_batch_stride"), (0, K - 1, "g_batch_stride"),
                          (K + 7, (F - 1) * (K + 7) + K - 1, "g_batch_stride")):
        for call in _calls(sa, ss, gs=gs, gbs=gbs):
            assert call(ref) == BADARG and text in _err(), (gs, gbs, _err())
        with pytest.raises(B.BhwError, match=text):
            B.describe_mask_mfft(p, 400, sa, ss, g_stride=gs, g_batch_stride=gbs)
    for gs, gbs in ((0, 0), (K, 0), (0, K), (K, F * K), (K + 7, (F - 1) * (K + 7) + K)):
        assert B.lib().bhw_mask_mfft_f32_from_table(None, ref, 400, None, ctypes.byref(sa), ctypes.byref(ss), 1, X, G, gs, gbs, O) == BADARG
        assert "table is NULL" in _err(), (gs, gbs, _err())
    # the pointers
    for kw in (dict(x=None), dict(g=None), dict(out=None)):
        for call in _calls(sa, ss, **kw):
            assert call(ref) == BADARG and "NULL" in _err()
    for kw, name in ((dict(x=ctypes.c_void_p(0x10000002)), "d_x"), (dict(g=ctypes.c_void_p(0x40000001)), "d_g"),
                     (dict(out=ctypes.c_void_p(0x80000003)), "d_out")):
        for call in _calls(sa, ss, **kw):
            assert call(ref) == BADARG and name + " is not 4-byte aligned" in _err()
    # d_out against d_x and against d_g: inside, and the first byte behind each.  x and out hold 4 * 16000 floats, g 4 * 101 * 201
    xb, gb = NB * T * 4, NB * F * K * 4
    lib = B.lib()
    for x, g, out, bad in ((0x10000000, 0x40000000, 0x10000000 + xb - 4, "d_x and d_out"), (0x10000000, 0x40000000, 0x10000000 + xb, None),
                           (0x10000000 + xb - 4, 0x40000000, 0x10000000, "d_x and d_out"), (0x10000000, 0x40000000, 0x10000000, "d_x and d_out"),
                           (0x10000000, 0x40000000, 0x40000000 + gb - 4, "d_g and d_out"), (0x10000000, 0x40000000, 0x40000000 + gb, None),
                           (0x10000000, 0x80000000 + xb - 4, 0x80000000, "d_g and d_out"), (0x10000000, 0x10000000, 0x80000000, None)):
        rc = lib.bhw_mask_mfft_f32_from_table(None, ref, 400, None, ctypes.byref(sa), ctypes.byref(ss), 1, ctypes.c_void_p(x),
                                              ctypes.c_void_p(g), K, F * K, ctypes.c_void_p(out))
        assert rc == BADARG and (bad + " overlap" if bad else "table is NULL") in _err(), (hex(x), hex(g), hex(out), _err())
        if bad:
            assert lib.bhw_mask_mfft_f32_device(ref, 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), 1, ctypes.c_void_p(x), ctypes.c_void_p(g),
                                                K, F * K, ctypes.c_void_p(out)) == BADARG
    # a broadcast gain row is K floats however many signals there are: out right behind it does not overlap
    rc = lib.bhw_mask_mfft_f32_from_table(None, ref, 400, None, ctypes.byref(sa), ctypes.byref(ss), 1, X, G, 0, 0,
                                          ctypes.c_void_p(0x40000000 + K * 4))
    assert rc == BADARG and "table is NULL" in _err()


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    lib = B.lib()
    buf = ctypes.create_string_buffer(1280)
    took = []
    for n in range(1, 4200):
        sa = B.make_stft(2, 10000, 3, 7, n, pad=n // 2, pad_mode=0, shift=31)
        ss = B.make_stft(2, 1000, 3, 7, n, pad=n // 2, shift=31)
        rc = lib.bhw_describe_mask_mfft(None, ctypes.byref(p), min(n, 16), ctypes.byref(sa), ctypes.byref(ss), 1, 0, 0, buf, 1280)
        assert rc == (OK if B.mask_mfft_supported(n) else UNSUPPORTED), (n, rc, _err())
        if rc == OK:
            took.append(n)
    assert took == MM.SIZES and len(took) == 73


def test_samples_zero_is_ok_with_the_pointers_unchecked():
    p = B.make_params(B.WIN_BH7, 16, 32)
    for flags in (0, 1):
        sa, ss = _desc(True), _desc(False, samples=0)
        assert B.lib().bhw_mask_mfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), flags, None, None, 3, 5, None) == OK
        assert "nothing (samples 0)" in B.describe_mask_mfft(p, 400, sa, ss, normalize=bool(flags))
        sa, ss = _desc(True, frames=0), _desc(False, samples=0, frames=0)
        assert B.lib().bhw_mask_mfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), flags, None, None, 0, 0, None) == OK


def test_compute_entry_point_fails_loudly_without_a_gpu():
    """No CPU fallback: with every check passed and no HIP device the library call returns BHW_ERR_HIP."""
    import torch
    if torch.cuda.is_available():
        return
    p = B.make_params(B.WIN_BH7, 16, 32)
    sa, ss = _desc(True), _desc(False)
    rc = B.lib().bhw_mask_mfft_f32_device(ctypes.byref(p), 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), 1, X, G, K, F * K, O)
    assert rc == HIP, (rc, _err())
    with pytest.raises(RuntimeError):
        bhw.stft_mask_istft_mixed(p, torch.zeros(1000), torch.ones(201), 400, 160)


def test_describe_line_parses_and_names_the_gain_layout():
    p = B.make_params(B.WIN_BH7, 16, 32)
    sa, ss = _desc(True, batch=64, samples=159520, frames=998), _desc(False, batch=64, samples=159520, frames=998)
    d = MM.parse(B.describe_mask_mfft(p, 400, sa, ss, normalize=True, g_stride=K, g_batch_stride=998 * K))
    assert (d["signals"], d["frames"], d["n_fft"], d["L"], d["fy"], d["lds"], d["schedule"]) == (64, 998, 400, 400, 4, 17600, "5x5x4x2")
    assert d["both_ffts"] and d["pad_mode"] == "reflect" and d["T_in"] == 159520 and d["kernels"] == {"k_mask_mfft_direct": ("2",)}
    assert (d["g_stride"], d["g_batch_stride"]) == (K, 998 * K)
    line = B.describe_mask_mfft(p, 400, sa, ss)
    assert line.startswith("mask mfft direct ")
    assert "one gain row for every frame and every signal" in line and "not normalised" in line
    assert "one gain row for every frame, g_batch_stride 201" in B.describe_mask_mfft(p, 400, sa, ss, g_batch_stride=K)
    assert "g_stride 201, one set of gain rows for every signal" in B.describe_mask_mfft(p, 400, sa, ss, g_stride=K)
    assert "pad 200 constant" in B.describe_mask_mfft(p, 400, _desc(True, batch=64, samples=159520, frames=998, pad_mode=0), ss)
    # the power-of-two line keeps its words
    s2a = B.make_stft(4, 16000, 101, 160, 512, col0=56, pad=256, pad_mode=B.PAD_REFLECT, shift=31)
    s2s = B.make_stft(4, 16000, 101, 160, 512, col0=56, pad=256, shift=31)
    assert B.describe_mask_fft(p, 400, s2a, s2s).startswith("mask fft direct (L = 400, n_fft 512, col0 56, pad 256: t0 = 200; analysis of 16000 "
                                                            "samples, pad 256 reflect), not normalised: k_mask_fft_direct")


def test_python_surface():
    assert "stft_mask_istft_mixed" in bhw.__all__ and "describe_mask_mfft" in bhw.__all__
    sig = inspect.signature(bhw.stft_mask_istft_mixed)
    assert list(sig.parameters) == list(inspect.signature(bhw.stft_mask_istft).parameters)
    assert list(sig.parameters) == ["params", "x", "mask", "n_fft", "hop", "win_length", "center", "pad_mode", "length", "normalize", "shift",
                                    "out", "table"]
    for name in ("win_length", "center", "pad_mode", "length", "normalize", "shift", "out", "table"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
        assert sig.parameters[name].default == inspect.signature(bhw.stft_mask_istft).parameters[name].default
    assert not hasattr(bhw.ResidentTable, "stft_mask_istft_mixed")
    doc = bhw.stft_mask_istft_mixed.__doc__
    assert "BIT FOR BIT" in doc and "expand()" in doc and "stft_mixed" in doc and "stft_iq_mixed" in doc and "stft_mask_istft" in doc
    assert hasattr(B, "mask_mfft_supported") and hasattr(B, "describe_mask_mfft")


def test_python_refusals_name_the_routes_and_need_no_device():
    """The four ValueErrors come before anything looks at a device: the helper the public function starts with, on host tensors; and
    through the public function itself, which raises them for host tensors before it would refuse those."""
    import torch
    p = B.make_params(B.WIN_BH7, 16, 32)
    x, m = torch.zeros(2, 1000), torch.ones(201)
    cases = (((x, torch.ones(257), 512), r"bhw\.stft_mask_istft takes it"),
             ((x, torch.ones(9), 16), r"bhw\.stft_mask_istft takes it"),
             ((torch.zeros(2, 9000), torch.ones(2049), 4096), r"4096 is a power of two above 2048: bhw\.stft, a multiply and bhw\.istft take it"),
             ((torch.zeros(2, 9000), torch.ones(1281), 2560), r"bhw\.stft_mixed, a multiply and bhw\.istft_mixed take it"),
             ((torch.zeros(2, 9000), torch.ones(1081), 2160), r"bhw\.stft_mixed, a multiply and bhw\.istft_mixed take it"),
             ((x.to(torch.complex64), m, 400), r"bhw\.stft_iq_mixed, a multiply and bhw\.istft_iq_mixed"),
             ((x, m.to(torch.complex64), 400), r"bhw\.stft_mixed, a complex multiply and bhw\.istft_mixed"))
    for args, text in cases:
        with pytest.raises(ValueError, match=text):
            S._mask_mfft_refusals(torch, *args)
        with pytest.raises(ValueError, match=text):
            bhw.stft_mask_istft_mixed(p, args[0], args[1], args[2], 160)
    S._mask_mfft_refusals(torch, x, m, 400)
    # stft_mask_istft's own refusals stay exactly as they are
    with pytest.raises(ValueError, match=r"got 400 \(a mixed-radix n_fft: bhw\.stft_mixed, a multiply and bhw\.istft_mixed\)"):
        S._mask_fft_refusals(torch, x, m, 400)
