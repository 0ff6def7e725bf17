"""The fused STFT + complex gain + inverse STFT calls of both families (bhw_cmask_fft_f32_* / bhw_cmask_mfft_f32_* and their describe
calls): the checks that need no GPU -- exports and declarations held to the real-gain calls', every refusal of include/bhw.h before any
HIP call with the route it names, the parents' refusals as whole strings, the gain strides in pairs, the 8-byte alignment of d_g, the
extents, the wrap and the overlaps in 8-byte elements, samples 0, no GPU, the Python surface with its ValueErrors, and the real-gain
calls' tail messages, unchanged."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from blackman_harris_win_amd import selector as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED, HIP = 0, -1, -2, -3
# never dereferenced: every call below fails or has nothing to do
X, G, O = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x40000000), ctypes.c_void_p(0x80000000)
F, NB, T = 101, 4, 16000
FAM = {
    "fft": dict(n_fft=512, L=400, col0=56, pad=256, K=257, forward="bhw_stft_fft_f32_device", inverse="bhw_istft_fft_f32_device",
                other="bhw_cmask_mfft_f32_*", other_n=(400, 0, 200), own="bhw_cmask_fft_f32_*"),
    "mfft": dict(n_fft=400, L=400, col0=0, pad=200, K=201, forward="bhw_stft_mfft_f32_device", inverse="bhw_istft_mfft_f32_device",
                 other="bhw_cmask_fft_f32_*", other_n=(512, 56, 256), own="bhw_cmask_mfft_f32_*"),
}
FAMS = list(FAM)
NEW_SYMBOLS = tuple(n for fam in FAM for n in (f"bhw_cmask_{fam}_f32_device", f"bhw_cmask_{fam}_f32_from_table", f"bhw_describe_cmask_{fam}"))


def _err():
    return B.lib().bhw_last_error().decode()


def _desc(fam, analysis, **kw):
    """4 signals of 16000 samples, 101 frames at hop 160, window 400, centred; the analysis side padded by reflection."""
    f = FAM[fam]
    a = dict(batch=NB, samples=T, frames=F, hop=160, n_fft=f["n_fft"], col0=f["col0"], pad=f["pad"], shift=31)
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


def _fn(fam, which, real=False):
    c = "" if real else "c"
    return getattr(B.lib(), {"device": f"bhw_{c}mask_{fam}_f32_device", "table": f"bhw_{c}mask_{fam}_f32_from_table",
                             "describe": f"bhw_describe_{c}mask_{fam}"}[which])


def _calls(fam, sa, ss, flags=1, L=400, x=X, g=G, out=O, gs=None, gbs=None, real=False):
    K = FAM[fam]["K"]
    gs = K if gs is None else gs
    gbs = F * K if gbs is None else gbs
    dev, tab = _fn(fam, "device", real), _fn(fam, "table", real)
    return (lambda p: dev(p, L, 0, None, _ref(sa), _ref(ss), flags, x, g, gs, gbs, out),
            lambda p: tab(None, p, L, None, _ref(sa), _ref(ss), flags, x, g, gs, gbs, out))


def test_the_six_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    assert len(NEW_SYMBOLS) == 6
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        real = name.replace("cmask", "mask")
        assert getattr(L, name).argtypes == getattr(L, real).argtypes, name
        # the declaration is the real-gain call's, word for word apart from the name
        new = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
        old = re.search(r"\bint " + real + r"\(([^;]*)\);", header).group(1)
        assert " ".join(new.split()) == " ".join(old.split()), name
    assert L.bhw_abi_version() == 4 and ctypes.sizeof(B.BhwStft) == 96
    for text in ("fl32( fl32(re * gr) - fl32(im * gi) )", "fl32( fl32(re * gi) + fl32(im * gr) )", "count PAIRS", "8-byte aligned"):
        assert text in header, text


@pytest.mark.parametrize("fam", FAMS)
def test_the_parents_refusals_come_back_as_whole_strings(fam):
    f = FAM[fam]
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    lib = B.lib()
    fwd, inv = getattr(lib, f["forward"]), getattr(lib, f["inverse"])
    analysis = [dict(struct_size=8), dict(channels=3), dict(batch=0), dict(hop=0), dict(n_fft=0), dict(n_fft=8192), dict(n_fft=401),
                dict(shift=63), dict(pad_mode=2), dict(samples=0), dict(frames=102), dict(x_stride=T - 1), dict(pad=T, frames=1),
                dict(batch=1 << 20)]
    for kw in analysis:
        sa = _desc(fam, True, **kw)
        both = {k: v for k, v in kw.items() if k in ("batch", "frames", "hop", "n_fft", "col0", "shift", "channels")}
        ss = _desc(fam, False, **both)
        args = (ref, 400, 0, None, ctypes.byref(sa), 0) + ((None,) if fam == "mfft" else ()) + (X, O)
        rc = fwd(*args)
        want = _err()
        assert rc in (BADARG, UNSUPPORTED), (kw, rc)
        for call in _calls(fam, sa, ss):
            assert call(ref) == rc and _err() == want, (kw, want, _err())
    for kw in (dict(struct_size=8), dict(col0=60, pad=55), dict(pad_mode=B.PAD_REFLECT), dict(samples=(1 << 34) + 1), dict(x_stride=T - 1)):
        ss = _desc(fam, False, **kw)
        rc = inv(ref, 400, 0, None, ctypes.byref(ss), 1, G, O)
        want = _err()
        assert rc == BADARG, (kw, rc)
        for call in _calls(fam, _desc(fam, True), ss):
            assert call(ref) == rc and _err() == want, (kw, want, _err())


def test_the_forward_parents_take_the_arguments_this_file_gives_them():
    """(the mixed-radix forward call has one pointer more than the power-of-two one: guard the argument lists used above)"""
    L = B.lib()
    assert len(L.bhw_stft_mfft_f32_device.argtypes) == len(L.bhw_stft_fft_f32_device.argtypes) + 1 == 9


@pytest.mark.parametrize("fam", FAMS)
def test_refusals_that_name_the_route_that_takes_the_input(fam):
    f = FAM[fam]
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    iq = ("bhw_stft_cfft_f32_*", "bhw_istft_cfft_f32_*") if fam == "fft" else ("bhw_stft_cmfft_f32_*", "bhw_istft_cmfft_f32_*")
    n, col0, pad = f["other_n"]
    cases = [(dict(channels=2), 400, iq + ("complex-gain mask",)),
             (dict(n_fft=n, col0=col0, pad=pad), 400, (f["other"], "complex-gain mask")),
             (dict(n_fft=4096, col0=0, pad=2048), 4096, ("bhw_stft_fft_f32_*", "bhw_istft_fft_f32_*", "complex-gain mask")),
             (dict(n_fft=2160, col0=0, pad=1080), 2160, ("bhw_stft_mfft_f32_*", "bhw_istft_mfft_f32_*", "complex-gain mask")),
             (dict(n_fft=4050, col0=0, pad=2025), 4050, ("bhw_stft_mfft_f32_*", "bhw_istft_mfft_f32_*", "complex-gain mask"))]
    if fam == "fft":
        cases += [(dict(n_fft=18, col0=0, pad=9), 18, (f["other"],)), (dict(n_fft=2000, col0=0, pad=1000), 2000, (f["other"],))]
    else:
        cases += [(dict(n_fft=16, col0=0, pad=8), 16, (f["other"],)), (dict(n_fft=2048, col0=0, pad=1024), 2048, (f["other"],))]
    for kw, L, names in cases:
        for sa, ss in ((_desc(fam, True, **kw), _desc(fam, False, **kw)), (_desc(fam, True, **kw), _desc(fam, False)),
                       (_desc(fam, True), _desc(fam, False, **kw))):
            for call in _calls(fam, sa, ss, L=L):
                assert call(ref) == UNSUPPORTED and all(nm in _err() for nm in names), (kw, _err())
            # the real-gain fused calls are not the route for a complex gain
            assert "bhw_mask_" not in _err(), _err()
            buf = ctypes.create_string_buffer(1280)
            assert _fn(fam, "describe")(None, ref, L, ctypes.byref(sa), ctypes.byref(ss), 1, f["K"], F * f["K"], buf, 1280) == UNSUPPORTED
    # the sentence is the sibling's, about the complex-gain mask
    kw = dict(channels=2)
    _calls(fam, _desc(fam, True, **kw), _desc(fam, False, **kw), real=True)[0](ref)
    real = _err()
    _calls(fam, _desc(fam, True, **kw), _desc(fam, False, **kw))[0](ref)
    assert _err() == real.replace("fused mask", "fused complex-gain mask") != real


@pytest.mark.parametrize("fam", FAMS)
def test_the_descriptors_must_agree_and_have_no_row_strides(fam):
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    for field, kw in (("batch", dict(batch=5)), ("frames", dict(frames=100)), ("hop", dict(hop=161)), ("shift", dict(shift=30))):
        for call in _calls(fam, _desc(fam, True), _desc(fam, False, **kw)):
            assert call(ref) == BADARG and _err().startswith(field + ":") and "must agree" in _err(), (field, _err())
    for kw in (dict(y_stride=600), dict(y_batch_stride=F * 600)):
        for call in _calls(fam, _desc(fam, True, **kw), _desc(fam, False)):
            assert call(ref) == BADARG and "no spectrum rows" in _err() and "analysis" in _err(), _err()
        for call in _calls(fam, _desc(fam, True), _desc(fam, False, **kw)):
            assert call(ref) == BADARG and "no spectrum rows" in _err() and "synthesis" in _err(), _err()


@pytest.mark.parametrize("fam", FAMS)
def test_gain_strides_count_pairs(fam):
    K = FAM[fam]["K"]
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    sa, ss = _desc(fam, True), _desc(fam, False)
    describe = getattr(B, f"describe_cmask_{fam}")
    for gs, gbs, text in ((K - 1, F * K, f"g_stride {K - 1}: 0 (one gain row for every frame) or at least K = {K} pairs"), (1, 0, "g_stride 1"),
                          (K, (F - 1) * K + K - 1, f"or at least (frames - 1) * g_stride + K = {F * K} pairs"), (0, K - 1, f"= {K} pairs"),
                          (K + 7, (F - 1) * (K + 7) + K - 1, "g_batch_stride")):
        for call in _calls(fam, sa, ss, gs=gs, gbs=gbs):
            assert call(ref) == BADARG and text in _err(), (gs, gbs, _err())
        with pytest.raises(B.BhwError, match=re.escape(text)):
            describe(p, 400, sa, ss, g_stride=gs, g_batch_stride=gbs)
    # K pairs are enough where 2 K floats would be asked for if the strides counted floats
    for gs, gbs in ((0, 0), (K, 0), (0, K), (K, F * K), (K + 7, (F - 1) * (K + 7) + K)):
        assert _fn(fam, "table")(None, ref, 400, None, ctypes.byref(sa), ctypes.byref(ss), 1, X, G, gs, gbs, O) == BADARG
        assert "table is NULL" in _err(), (gs, gbs, _err())


@pytest.mark.parametrize("fam", FAMS)
def test_arguments_pointers_and_the_8_byte_alignment_of_d_g(fam):
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    sa, ss = _desc(fam, True), _desc(fam, False)
    for flags in (2, 4, 3, 1 << 31):
        for call in _calls(fam, sa, ss, flags=flags):
            assert call(ref) == BADARG and "flags" in _err()
    for call in _calls(fam, None, ss) + _calls(fam, sa, None):
        assert call(ref) == BADARG and "descriptor is NULL" in _err()
    for call in _calls(fam, sa, ss):
        assert call(None) == BADARG
    for call in _calls(fam, sa, ss, L=0):
        assert call(ref) == BADARG and "length" in _err()
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    for call in _calls(fam, sa, ss):
        assert call(ctypes.byref(taylor)) == UNSUPPORTED
    for kw in (dict(x=None), dict(g=None), dict(out=None)):
        for call in _calls(fam, sa, ss, **kw):
            assert call(ref) == BADARG and "NULL" in _err()
    for kw, name in ((dict(x=ctypes.c_void_p(0x10000002)), "d_x"), (dict(out=ctypes.c_void_p(0x80000003)), "d_out")):
        for call in _calls(fam, sa, ss, **kw):
            assert call(ref) == BADARG and name + " is not 4-byte aligned" in _err()
    # d_g: a message of its own, for a 4-byte aligned pointer too
    for addr in (0x40000004, 0x4000000c, 0x40000002, 0x40000001):
        for call in _calls(fam, sa, ss, g=ctypes.c_void_p(addr)):
            assert call(ref) == BADARG and "d_g is not 8-byte aligned" in _err() and "pairs (gr, gi)" in _err(), (hex(addr), _err())
    for call in _calls(fam, sa, ss, g=ctypes.c_void_p(0x40000008)):
        assert call(ref) in (BADARG, HIP) and "aligned" not in _err()
    # the real-gain call takes the 4-byte aligned pointer, as it did
    assert _calls(fam, sa, ss, g=ctypes.c_void_p(0x40000004), real=True)[1](ref) == BADARG and "table is NULL" in _err()


@pytest.mark.parametrize("fam", FAMS)
def test_extents_and_overlaps_are_computed_in_8_byte_elements(fam):
    K = FAM[fam]["K"]
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    sa, ss = _desc(fam, True), _desc(fam, False)
    tab, tab_real = _fn(fam, "table"), _fn(fam, "table", real=True)
    xb, g8, g4 = NB * T * 4, NB * F * K * 8, NB * F * K * 4
    x0, g0 = 0x10000000, 0x40000000

    def run(fn, x, g, out, gs=K, gbs=F * K):
        rc = fn(None, ref, 400, None, ctypes.byref(sa), ctypes.byref(ss), 1, ctypes.c_void_p(x), ctypes.c_void_p(g), gs, gbs, ctypes.c_void_p(out))
        assert rc == BADARG
        return _err()

    for out, bad in ((x0 + xb - 4, "d_x and d_out"), (x0 + xb, None), (x0, "d_x and d_out"),
                     (g0, "d_g and d_out"), (g0 + g4 - 4, "d_g and d_out"),
                     (g0 + g4, "d_g and d_out"),                       # the first byte of the SECOND half of the gain array
                     (g0 + g8 - 4, "d_g and d_out"), (g0 + g8, None)):
        assert (bad + " overlap" if bad else "table is NULL") in run(tab, x0, g0, out), hex(out)
    # the 4-byte extent misses exactly that: the real-gain call, whose array ends there, passes the same pointers
    assert "table is NULL" in run(tab_real, x0, g0, g0 + g4)
    assert "d_g and d_out overlap" in run(tab_real, x0, g0, g0 + g4 - 4)
    # out in front of the gains: its last float against their first pair
    assert "d_g and d_out overlap" in run(tab, x0, 0x80000000 + xb - 8, 0x80000000)
    assert "table is NULL" in run(tab, x0, 0x80000000 + xb, 0x80000000)
    # a broadcast row is K pairs however many signals there are
    assert "d_g and d_out overlap" in run(tab, x0, g0, g0 + K * 8 - 4, 0, 0)
    assert "table is NULL" in run(tab, x0, g0, g0 + K * 8, 0, 0)
    # padded strides: the last row ends K pairs in
    gs, gbs = K + 7, (F - 1) * (K + 7) + K + 11
    end = ((NB - 1) * gbs + (F - 1) * gs + K) * 8
    assert "d_g and d_out overlap" in run(tab, x0, g0, g0 + end - 4, gs, gbs)
    assert "table is NULL" in run(tab, x0, g0, g0 + end, gs, gbs)
    # the wrap of the address space: the gain array's bytes, 8 per element
    top = (1 << 64) - g8
    assert top % 8 == 0 and "table is NULL" in run(tab, x0, top - 8, 0x80000000)
    assert "wraps the address space" in run(tab, x0, top, 0x80000000)
    assert "table is NULL" in run(tab_real, x0, top, 0x80000000)          # 4-byte elements: half the bytes, no wrap
    # the 2^60 bound counts elements
    assert "beyond 2^60" in run(tab, x0, g0, 0x80000000, K, 1 << 59)


@pytest.mark.parametrize("fam", FAMS)
def test_samples_zero_is_ok_with_the_pointers_unchecked(fam):
    p = B.make_params(B.WIN_BH7, 16, 32)
    describe = getattr(B, f"describe_cmask_{fam}")
    for flags in (0, 1):
        sa, ss = _desc(fam, True), _desc(fam, False, samples=0)
        assert _fn(fam, "device")(ctypes.byref(p), 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), flags, None, None, 3, 5, None) == OK
        assert "nothing (samples 0)" in describe(p, 400, sa, ss, normalize=bool(flags))
        sa, ss = _desc(fam, True, frames=0), _desc(fam, False, samples=0, frames=0)
        assert _fn(fam, "device")(ctypes.byref(p), 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), flags, None, None, 0, 0, None) == OK


@pytest.mark.parametrize("fam", FAMS)
def test_compute_entry_point_fails_loudly_without_a_gpu(fam):
    """No CPU fallback: with every check passed and no HIP device the library call returns BHW_ERR_HIP."""
    import torch
    if torch.cuda.is_available():
        return
    p = B.make_params(B.WIN_BH7, 16, 32)
    sa, ss = _desc(fam, True), _desc(fam, False)
    K = FAM[fam]["K"]
    rc = _fn(fam, "device")(ctypes.byref(p), 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), 1, X, G, K, F * K, O)
    assert rc == HIP, (rc, _err())
    call = bhw.stft_cmask_istft if fam == "fft" else bhw.stft_cmask_istft_mixed
    with pytest.raises(RuntimeError):
        call(p, torch.zeros(1000), torch.ones(K, dtype=torch.complex64), FAM[fam]["n_fft"], 160)


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    buf = ctypes.create_string_buffer(1280)
    took = {"fft": [], "mfft": []}
    for n in range(1, 4200):
        sa = B.make_stft(2, 10000, 3, 7, n, pad=n // 2, pad_mode=0, shift=31)
        ss = B.make_stft(2, 1000, 3, 7, n, pad=n // 2, shift=31)
        for fam, ok in (("fft", B.mask_fft_supported(n)), ("mfft", B.mask_mfft_supported(n))):
            rc = _fn(fam, "describe")(None, ctypes.byref(p), min(n, 16), ctypes.byref(sa), ctypes.byref(ss), 1, 0, 0, buf, 1280)
            assert rc == (OK if ok else (UNSUPPORTED if n >= 14 else rc)), (fam, n, rc, _err())
            if rc == OK:
                took[fam].append(n)
    assert took["fft"] == [16, 32, 64, 128, 256, 512, 1024, 2048] and len(took["mfft"]) == 73 and took["mfft"][0] == 18 and took["mfft"][-1] == 2000


def test_python_surface():
    for name in ("stft_cmask_istft", "stft_cmask_istft_mixed", "describe_cmask_fft", "describe_cmask_mfft"):
        assert name in bhw.__all__ and hasattr(bhw, name), name
    want = list(inspect.signature(bhw.stft_mask_istft).parameters)
    assert want == ["params", "x", "mask", "n_fft", "hop", "win_length", "center", "pad_mode", "length", "normalize", "shift", "out", "table"]
    for fn in (bhw.stft_cmask_istft, bhw.stft_cmask_istft_mixed):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == want
        for name in want[5:]:
            assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
            assert sig.parameters[name].default == inspect.signature(bhw.stft_mask_istft).parameters[name].default
        doc = " ".join(fn.__doc__.split())
        assert "BIT FOR BIT" in doc and "complex64" in doc and "complex multiply" in doc
        assert not hasattr(bhw.ResidentTable, fn.__name__)
    doc = " ".join(bhw.stft_cmask_istft.__doc__.split())
    assert "Y.real * G.real - Y.imag * G.imag" in doc and "Y.real * G.imag + Y.imag * G.real" in doc and "expand()" in doc
    assert "not promised to equal Y * G of torch complex tensors bit for bit" in doc
    assert hasattr(B, "describe_cmask_fft") and hasattr(B, "describe_cmask_mfft")
    # one text behind all four public calls
    src = inspect.getsource(S)
    assert src.count("def _stft_mask_istft(") == 1 and src.count("_stft_mask_istft(torch, params, x, mask") == 5
    # the real calls point here, and keep their refusal of a complex mask
    assert "stft_cmask_istft" in bhw.stft_mask_istft.__doc__ and "stft_cmask_istft_mixed" in bhw.stft_mask_istft_mixed.__doc__


def test_python_refusals_name_the_routes_and_need_no_device():
    """Each ValueError through the public function on host tensors: raised before any device is looked at."""
    import torch
    p = B.make_params(B.WIN_BH7, 16, 32)
    x = torch.zeros(2, 1000)

    def g(K):
        return torch.ones(K, dtype=torch.complex64)

    cases = (
        (bhw.stft_cmask_istft, (x, torch.ones(257), 512), r"complex64 gains, got torch\.float32: bhw\.stft_mask_istft takes real gains"),
        (bhw.stft_cmask_istft_mixed, (x, torch.ones(201), 400), r"complex64 gains, got torch\.float32: bhw\.stft_mask_istft_mixed takes real gains"),
        (bhw.stft_cmask_istft, (x.to(torch.complex64), g(257), 512), r"I/Q input: bhw\.stft_iq, a complex multiply and bhw\.istft_iq\)"),
        (bhw.stft_cmask_istft_mixed, (x.to(torch.complex64), g(201), 400), r"bhw\.stft_iq_mixed, a complex multiply and bhw\.istft_iq_mixed"),
        (bhw.stft_cmask_istft, (x, g(201), 400), r"got 400 \(a mixed-radix n_fft: bhw\.stft_cmask_istft_mixed takes it\)"),
        (bhw.stft_cmask_istft, (x, g(10), 18), r"bhw\.stft_cmask_istft_mixed takes it"),
        (bhw.stft_cmask_istft_mixed, (x, g(257), 512), r"512 is a power of two: bhw\.stft_cmask_istft takes it"),
        (bhw.stft_cmask_istft_mixed, (x, g(9), 16), r"bhw\.stft_cmask_istft takes it"),
        (bhw.stft_cmask_istft, (torch.zeros(2, 9000), g(2049), 4096), r"got 4096 \(bhw\.stft, a complex multiply and bhw\.istft take it\)"),
        (bhw.stft_cmask_istft_mixed, (torch.zeros(2, 9000), g(2049), 4096), r"above 2048: bhw\.stft, a complex multiply and bhw\.istft take it"),
        (bhw.stft_cmask_istft_mixed, (torch.zeros(2, 9000), g(1281), 2560), r"got 2560 \(bhw\.stft_mixed, a complex multiply and bhw\.istft_mixed take it\)"),
        (bhw.stft_cmask_istft, (torch.zeros(2, 9000), g(1081), 2160), r"got 2160 \(bhw\.stft_mixed, a complex multiply and bhw\.istft_mixed take it\)"),
    )
    for fn, args, text in cases:
        with pytest.raises(ValueError, match=text):
            fn(p, args[0], args[1], args[2], 160)
    S._cmask_refusals(torch, x, g(257), 512, False)
    S._cmask_refusals(torch, x, g(201), 400, True)
    # the real-gain calls refuse a complex mask in their present words
    with pytest.raises(ValueError, match=r"complex gains are not built: bhw\.stft, a complex multiply and bhw\.istft apply them"):
        S._mask_fft_refusals(torch, x, g(257), 512)
    with pytest.raises(ValueError, match=r"complex gains are not built: bhw\.stft_mixed, a complex multiply and bhw\.istft_mixed apply them"):
        S._mask_mfft_refusals(torch, x, g(201), 400)


@pytest.mark.parametrize("fam", FAMS)
def test_the_real_gain_calls_tail_messages_are_unchanged(fam):
    """The four messages of the shared tail that speak of the gain element, through the real-gain calls: floats, and 4-byte alignment."""
    K = FAM[fam]["K"]
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    sa, ss = _desc(fam, True), _desc(fam, False)

    def msg(**kw):
        rc = _calls(fam, sa, ss, real=True, **kw)[0](ref)
        assert rc == BADARG
        return _err()

    assert msg(gs=K - 1) == f"g_stride {K - 1}: 0 (one gain row for every frame) or at least K = {K} floats"
    assert msg(gs=0, gbs=K - 1) == (f"g_batch_stride {K - 1}: 0 (the same gains for every signal) or at least (frames - 1) * g_stride + K = "
                                    f"{K} floats")
    assert msg(g=ctypes.c_void_p(0x40000002)) == "d_g is not 4-byte aligned"
    assert msg(out=G) == "d_g and d_out overlap"
    assert msg(out=X) == "d_x and d_out overlap" and msg(x=None) == "d_x / d_g / d_out is NULL"
    assert msg(gs=K, gbs=1 << 59) == "x, g or out extent beyond 2^60 elements"
