"""The fused STFT + gain + inverse STFT calls for I/Q input (bhw_mask_cfft_f32_*, bhw_cmask_cfft_f32_*, bhw_mask_cmfft_f32_*,
bhw_cmask_cmfft_f32_* and their describe calls): the checks that need no GPU -- exports and declarations held to the real-signal mask
calls', every refusal before any HIP call with the route it names, the parents' refusals as whole strings and their order, the gain
strides with K = n_fft, the 8-byte alignment of pair gains and of nothing else, the extents and overlaps in floats of two per sample and
in gain elements, samples 0, no GPU, the Python surface, and the existing calls' refusals of channels = 2, unchanged."""
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
    "cfft": dict(n_fft=512, L=400, col0=56, pad=256, forward="bhw_stft_cfft_f32_device", inverse="bhw_istft_cfft_f32_device",
                 other="cmfft", other_n=(400, 0, 200), real="fft", pair=("bhw_stft_cfft_f32_*", "bhw_istft_cfft_f32_*")),
    "cmfft": dict(n_fft=400, L=400, col0=0, pad=200, forward="bhw_stft_cmfft_f32_device", inverse="bhw_istft_cmfft_f32_device",
                  other="cfft", other_n=(512, 56, 256), real="mfft", pair=("bhw_stft_cmfft_f32_*", "bhw_istft_cmfft_f32_*")),
}
CALLS = [(fam, c) for fam in FAM for c in ("", "c")]
IDS = [f"{c}mask_{fam}" for fam, c in CALLS]
NEW_SYMBOLS = tuple(n for fam, c in CALLS for n in (f"bhw_{c}mask_{fam}_f32_device", f"bhw_{c}mask_{fam}_f32_from_table",
                                                    f"bhw_describe_{c}mask_{fam}"))


def _err():
    return B.lib().bhw_last_error().decode()


def _desc(fam, analysis, **kw):
    """4 I/Q signals of 16000 samples, 101 frames at hop 160, window 400, centred; the analysis side padded by reflection."""
    f = FAM[fam]
    a = dict(batch=NB, samples=T, frames=F, hop=160, n_fft=f["n_fft"], col0=f["col0"], pad=f["pad"], shift=31, channels=2)
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


def _fn(fam, c, which):
    return getattr(B.lib(), {"device": f"bhw_{c}mask_{fam}_f32_device", "table": f"bhw_{c}mask_{fam}_f32_from_table",
                             "describe": f"bhw_describe_{c}mask_{fam}"}[which])


def _calls(fam, c, sa, ss, flags=1, L=400, x=X, g=G, out=O, gs=None, gbs=None):
    K = (ss if ss is not None else sa).n_fft if (ss is not None or sa is not None) else FAM[fam]["n_fft"]
    gs = K if gs is None else gs
    gbs = F * K if gbs is None else gbs
    dev, tab = _fn(fam, c, "device"), _fn(fam, c, "table")
    return (lambda p: dev(p, L, 0, None, _ref(sa), _ref(ss), flags, x, g, gs, gbs, out),
            lambda p: tab(None, p, L, None, _ref(sa), _ref(ss), flags, x, g, gs, gbs, out))


def test_the_twelve_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    assert len(NEW_SYMBOLS) == 12
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        real = re.sub(r"c?mask_cm?fft", "mask_fft", name)
        assert getattr(L, name).argtypes == getattr(L, real).argtypes, name
        # the declaration is the real-signal call's, argument for argument
        new = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
        old = re.search(r"\bint " + real + r"\(([^;]*)\);", header).group(1)
        assert " ".join(new.split()) == " ".join(old.split()), name
    assert L.bhw_abi_version() == 4 and ctypes.sizeof(B.BhwStft) == 96
    for text in ("NO BIN IS SPECIAL", "K = n_fft", "(fl32(re * g), fl32(im * g))", "column (k + n_fft / 2) mod"):
        assert text in " ".join(header.split()), text


@pytest.mark.parametrize("fam,c", CALLS, ids=IDS)
def test_the_parents_refusals_come_back_as_whole_strings_and_in_their_order(fam, c):
    f = FAM[fam]
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    lib = B.lib()
    fwd, inv = getattr(lib, f["forward"]), getattr(lib, f["inverse"])
    analysis = [dict(struct_size=8), dict(channels=3), dict(batch=0), dict(hop=0), dict(n_fft=0), dict(n_fft=8192), dict(n_fft=401),
                dict(shift=63), dict(pad_mode=2), dict(samples=0), dict(frames=102), dict(x_stride=2 * T - 1), dict(pad=T, frames=1),
                dict(batch=1 << 20)]
    for kw in analysis:
        sa = _desc(fam, True, **kw)
        both = {k: v for k, v in kw.items() if k in ("batch", "frames", "hop", "n_fft", "col0", "shift", "channels")}
        ss = _desc(fam, False, **both)
        rc = fwd(ref, 400, 0, None, ctypes.byref(sa), 0, X, O)
        want = _err()
        assert rc in (BADARG, UNSUPPORTED), (kw, rc)
        for call in _calls(fam, c, sa, ss):
            assert call(ref) == rc and _err() == want, (kw, want, _err())
    for kw in (dict(struct_size=8), dict(col0=60, pad=55), dict(pad_mode=B.PAD_REFLECT), dict(samples=(1 << 34) + 1), dict(x_stride=2 * T - 1)):
        ss = _desc(fam, False, **kw)
        rc = inv(ref, 400, 0, None, ctypes.byref(ss), 1, G, O)
        want = _err()
        assert rc == BADARG, (kw, rc)
        for call in _calls(fam, c, _desc(fam, True), ss):
            assert call(ref) == rc and _err() == want, (kw, want, _err())
    # the order: the analysis descriptor's fault is reported before the synthesis one's, both before a bad gain stride or pointer
    sa, ss = _desc(fam, True, hop=0), _desc(fam, False, col0=60, pad=55)
    fwd(ref, 400, 0, None, ctypes.byref(sa), 0, X, O)
    first = _err()
    for call in _calls(fam, c, sa, ss, gs=1, x=None):
        assert call(ref) == BADARG and _err() == first
    ss = _desc(fam, False, x_stride=2 * T - 1)
    inv(ref, 400, 0, None, ctypes.byref(ss), 1, G, O)
    second = _err()
    for call in _calls(fam, c, _desc(fam, True), ss, gs=1, x=None):
        assert call(ref) == BADARG and _err() == second
    for call in _calls(fam, c, _desc(fam, True), _desc(fam, False), gs=1, x=None):
        assert call(ref) == BADARG and _err().startswith("g_stride 1:")


@pytest.mark.parametrize("fam,c", CALLS, ids=IDS)
def test_flags_the_shift_is_taken_and_detrending_is_refused(fam, c):
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    sa, ss = _desc(fam, True), _desc(fam, False)
    for flags in (0, B.OLA_NORMALIZE, B.CFFT_SHIFT, B.OLA_NORMALIZE | B.CFFT_SHIFT):
        assert _calls(fam, c, sa, ss, flags=flags)[1](ref) == BADARG and "table is NULL" in _err(), flags
    for flags in (B.CFFT_POWER, 8, 1 << 31, B.CFFT_POWER | B.OLA_NORMALIZE):
        for call in _calls(fam, c, sa, ss, flags=flags):
            assert call(ref) == BADARG and _err() == f"flags 0x{flags:x} (BHW_OLA_NORMALIZE, BHW_CFFT_SHIFT)", _err()
    describe = getattr(B, f"describe_{c}mask_{fam}")
    assert ", gain columns shifted, " in describe(p, 400, sa, ss, fftshift=True)
    assert ", gain columns in order, " in describe(p, 400, sa, ss)
    assert ("complex gains: " in describe(p, 400, sa, ss)) == (c == "c")
    assert describe(p, 400, sa, ss).startswith(f"{c}mask {fam} direct (L = 400, n_fft {FAM[fam]['n_fft']}, ")


@pytest.mark.parametrize("fam,c", CALLS, ids=IDS)
def test_refusals_that_name_the_route_that_takes_the_input(fam, c):
    f = FAM[fam]
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    n, col0, pad = f["other_n"]
    what = "fused I/Q complex-gain mask" if c else "fused I/Q mask"
    cases = [(dict(channels=1), 400, (f"bhw_{c}mask_{f['real']}_f32_* takes a real signal", what)),
             (dict(n_fft=n, col0=col0, pad=pad), 400, (f"bhw_{c}mask_{f['other']}_f32_*", what)),
             (dict(n_fft=4096, col0=0, pad=2048), 4096, f["pair"] + (what,))]
    if fam == "cfft":
        cases += [(dict(n_fft=18, col0=0, pad=9), 18, (f"bhw_{c}mask_cmfft_f32_*",)), (dict(n_fft=2025, col0=0, pad=1012), 2025, (f"bhw_{c}mask_cmfft_f32_*",))]
    else:
        cases += [(dict(n_fft=16, col0=0, pad=8), 16, (f"bhw_{c}mask_cfft_f32_*",)), (dict(n_fft=2048, col0=0, pad=1024), 2048, (f"bhw_{c}mask_cfft_f32_*",)),
                  (dict(n_fft=2160, col0=0, pad=1080), 2160, f["pair"] + (what,)), (dict(n_fft=4050, col0=0, pad=2025), 4050, f["pair"] + (what,))]
    for kw, L, names in cases:
        for sa, ss in ((_desc(fam, True, **kw), _desc(fam, False, **kw)), (_desc(fam, True, **kw), _desc(fam, False)),
                       (_desc(fam, True), _desc(fam, False, **kw))):
            for call in _calls(fam, c, sa, ss, L=L):
                assert call(ref) == UNSUPPORTED and all(nm in _err() for nm in names), (kw, _err())
            if not c:
                assert "cmask" not in _err(), _err()                   # a real-gain call names real-gain routes
            buf = ctypes.create_string_buffer(1280)
            K = ss.n_fft
            assert _fn(fam, c, "describe")(None, ref, L, ctypes.byref(sa), ctypes.byref(ss), 1, K, F * K, buf, 1280) == UNSUPPORTED
    # the sentence names which descriptor
    _calls(fam, c, _desc(fam, True), _desc(fam, False, channels=1))[0](ref)
    assert "channels 1 (synthesis descriptor)" in _err()
    _calls(fam, c, _desc(fam, True, channels=1), _desc(fam, False))[0](ref)
    assert "channels 1 (analysis descriptor)" in _err()


@pytest.mark.parametrize("fam", ["fft", "mfft"])
def test_the_existing_calls_refusals_of_channels_2_are_unchanged(fam):
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    n, col0, pad = (512, 56, 256) if fam == "fft" else (400, 0, 200)
    sa = B.make_stft(NB, T, F, 160, n, col0=col0, pad=pad, pad_mode=1, shift=31, channels=2)
    ss = B.make_stft(NB, T, F, 160, n, col0=col0, pad=pad, shift=31, channels=2)
    K = n // 2 + 1
    want = {("fft", ""): "channels 2 (analysis descriptor): the fused mask takes real input and gives real output; bhw_stft_cfft_f32_* + "
                         "bhw_istft_cfft_f32_* take I/Q",
            ("fft", "c"): "channels 2 (analysis descriptor): the fused complex-gain mask takes real input and gives real output; "
                          "bhw_stft_cfft_f32_* + bhw_istft_cfft_f32_* take I/Q",
            ("mfft", ""): "channels 2 (analysis descriptor): the mixed-radix fused mask takes real input and gives real output; "
                          "bhw_stft_cmfft_f32_* + bhw_istft_cmfft_f32_* take I/Q",
            ("mfft", "c"): "channels 2 (analysis descriptor): the mixed-radix fused complex-gain mask takes real input and gives real output; "
                           "bhw_stft_cmfft_f32_* + bhw_istft_cmfft_f32_* take I/Q"}
    for c in ("", "c"):
        fn = getattr(B.lib(), f"bhw_{c}mask_{fam}_f32_device")
        assert fn(ref, 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), 1, X, G, K, F * K, O) == UNSUPPORTED
        assert _err() == want[(fam, c)]


@pytest.mark.parametrize("fam,c", CALLS, ids=IDS)
def test_the_descriptors_must_agree_and_have_no_row_strides(fam, c):
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    for field, kw in (("batch", dict(batch=5)), ("frames", dict(frames=100)), ("hop", dict(hop=161)), ("shift", dict(shift=30))):
        for call in _calls(fam, c, _desc(fam, True), _desc(fam, False, **kw)):
            assert call(ref) == BADARG and _err().startswith(field + ":") and "must agree" in _err(), (field, _err())
    for kw in (dict(y_stride=1200), dict(y_batch_stride=F * 1200)):
        for call in _calls(fam, c, _desc(fam, True, **kw), _desc(fam, False)):
            assert call(ref) == BADARG and "no spectrum rows" in _err() and "analysis" in _err(), _err()
        for call in _calls(fam, c, _desc(fam, True), _desc(fam, False, **kw)):
            assert call(ref) == BADARG and "no spectrum rows" in _err() and "synthesis" in _err(), _err()


@pytest.mark.parametrize("fam,c", CALLS, ids=IDS)
def test_gain_stride_minima_with_k_equal_to_n_fft(fam, c):
    K = FAM[fam]["n_fft"]
    unit = "pairs" if c else "floats"
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    sa, ss = _desc(fam, True), _desc(fam, False)
    describe = getattr(B, f"describe_{c}mask_{fam}")
    for gs, gbs, text in ((K - 1, F * K, f"g_stride {K - 1}: 0 (one gain row for every frame) or at least K = {K} {unit}"),
                          (K // 2 + 1, 0, f"at least K = {K} {unit}"),         # the real-signal K is not enough
                          (K, (F - 1) * K + K - 1, f"or at least (frames - 1) * g_stride + K = {F * K} {unit}"), (0, K - 1, f"= {K} {unit}"),
                          (K + 7, (F - 1) * (K + 7) + K - 1, "g_batch_stride")):
        for call in _calls(fam, c, sa, ss, gs=gs, gbs=gbs):
            assert call(ref) == BADARG and text in _err(), (gs, gbs, _err())
        with pytest.raises(B.BhwError, match=re.escape(text)):
            describe(p, 400, sa, ss, g_stride=gs, g_batch_stride=gbs)
    for gs, gbs in ((0, 0), (K, 0), (0, K), (K, F * K), (K + 7, (F - 1) * (K + 7) + K)):
        assert _fn(fam, c, "table")(None, ref, 400, None, ctypes.byref(sa), ctypes.byref(ss), 1, X, G, gs, gbs, O) == BADARG
        assert "table is NULL" in _err(), (gs, gbs, _err())
    # an odd n_fft takes all its bins too
    if fam == "cmfft":
        kw = dict(n_fft=75, col0=0, pad=37, frames=100)
        sa, ss = _desc(fam, True, **kw), _desc(fam, False, **kw)
        for call in _calls(fam, c, sa, ss, L=75, gs=74):
            assert call(ref) == BADARG and f"at least K = 75 {unit}" in _err()
        assert _calls(fam, c, sa, ss, L=75, gs=75, gbs=100 * 75)[1](ref) == BADARG and "table is NULL" in _err()


@pytest.mark.parametrize("fam,c", CALLS, ids=IDS)
def test_arguments_pointers_and_alignment(fam, c):
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    sa, ss = _desc(fam, True), _desc(fam, False)
    for call in _calls(fam, c, None, ss) + _calls(fam, c, sa, None):
        assert call(ref) == BADARG and "descriptor is NULL" in _err()
    for call in _calls(fam, c, sa, ss):
        assert call(None) == BADARG
    for call in _calls(fam, c, sa, ss, L=0):
        assert call(ref) == BADARG and "length" in _err()
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    for call in _calls(fam, c, sa, ss):
        assert call(ctypes.byref(taylor)) == UNSUPPORTED
    for kw in (dict(x=None), dict(g=None), dict(out=None)):
        for call in _calls(fam, c, sa, ss, **kw):
            assert call(ref) == BADARG and _err() == "d_x / d_g / d_out is NULL"
    for kw, name in ((dict(x=ctypes.c_void_p(0x10000002)), "d_x"), (dict(out=ctypes.c_void_p(0x80000003)), "d_out")):
        for call in _calls(fam, c, sa, ss, **kw):
            assert call(ref) == BADARG and name + " is not 4-byte aligned" in _err()
    # the signals may sit one float off the 8-byte grid (the kernels then take two 4-byte accesses a sample)
    assert _calls(fam, c, sa, ss, x=ctypes.c_void_p(0x10000004), out=ctypes.c_void_p(0x80000004))[1](ref) == BADARG and "table is NULL" in _err()
    if c:                                                                  # pair gains: 8-byte aligned, a message of its own
        for addr in (0x40000004, 0x4000000c, 0x40000002, 0x40000001):
            for call in _calls(fam, c, sa, ss, g=ctypes.c_void_p(addr)):
                assert call(ref) == BADARG and "d_g is not 8-byte aligned" in _err() and "pairs (gr, gi)" in _err(), (hex(addr), _err())
    else:                                                                  # real gains: 4 bytes are enough
        assert _calls(fam, c, sa, ss, g=ctypes.c_void_p(0x40000004))[1](ref) == BADARG and "table is NULL" in _err()
        for call in _calls(fam, c, sa, ss, g=ctypes.c_void_p(0x40000002)):
            assert call(ref) == BADARG and _err() == "d_g is not 4-byte aligned"


@pytest.mark.parametrize("fam,c", CALLS, ids=IDS)
def test_extents_and_overlaps_in_the_right_element_sizes(fam, c):
    K = FAM[fam]["n_fft"]
    ge = 8 if c else 4
    p = B.make_params(B.WIN_BH4, 24, 32)
    ref = ctypes.byref(p)
    sa, ss = _desc(fam, True), _desc(fam, False)
    tab = _fn(fam, c, "table")
    xb, gb = NB * T * 8, NB * F * K * ge                                   # a complex sample is 8 bytes
    x0, g0 = 0x10000000, 0x40000000

    def run(x, g, out, gs=K, gbs=F * K, sa=sa, ss=ss):
        rc = tab(None, ref, 400, None, ctypes.byref(sa), ctypes.byref(ss), 1, ctypes.c_void_p(x), ctypes.c_void_p(g), gs, gbs, ctypes.c_void_p(out))
        assert rc == BADARG
        return _err()

    for out, bad in ((x0, "d_x and d_out"), (x0 + xb // 2 - 4, "d_x and d_out"),
                     (x0 + xb // 2, "d_x and d_out"),                      # where d_x would end if its extent were counted in samples of 4 bytes
                     (x0 + xb - 4, "d_x and d_out"),                       # inside the second half of d_x's last complex sample
                     (x0 + xb, None),
                     (g0, "d_g and d_out"), (g0 + gb - 4, "d_g and d_out"), (g0 + gb, None)):
        assert (bad + " overlap" if bad else "table is NULL") in run(x0, g0, out), hex(out)
    # out in front of the input: its last float (the imaginary part of its last sample) against the input's first
    assert "d_x and d_out overlap" in run(0x20000000 + xb - 4, g0, 0x20000000)
    assert "table is NULL" in run(0x20000000 + xb, g0, 0x20000000)
    # out in front of the gains
    assert "d_g and d_out overlap" in run(x0, 0x80000000 + xb - ge, 0x80000000)
    assert "table is NULL" in run(x0, 0x80000000 + xb, 0x80000000)
    # strided signals: the extent is (B - 1) * x_stride + 2 * samples floats
    sp = _desc(fam, True, x_stride=2 * T + 6)
    xe = ((NB - 1) * (2 * T + 6) + 2 * T) * 4
    assert "d_x and d_out overlap" in run(x0, g0, x0 + xe - 4, sa=sp)
    assert "table is NULL" in run(x0, g0, x0 + xe, sa=sp)
    # a broadcast row is K gains however many signals there are
    assert "d_g and d_out overlap" in run(x0, g0, g0 + K * ge - 4, 0, 0)
    assert "table is NULL" in run(x0, g0, g0 + K * ge, 0, 0)
    # the wrap of the address space and the 2^60 bound
    top = (1 << 64) - gb
    assert "table is NULL" in run(x0, top - 8, 0x80000000)
    assert "wraps the address space" in run(x0, top, 0x80000000)
    assert "beyond 2^60" in run(x0, g0, 0x80000000, K, 1 << 59)


@pytest.mark.parametrize("fam,c", CALLS, ids=IDS)
def test_samples_zero_is_ok_with_the_pointers_unchecked(fam, c):
    p = B.make_params(B.WIN_BH7, 16, 32)
    describe = getattr(B, f"describe_{c}mask_{fam}")
    for flags in (0, 1, 5):
        sa, ss = _desc(fam, True), _desc(fam, False, samples=0)
        assert _fn(fam, c, "device")(ctypes.byref(p), 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), flags, None, None, 3, 5, None) == OK
        assert "nothing (samples 0)" in describe(p, 400, sa, ss, normalize=bool(flags & 1), fftshift=bool(flags & 4))


@pytest.mark.parametrize("fam,c", CALLS, ids=IDS)
def test_compute_entry_point_fails_loudly_without_a_gpu(fam, c):
    """No CPU fallback: with every check passed and no HIP device the library call returns BHW_ERR_HIP."""
    import torch
    if torch.cuda.is_available():
        return
    p = B.make_params(B.WIN_BH7, 16, 32)
    sa, ss = _desc(fam, True), _desc(fam, False)
    K = FAM[fam]["n_fft"]
    rc = _fn(fam, c, "device")(ctypes.byref(p), 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), 1, X, G, K, F * K, O)
    assert rc == HIP, (rc, _err())
    call = getattr(bhw, f"stft_{c}mask_istft_iq" + ("_mixed" if fam == "cmfft" else ""))
    with pytest.raises(RuntimeError):
        call(p, torch.zeros(1000, dtype=torch.complex64), torch.ones(K, dtype=torch.complex64 if c else torch.float32), K, 160)


def test_every_supported_size_passes_and_its_neighbours_do_not():
    p = B.make_params(B.WIN_BH7, 16, 32)
    buf = ctypes.create_string_buffer(1280)
    took = {"cfft": [], "cmfft": []}
    for n in range(1, 4200):
        sa = B.make_stft(2, 10000, 3, 7, n, pad=n // 2, pad_mode=0, shift=31, channels=2)
        ss = B.make_stft(2, 1000, 3, 7, n, pad=n // 2, shift=31, channels=2)
        for fam, ok in (("cfft", B.cfft_supported(n)), ("cmfft", B.cmfft_supported(n))):
            for c in ("", "c"):
                rc = _fn(fam, c, "describe")(None, ctypes.byref(p), min(n, 16), ctypes.byref(sa), ctypes.byref(ss), 1, 0, 0, buf, 1280)
                assert rc == (OK if ok else (UNSUPPORTED if n >= 14 else rc)), (fam, c, n, rc, _err())
            if rc == OK:
                took[fam].append(n)
    assert took["cfft"] == [16, 32, 64, 128, 256, 512, 1024, 2048]
    assert len(took["cmfft"]) == 91 and took["cmfft"][0] == 18 and took["cmfft"][-1] == 2025 and sum(n & 1 for n in took["cmfft"]) == 18


def test_python_surface():
    names = ("stft_mask_istft_iq", "stft_cmask_istft_iq", "stft_mask_istft_iq_mixed", "stft_cmask_istft_iq_mixed")
    for name in names + ("describe_mask_cfft", "describe_cmask_cfft", "describe_mask_cmfft", "describe_cmask_cmfft"):
        assert name in bhw.__all__ and hasattr(bhw, name), name
    want = ["params", "x", "mask", "n_fft", "hop", "win_length", "center", "pad_mode", "length", "normalize", "shift", "fftshift", "out", "table"]
    first = inspect.signature(bhw.stft_mask_istft_iq)
    for name in names:
        sig = inspect.signature(getattr(bhw, name))
        assert list(sig.parameters) == want, name
        for k in want[5:]:
            assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == first.parameters[k].default
        assert sig.parameters["fftshift"].default is False
        assert not hasattr(bhw.ResidentTable, name)                        # table= is the route
        assert "BIT FOR BIT" in getattr(bhw, name).__doc__
    doc = " ".join(bhw.stft_cmask_istft_iq.__doc__.split())
    assert "Y.real * G.real - Y.imag * G.imag" in doc and "Y.real * G.imag + Y.imag * G.real" in doc and "No bin is special" in doc
    # one text behind all eight public calls
    src = inspect.getsource(S)
    assert src.count("def _stft_mask_istft(") == 1 and src.count("return _stft_mask_istft(torch, params, ") == 5


def test_python_refusals_name_the_routes_and_need_no_device():
    """Each ValueError through the public function on host tensors: raised before any device is looked at."""
    import torch
    p = B.make_params(B.WIN_BH7, 16, 32)
    x = torch.zeros(2, 1000, dtype=torch.complex64)
    big = torch.zeros(2, 9000, dtype=torch.complex64)

    def g(K, complex_gains=True):
        return torch.ones(K, dtype=torch.complex64 if complex_gains else torch.float32)

    cases = (
        (bhw.stft_mask_istft_iq, (x.real, g(512, False), 512), r"got torch\.float32: bhw\.stft_mask_istft takes a real signal"),
        (bhw.stft_cmask_istft_iq, (x.real, g(512), 512), r"bhw\.stft_cmask_istft takes a real signal"),
        (bhw.stft_mask_istft_iq_mixed, (x.real, g(400, False), 400), r"bhw\.stft_mask_istft_mixed takes a real signal"),
        (bhw.stft_cmask_istft_iq_mixed, (x.real, g(400), 400), r"bhw\.stft_cmask_istft_mixed takes a real signal"),
        (bhw.stft_mask_istft_iq, (x, g(512), 512), r"real float32 gains, got torch\.complex64: bhw\.stft_cmask_istft_iq takes complex gains"),
        (bhw.stft_cmask_istft_iq, (x, g(512, False), 512), r"complex64 gains, got torch\.float32: bhw\.stft_mask_istft_iq takes real gains"),
        (bhw.stft_mask_istft_iq_mixed, (x, g(400), 400), r"bhw\.stft_cmask_istft_iq_mixed takes complex gains"),
        (bhw.stft_cmask_istft_iq_mixed, (x, g(400, False), 400), r"bhw\.stft_mask_istft_iq_mixed takes real gains"),
        (bhw.stft_mask_istft_iq, (x, g(400, False), 400), r"got 400 \(a mixed-radix n_fft: bhw\.stft_mask_istft_iq_mixed takes it\)"),
        (bhw.stft_cmask_istft_iq, (x, g(75), 75), r"bhw\.stft_cmask_istft_iq_mixed takes it"),
        (bhw.stft_mask_istft_iq_mixed, (x, g(512, False), 512), r"512 is a power of two: bhw\.stft_mask_istft_iq takes it"),
        (bhw.stft_cmask_istft_iq_mixed, (x, g(16), 16), r"bhw\.stft_cmask_istft_iq takes it"),
        (bhw.stft_cmask_istft_iq, (big, g(4096), 4096), r"got 4096: no fused I/Q transform takes it \(the three-call route"),
        (bhw.stft_mask_istft_iq_mixed, (big, g(2160, False), 2160), r"got 2160: no fused I/Q transform takes it \(the three-call route"),
        (bhw.stft_cmask_istft_iq_mixed, (big, g(4096), 4096), r"the three-call route"),
    )
    for fn, args, text in cases:
        with pytest.raises(ValueError, match=text):
            fn(p, args[0], args[1], args[2], 160)
    for cg in (False, True):
        S._mask_iq_refusals(torch, x, g(512, cg), 512, cg, False)
        S._mask_iq_refusals(torch, x, g(400, cg), 400, cg, True)
        S._mask_iq_refusals(torch, x, g(2048, cg), 2048, cg, False)
        S._mask_iq_refusals(torch, x, g(2025, cg), 2025, cg, True)
    # the real-signal calls keep their refusal of complex input, and point here
    with pytest.raises(ValueError, match=r"I/Q input: bhw\.stft_iq, a multiply and bhw\.istft_iq\)"):
        S._mask_fft_refusals(torch, x, g(257, False), 512)
    for fn in (bhw.stft_mask_istft, bhw.stft_mask_istft_mixed, bhw.stft_cmask_istft, bhw.stft_cmask_istft_mixed):
        assert "_iq" in fn.__doc__ and "stft_" in fn.__doc__
