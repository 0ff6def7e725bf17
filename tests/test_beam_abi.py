"""The fused multichannel filter-and-sum calls of both families (bhw_beam_fft_f32_* / bhw_beam_mfft_f32_* and their describe calls):
the checks that need no GPU -- exports and declarations held to the complex-gain calls' with the four additions, every refusal of
include/bhw.h before any HIP call with its order and text, the complex-gain calls' refusals in their order about "the fused
beamformer", n_ch and the channel strides, the extents with the channel axis, the alignment, the wrap and the overlaps of d_out with
every channel of d_x and with d_g, samples 0, and the Python refusals raised before a device is asked for."""
import ctypes
import os
import re

import pytest
import torch

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, UNSUPPORTED = 0, -1, -2
# never dereferenced: every call below fails or has nothing to do
X, G, O = 0x10000000, 0x40000000, 0x80000000
F, NB, T, C = 101, 4, 16000, 3
FAM = {
    "fft": dict(n_fft=512, L=400, col0=56, pad=256, K=257, other="bhw_beam_mfft_f32_*", other_n=(400, 0, 200)),
    "mfft": dict(n_fft=400, L=400, col0=0, pad=200, K=201, other="bhw_beam_fft_f32_*", other_n=(512, 56, 256)),
}
FAMS = list(FAM)
NEW_SYMBOLS = tuple(n for fam in FAM for n in (f"bhw_beam_{fam}_f32_device", f"bhw_beam_{fam}_f32_from_table", f"bhw_describe_beam_{fam}"))


def _err():
    return B.lib().bhw_last_error().decode()


def _desc(fam, analysis, **kw):
    """4 signals of 16000 samples, 101 frames at hop 160, window 400, centred; the analysis side padded by reflection."""
    f = FAM[fam]
    a = dict(batch=NB, samples=T, frames=F, hop=160, n_fft=f["n_fft"], col0=f["col0"], pad=f["pad"], shift=31)
    if analysis:
        a["pad_mode"] = B.PAD_REFLECT
    a.update(kw)
    return B.make_stft(a.pop("batch"), a.pop("samples"), a.pop("frames"), a.pop("hop"), a.pop("n_fft"), **a)


def _calls(fam, sa, ss, flags=1, L=400, x=X, g=G, out=O, n_ch=C, xcs=0, gs=None, gcs=None, gbs=None):
    """The device form, the table form with a NULL table (the checks come first) and the describe call."""
    K = FAM[fam]["K"]
    gs = K if gs is None else gs
    gcs = F * K if gcs is None else gcs
    gbs = n_ch * gcs if gbs is None else gbs
    lib = B.lib()
    dev, tab = getattr(lib, f"bhw_beam_{fam}_f32_device"), getattr(lib, f"bhw_beam_{fam}_f32_from_table")
    vp = ctypes.c_void_p
    return (lambda p: dev(p, L, 0, None, ctypes.byref(sa), ctypes.byref(ss), flags, vp(x), n_ch, xcs, vp(g), gs, gcs, gbs, vp(out)),
            lambda p: tab(None, p, L, None, ctypes.byref(sa), ctypes.byref(ss), flags, vp(x), n_ch, xcs, vp(g), gs, gcs, gbs, vp(out)))


def _refused(fam, code, *words, **kw):
    p = B.make_params(B.WIN_BH4, 24, 32)
    sa, ss = kw.pop("sa", None) or _desc(fam, True), kw.pop("ss", None) or _desc(fam, False)
    for call in _calls(fam, sa, ss, **kw):
        assert call(ctypes.byref(p)) == code, (kw, _err())
        assert all(w in _err() for w in words), (words, _err())


def test_the_six_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    assert len(NEW_SYMBOLS) == 6 and B.BEAM_MAX_CH == 64 and "#define BHW_BEAM_MAX_CH 64u" in header
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS and hasattr(L, name), name
        cm = name.replace("beam", "cmask")
        new = " ".join(re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1).split())
        old = " ".join(re.search(r"\bint " + cm + r"\(([^;]*)\);", header).group(1).split())
        # the declaration is the complex-gain call's with n_ch and x_ch_stride behind d_x and g_ch_stride between the gain strides
        if "describe" in name:
            want = old.replace("uint64_t g_stride, uint64_t g_batch_stride", "uint32_t n_ch, uint64_t x_ch_stride, uint64_t g_stride, "
                               "uint64_t g_ch_stride, uint64_t g_batch_stride")
        else:
            want = old.replace("const float *d_x,", "const float *d_x, uint32_t n_ch, uint64_t x_ch_stride,") \
                      .replace("uint64_t g_stride, uint64_t g_batch_stride", "uint64_t g_stride, uint64_t g_ch_stride, uint64_t g_batch_stride")
        assert new == want, name
        assert len(getattr(L, name).argtypes) == len(getattr(L, cm).argtypes) + 3
    assert L.bhw_abi_version() == 4
    for text in ("Z = P_0, then Z = fl32(Z + P_c)", "ascending channel order", "d_x + b * sa->x_stride + c * x_ch_stride",
                 "d_g + 2 * (b * g_batch_stride + c * g_ch_stride + f * g_stride)", "may not be 0 when n_ch > 1"):
        assert text in header, text
    for name in ("stft_beamform_istft", "stft_beamform_istft_mixed", "describe_beam_fft", "describe_beam_mfft", "BEAM_MAX_CH"):
        assert name in bhw.__all__ and hasattr(bhw, name), name


@pytest.mark.parametrize("fam", FAMS)
def test_refusals_that_name_the_route_that_takes_the_input(fam):
    f = FAM[fam]
    n, col0, pad = f["other_n"]
    iq = ("bhw_stft_cfft_f32_*", "bhw_istft_cfft_f32_*") if fam == "fft" else ("bhw_stft_cmfft_f32_*", "bhw_istft_cmfft_f32_*")
    cases = [(dict(channels=2), 400, iq),
             (dict(n_fft=n, col0=col0, pad=pad), 400, (f["other"],)),
             (dict(n_fft=4096, col0=0, pad=2048), 4096, ("bhw_stft_fft_f32_*", "bhw_istft_fft_f32_*")),
             (dict(n_fft=2160, col0=0, pad=1080), 2160, ("bhw_stft_mfft_f32_*", "bhw_istft_mfft_f32_*"))]
    cases += [(dict(n_fft=2000, col0=0, pad=1000), 2000, (f["other"],))] if fam == "fft" else [(dict(n_fft=2048, col0=0, pad=1024), 2048, (f["other"],))]
    p = B.make_params(B.WIN_BH4, 24, 32)
    for kw, L, names in cases:
        for sa, ss in ((_desc(fam, True, **kw), _desc(fam, False, **kw)), (_desc(fam, True), _desc(fam, False, **kw))):
            _refused(fam, UNSUPPORTED, "fused beamformer", *names, sa=sa, ss=ss, L=L)
            assert "mask" not in _err(), _err()
            buf = ctypes.create_string_buffer(1280)
            fn = getattr(B.lib(), f"bhw_describe_beam_{fam}")
            assert fn(None, ctypes.byref(p), L, ctypes.byref(sa), ctypes.byref(ss), 1, C, 0, f["K"], F * f["K"], 0, buf, 1280) == UNSUPPORTED


@pytest.mark.parametrize("fam", FAMS)
def test_the_checks_of_the_complex_gain_calls_come_first_and_in_their_words(fam):
    """What the complex-gain call refuses for (sa, ss, flags, the frame stride of the gains), this call refuses with the same code and
    the same text: the parents' refusals, the fields that must agree, g_stride."""
    K = FAM[fam]["K"]
    p = B.make_params(B.WIN_BH4, 24, 32)
    cm = getattr(B.lib(), f"bhw_cmask_{fam}_f32_device")
    vp = ctypes.c_void_p
    for akw, skw, gs in ((dict(hop=0), dict(hop=0), K), (dict(shift=63), dict(shift=63), K), (dict(frames=102), dict(frames=102), K),
                         (dict(x_stride=T - 1), {}, K), ({}, dict(hop=161), K), ({}, dict(col0=1), K), ({}, dict(batch=5), K),
                         ({}, dict(y_stride=4), K), ({}, {}, K - 1)):
        sa, ss = _desc(fam, True, **akw), _desc(fam, False, **skw)
        rc = cm(ctypes.byref(p), 400, 0, None, ctypes.byref(sa), ctypes.byref(ss), 1, vp(X), vp(G), gs, 0, vp(O))
        want = _err()
        assert rc in (BADARG, UNSUPPORTED), (akw, skw, gs)
        # with valid channel arguments, and with invalid ones: the earlier check speaks either way
        # (n_ch itself stands behind the fields the descriptors share and before g_stride)
        for n_ch, gcs in ((C, F * K), (0, 0))[:1 if gs < K else 2]:
            for call in _calls(fam, sa, ss, gs=gs, n_ch=n_ch, gcs=gcs, gbs=0):
                assert call(ctypes.byref(p)) == rc and _err() == want, (akw, skw, want, _err())
    # flags the inverse call does not know
    _refused(fam, BADARG, flags=1 << 9)


@pytest.mark.parametrize("fam", FAMS)
def test_the_channel_axis_its_order_and_text(fam):
    K = FAM[fam]["K"]
    rows = (F - 1) * K + K
    _refused(fam, BADARG, "n_ch 0: 1..64 channels a signal", n_ch=0)
    _refused(fam, BADARG, "n_ch 65: 1..64 channels a signal", n_ch=65)
    # n_ch comes before the gain strides, the channel strides behind g_stride, the pointers last
    _refused(fam, BADARG, "n_ch 0", n_ch=0, gs=K - 1, x=0)
    _refused(fam, BADARG, f"g_stride {K - 1}", gs=K - 1, xcs=T - 1)
    _refused(fam, BADARG, f"x_ch_stride {T - 1}: 0 (packed channels) or at least the analysis samples {T}", xcs=T - 1, gcs=0, x=0)
    _refused(fam, BADARG, f"x_stride {3 * T - 1} of the analysis descriptor: 0 (n_ch channel strides) or at least (n_ch - 1) * x_ch_stride + samples = "
             f"{3 * T}", sa=_desc(fam, True, x_stride=3 * T - 1), gcs=0)
    _refused(fam, BADARG, f"= {2 * (T + 7) + T}", sa=_desc(fam, True, x_stride=3 * T + 13), xcs=T + 7)
    _refused(fam, BADARG, "g_ch_stride 0 with n_ch 3", "sum of the channels of x", "bhw_cmask_*", gcs=0, gbs=0, x=0)
    _refused(fam, BADARG, f"g_ch_stride {rows - 1}: at least (frames - 1) * g_stride + K = {rows} pairs", gcs=rows - 1, gbs=0, x=0)
    _refused(fam, BADARG, f"g_ch_stride {K - 1}: at least (frames - 1) * g_stride + K = {K} pairs", gs=0, gcs=K - 1, gbs=0)
    _refused(fam, BADARG, f"g_batch_stride {3 * rows - 1}: 0 (the same gains for every signal) or at least (n_ch - 1) * g_ch_stride + (frames - 1) * "
             f"g_stride + K = {3 * rows} pairs", gcs=rows, gbs=3 * rows - 1, x=0)
    _refused(fam, BADARG, "g extent beyond 2^60", gcs=1 << 59, gbs=0)
    _refused(fam, BADARG, "x extent beyond 2^60", xcs=1 << 59)
    _refused(fam, BADARG, "d_x / d_g / d_out is NULL", x=0)
    _refused(fam, BADARG, "d_g is not 8-byte aligned", g=G + 4)
    _refused(fam, BADARG, "d_x is not 4-byte aligned", x=X + 2)
    _refused(fam, BADARG, "extent beyond 2^60", sa=_desc(fam, True, x_stride=1 << 59))
    # one channel: the channel stride of the gains is not used and may be 0; the call is the complex-gain call's
    p = B.make_params(B.WIN_BH4, 24, 32)
    for call in _calls(fam, _desc(fam, True), _desc(fam, False, samples=0), n_ch=1, gcs=0, gbs=0):
        assert call(ctypes.byref(p)) in (OK, BADARG)       # (the table form: "table is NULL" after the checks)
    text = getattr(B, f"describe_beam_{fam}")(p, 400, _desc(fam, True), _desc(fam, False), 1, normalize=True, g_stride=K, g_batch_stride=rows)
    assert ", complex gains: channels 1, " in text


@pytest.mark.parametrize("fam", FAMS)
def test_overlaps_count_every_channel_of_x_and_of_the_gains(fam):
    K = FAM[fam]["K"]
    rows = (F - 1) * K + K
    xe = (NB - 1) * C * T + (C - 1) * T + T                    # floats of x, packed
    ge = (NB - 1) * C * rows + (C - 1) * rows + rows           # pairs of g, packed
    _refused(fam, BADARG, "d_x and d_out overlap", out=X + 4 * (xe - 1))
    _refused(fam, BADARG, "d_x and d_out overlap", out=X + 4 * (C * T + T))            # the second channel of the second signal
    _refused(fam, BADARG, "d_x and d_out overlap", out=X - 4 * (NB * T - 1))
    _refused(fam, BADARG, "d_g and d_out overlap", out=G + 8 * ge - 4)
    _refused(fam, BADARG, "d_g and d_out overlap", out=G + 8 * (2 * rows))
    _refused(fam, BADARG, "wraps the address space", x=(1 << 64) - 4096)
    # padded channel strides widen the extents
    _refused(fam, BADARG, "d_x and d_out overlap", out=X + 4 * xe + 4 * 2 * 7, xcs=T + 7, sa=_desc(fam, True, x_stride=3 * (T + 7)))
    p = B.make_params(B.WIN_BH4, 24, 32)
    # right behind the last channel everything passes the checks: the table form then says that its table is NULL
    for out in (X + 4 * xe, G + 8 * ge):
        tab = _calls(fam, _desc(fam, True), _desc(fam, False), out=out)[1]
        assert tab(ctypes.byref(p)) == BADARG and "table is NULL" in _err(), _err()


@pytest.mark.parametrize("fam", FAMS)
def test_samples_zero_has_nothing_to_do(fam):
    p = B.make_params(B.WIN_BH4, 24, 32)
    sa, s0 = _desc(fam, True), _desc(fam, False, samples=0)
    dev = _calls(fam, sa, s0, x=0, g=0, out=0)[0]
    assert dev(ctypes.byref(p)) == OK, _err()                                   # BHW_OK with the pointers unchecked, and no device asked for
    assert _calls(fam, sa, s0, x=0, g=0, out=0, n_ch=0)[0](ctypes.byref(p)) == BADARG and "n_ch 0" in _err()
    text = getattr(B, f"describe_beam_{fam}")(p, 400, sa, s0, C)
    assert text.startswith(f"beam {fam} direct (") and "nothing (samples 0)" in text


def test_the_python_refusals_come_before_any_device_is_asked_for(monkeypatch):
    from blackman_harris_win_amd import selector as S

    def no_device():
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(S, "_torch", no_device)
    p = B.make_params(B.WIN_HANN, 10, 16)
    x = torch.zeros((2, 3, 1000))
    w = torch.ones((3, 33), dtype=torch.complex64)
    for call, tail, n, other_n in ((bhw.stft_beamform_istft, "", 64, 60), (bhw.stft_beamform_istft_mixed, "_mixed", 60, 64)):
        with pytest.raises(ValueError, match="takes complex64 weights, got torch.float32: real gains per channel are not built"):
            call(p, x, w.real.contiguous(), n, 16)
        with pytest.raises(ValueError, match=rf"the I/Q beamformer is not built \(bhw.stft_cmask_istft_iq{tail} per channel and a sum"):
            call(p, x.to(torch.complex64), w, n, 16)
        other = "bhw.stft_beamform_istft takes it" if tail else "bhw.stft_beamform_istft_mixed takes it"
        with pytest.raises(ValueError, match=other):
            call(p, x, w, other_n, 16)
        with pytest.raises(ValueError, match="bhw.stft, the weights and a sum over the channels, and bhw.istft take it"):
            call(p, x, w, 4096, 16)
        big = 2160 if tail else 2000
        with pytest.raises(ValueError, match="bhw.stft_mixed, the weights and a sum over the channels, and bhw.istft_mixed take it" if tail
                           else "bhw.stft_beamform_istft_mixed takes it"):
            call(p, x, w, big, 16)
        with pytest.raises(ValueError, match=r"x must be \(C, T\) or \(B, C, T\)"):
            call(p, x[0, 0], w, n, 16)
        with pytest.raises(ValueError, match="65 channels: the fused beamformer takes 1..64"):
            call(p, torch.zeros((65, 100)), torch.ones((65, 33), dtype=torch.complex64), n, 16)
        with pytest.raises(ValueError, match="broadcast along the channels"):
            call(p, x, w[0:1], n, 16)
        with pytest.raises(ValueError, match="broadcast along the channels"):
            call(p, x, w[0:1].expand(3, 33), n, 16)
        with pytest.raises(ValueError, match="broadcast along the channels"):
            call(p, x, torch.ones((2, 1, 5, 33), dtype=torch.complex64), n, 16)
        with pytest.raises(ValueError, match="have 2 channels, x has 3"):
            call(p, x, torch.ones((2, 33), dtype=torch.complex64), n, 16)
        with pytest.raises(ValueError, match=r"weights must be \(C, K\), \(C, F, K\) or"):
            call(p, x, torch.ones((33,), dtype=torch.complex64), n, 16)
