"""Welch cross spectra (bhw_welch_csd_workspace_bytes / bhw_welch_csd_f32 / bhw_describe_csd): the checks that need no GPU -- exports
and declarations, the pinned descriptor, every argument error before any HIP call, the workspace sizes, the describe line and the
Python surface."""
import ctypes
import inspect
import os
import re

import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, WORKSPACE = -1, -4
NEW_SYMBOLS = ("bhw_welch_csd_workspace_bytes", "bhw_welch_csd_f32", "bhw_describe_csd")
ALL = ("pxy", "pxx", "pyy", "coherence", "h1")
# never dereferenced: every call below fails before any HIP call
XA, YA, W = 0x10000000, 0x80000000, 0x4000000000
OUTS = {"pxy": 0x100000000, "pxx": 0x110000000, "pyy": 0x120000000, "coherence": 0x130000000, "h1": 0x140000000}


def _err():
    return B.lib().bhw_last_error().decode()


def _csd(**kw):
    a = dict(batch=2, frames=300, bins=257, n_fft=512, scale=0.5, onesided=True, outputs=ALL)
    a.update(kw)
    return B.make_csd(a.pop("batch"), a.pop("frames"), a.pop("bins"), a.pop("n_fft"), a.pop("scale"), **a)


def _call(d, X=XA, Y=YA, ws=W, ws_bytes=1 << 30, **outs):
    p = dict(OUTS)
    p.update(outs)
    vp = ctypes.c_void_p
    return B.lib().bhw_welch_csd_f32(0, None, ctypes.byref(d) if d is not None else None, vp(X), vp(Y),
                                     *[vp(p[n]) for n in ALL], vp(ws), ws_bytes)


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\b(int|uint64_t) " + name + r"\(", header), name
    for line in ("#define BHW_CSD_ONESIDED 1u", "#define BHW_CSD_BROADCAST_X 2u", "#define BHW_CSD_PXY 0x10u", "#define BHW_CSD_PXX 0x20u",
                 "#define BHW_CSD_PYY 0x40u", "#define BHW_CSD_COHERENCE 0x80u", "#define BHW_CSD_H1 0x100u"):
        assert line in header, line
    assert (B.CSD_ONESIDED, B.CSD_BROADCAST_X, B.CSD_PXY, B.CSD_PXX, B.CSD_PYY, B.CSD_COHERENCE, B.CSD_H1) == (1, 2, 0x10, 0x20, 0x40, 0x80, 0x100)
    assert L.bhw_abi_version() == 4                                  # additions only


def test_descriptor_layout_is_pinned():
    assert ctypes.sizeof(B.BhwCsd) == 96
    offs = {n: getattr(B.BhwCsd, n).offset for n, _ in B.BhwCsd._fields_}
    assert offs == dict(struct_size=0, flags=4, batch=8, frames=16, bins=24, n_fft=32, x_stride=40, x_batch_stride=48, y_stride=56,
                        y_batch_stride=64, o_stride=72, scale=80, reserved=88)
    assert _csd().struct_size == 96
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        assert "sizeof(bhw_csd) = 96" in fh.read()


def test_argument_errors_before_any_hip_call():
    cases = [
        (dict(batch=0), "is 0"), (dict(frames=0), "is 0"), (dict(bins=0), "is 0"),
        (dict(n_fft=0), "n_fft"), (dict(n_fft=(1 << 31) + 1, bins=5, onesided=False), "n_fft"),
        (dict(bins=513, onesided=False), "above n_fft"),
        (dict(bins=256), "BHW_CSD_ONESIDED needs bins"),
        (dict(scale=float("inf")), "not finite"), (dict(scale=float("nan")), "not finite"),
        (dict(x_stride=256), "x_stride"), (dict(y_stride=256), "y_stride"),
        (dict(x_batch_stride=299 * 257 + 256), "x_batch_stride"), (dict(y_batch_stride=299 * 257 + 256), "y_batch_stride"),
        (dict(o_stride=256), "o_stride"),
        (dict(batch=1 << 17, frames=1 << 10, bins=513, n_fft=1024), "2^34"),
        (dict(batch=1 << 33, frames=1, bins=1, n_fft=1), "2^31 - 1 workgroups"),
        (dict(broadcast_x=True, x_batch_stride=300 * 257), "BHW_CSD_BROADCAST_X"),
    ]
    for kw, text in cases:
        rc = _call(_csd(**kw))
        assert rc == BADARG and text in _err(), (kw, rc, _err())
    d = _csd()
    d.struct_size = 88
    assert _call(d) == BADARG and "struct_size" in _err()
    d = _csd()
    d.reserved = 1
    assert _call(d) == BADARG and "reserved" in _err()
    d = _csd()
    d.flags |= 0x200
    assert _call(d) == BADARG and "flags 0x" in _err()
    d = _csd()
    d.flags |= 4
    assert _call(d) == BADARG and "flags 0x" in _err()
    d = _csd()
    d.flags &= 3
    assert _call(d) == BADARG and "output mask is empty" in _err()
    assert _call(None) == BADARG and "descriptor is NULL" in _err()
    d = _csd()                                                       # (a call that passes every check would reach HIP: none is made here)
    assert _call(d, X=0) == BADARG and "NULL" in _err()
    assert _call(d, Y=0) == BADARG and "NULL" in _err()
    assert _call(d, X=XA + 4) == BADARG and "8-byte aligned" in _err()
    assert _call(d, Y=YA + 4) == BADARG and "8-byte aligned" in _err()
    # a requested output: NULL, misaligned (8 bytes for the complex ones, 4 for the others), inside an input, another output, the workspace
    for n in ALL:
        assert _call(d, **{n: 0}) == BADARG and "NULL" in _err() and "requested" in _err(), n
        mis = 4 if n in ("pxy", "h1") else 2
        assert _call(d, **{n: OUTS[n] + mis}) == BADARG and f"{8 if n in ('pxy', 'h1') else 4}-byte aligned" in _err(), (n, _err())
        assert _call(d, **{n: XA + 64}) == BADARG and "overlap" in _err() and "d_X" in _err(), (n, _err())
        assert _call(d, **{n: YA + 64}) == BADARG and "overlap" in _err() and "d_Y" in _err(), (n, _err())
        assert _call(d, **{n: W + 64}) == BADARG and "workspace overlaps" in _err(), (n, _err())
        other = "pxx" if n != "pxx" else "pyy"
        assert _call(d, **{n: OUTS[other] + 8}) == BADARG and "overlap" in _err(), (n, _err())
    # ... and a pointer whose flag is not set is not looked at: with P_xy alone, the four others may be anything
    d1 = _csd(outputs=("pxy",), frames=200)
    assert _call(d1, pxy=0) == BADARG and "d_Pxy is NULL" in _err()
    assert _call(d1, pxy=XA) == BADARG and "overlap" in _err()
    # X and Y are only read: they may be the same tensor (csd(x, x)); the checks pass up to the workspace
    need = 2 * 2 * 257 * 4 * 8
    assert _call(d, Y=XA, ws_bytes=need - 1) == WORKSPACE
    assert _call(d, ws=0, ws_bytes=0) == BADARG and "workspace is NULL" in _err() and str(need) in _err()
    assert _call(d, ws=W + 4) == BADARG and "8-byte aligned" in _err()
    assert _call(d, ws_bytes=need - 1) == WORKSPACE and str(need) in _err()
    assert _call(d, ws=YA + 8) == BADARG and "workspace overlaps d_Y" in _err()
    assert _call(d, ws=XA + 8) == BADARG and "workspace overlaps d_X" in _err()
    # under broadcast X is one signal: an output just behind its F * K elements does not overlap it
    db = _csd(broadcast_x=True, outputs=("pxx",), frames=200)
    assert _call(db, pxx=XA + 200 * 257 * 8 - 4) == BADARG and "overlap" in _err()
    dn = _csd(outputs=("pxx",), frames=200)
    assert _call(dn, pxx=XA + 200 * 257 * 8) == BADARG and "overlap" in _err()          # not broadcast: X has two signals


def test_workspace_bytes():
    lib = B.lib()
    for outs, chains in ((("pxy",), 2), (("pxx",), 4), (("coherence",), 4), (("h1",), 4), (("pxy", "pyy"), 4), (ALL, 4)):
        for F, blocks in ((1, 1), (255, 1), (256, 1), (257, 2), (3 * 256 + 7, 4)):
            for bc in (False, True):
                d = _csd(batch=3, frames=F, bins=33, n_fft=64, outputs=outs, broadcast_x=bc)
                want = 0 if blocks == 1 else 3 * blocks * 33 * chains * 8
                assert lib.bhw_welch_csd_workspace_bytes(ctypes.byref(d)) == want, (outs, F, bc)
    assert lib.bhw_welch_csd_workspace_bytes(None) == 0
    assert lib.bhw_welch_csd_workspace_bytes(ctypes.byref(_csd(bins=256))) == 0         # a descriptor the checks refuse


def test_describe_names_form_plan_and_kernels():
    d = B.describe_csd(_csd())
    assert d.startswith("welch csd (one-sided, n_fft 512, pxy+pxx+pyy+coherence+h1): k_welch_csd<4,1>, 4 chains (S_xx, S_yy, C_re, C_im), "
                        "2 signals x 300 frames x 257 bins, 2 blocks of 256 frames"), d
    assert "grid 20 x 256 lanes (64 along the bins x 4 waves of 4 frames a pass, 32768 bytes of LDS), then k_welch_csd_join<4> in block order, " \
           "workspace 32896 bytes" in d, d
    d = B.describe_csd(_csd(outputs=("pxy",), frames=200, onesided=False, bins=512, broadcast_x=True))
    assert d.startswith("welch csd (two-sided, n_fft 512, pxy, X broadcast): k_welch_csd<2,0>, 2 chains (C_re, C_im)"), d
    assert "1 block of 256 frames" in d and "4 waves of 8 frames a pass, 32768 bytes of LDS" in d and "workspace 0 bytes" in d and "join" not in d
    d = B.describe_csd(_csd(outputs=("coherence",), frames=998, batch=64))
    assert "(one-sided, n_fft 512, coherence)" in d and "k_welch_csd<4,1>" in d and "grid 1280 x 256 lanes" in d
    buf = ctypes.create_string_buffer(64)
    assert B.lib().bhw_describe_csd(None, buf, 64) == BADARG and "descriptor is NULL" in _err()
    assert B.lib().bhw_describe_csd(ctypes.byref(_csd(o_stride=3)), buf, 64) == BADARG and "o_stride" in _err()
    assert B.lib().bhw_describe_csd(ctypes.byref(_csd()), None, 0) == BADARG


def test_output_selection_of_the_binding():
    assert B.csd_mask("pxy") == 0x10 and B.csd_mask(ALL) == 0x1F0 and B.csd_mask(("h1", "pxx")) == 0x120
    for bad in ((), ("pxy", "pxy"), ("pxz",), ("Pxy",)):
        with pytest.raises(ValueError, match="outputs"):
            B.csd_mask(bad)
    assert tuple(B.CSD_OUTPUTS) == ALL                               # the order of the pointers of bhw_welch_csd_f32


def test_python_surface():
    for name in ("welch_csd", "csd", "coherence", "transfer_function", "cross_spectra", "describe_csd", "BhwCsd"):
        assert hasattr(bhw, name), name
    for name in ("csd", "coherence", "transfer_function", "cross_spectra"):
        assert hasattr(bhw.ResidentTable, name), name
        for fn in (getattr(bhw, name), getattr(bhw.ResidentTable, name)):
            sig = inspect.signature(fn)
            names = [n for n in sig.parameters if n != "self"]
            assert names[:4] == ["params", "x", "y", "fs"] and sig.parameters["fs"].default == 1.0, name
            assert sig.parameters["length"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["length"].default is inspect.Parameter.empty
            assert sig.parameters["noverlap"].default is None and sig.parameters["nfft"].default is None
            assert sig.parameters["detrend"].default == "constant" and sig.parameters["return_onesided"].default is True
            assert sig.parameters["scaling"].default == "density" and sig.parameters["shift"].default is None
    sig = inspect.signature(bhw.welch_csd)
    assert list(sig.parameters)[:3] == ["X", "Y", "scale"] and sig.parameters["outputs"].default == ("pxy",)
    assert sig.parameters["nfft"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["onesided"].default is True
    assert "cross spectra" not in bhw.welch.__doc__.split("Not built")[1].split(".")[0]
