"""Every plan branch of the frame, overlap-add and spectra fronts against a reference: each case of tests/plan_cases.py (which
tests/test_plan_coverage.py proves to reach every class of every planner) runs through the library call and the from-table call, and
ALL of its output is compared bit for bit (NaN by position) with the restatement the front's own test file already has.  The
restatements are imported, not copied; inputs carry the IEEE special values where the front's own tests use them; the cases marked
`padded` write rows and signals with gaps behind them into a buffer of sentinels, so a row written twice or into a gap shows.
No tolerance appears here."""
import ctypes

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import plan_cases as PC
from test_gpu_stft import _same, _signal as _stft_signal, _v
from test_gpu_stft import _frames_ref as _stft_frames_ref, _ola_ref as _istft_ola_ref
from test_gpu_welch import _psd_ref, _segments_ref, _signal as _welch_signal
from test_gpu_csd import _csd_ref, _same_out, _spectra
from test_gpu_apply_frames import _expected as _frames_expected_pow2
from test_gpu_overlap_add import _expected as _ola_expected_pow2
from test_gpu_len import _frames_expected as _frames_expected_len, _ola_expected as _ola_expected_len
from test_gpu_f32 import _frames_ref as _f32_frames_ref, _ola_ref as _f32_ola_ref, _signal as _f32_signal

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-123.25)
ISENTINEL = -1234567


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _seed(cid):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(cid))


def _classes_hold(front, c, line):
    """The from-table line names the table kernel and is of the classes of the case (the direct form is the library call's)."""
    d = PC.parse(line)
    assert d["table"], line
    for name in c["classes"]:
        if "direct form" not in name:
            assert PC.FRONTS[front][1][name](c, d), (c["id"], name, line)


# ---- periodogram ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", PC.case_ids("psd"))
def test_periodogram(torch, cid):
    c = PC.case("psd", cid)
    nb, F, K, strided = c["B"], c["F"], c["K"], bool(c.get("strided"))
    rng = np.random.default_rng(_seed(cid))
    nfft, scale = PC._nfft(K), 1.0 / (3.7 * F)
    Yh = _spectra(rng, nb, F, K, True, pad=3 if strided else 0)      # inf / NaN / huge / tiny / signed-zero parts
    Yd = torch.from_numpy(Yh).cuda()
    Y = Yd[..., :K]
    want = _psd_ref(Yh[..., :K], scale, nfft, True)
    if strided:
        big = torch.full((nb, K + 5), float(SENTINEL), device="cuda")
        got = bhw.welch_psd(Y, scale, nfft=nfft, onesided=True, out=big[:, :K])
        assert bool((big[:, K:] == float(SENTINEL)).all()), cid
    else:
        got = bhw.welch_psd(Y, scale, nfft=nfft, onesided=True)
    assert got.shape == (nb, K) and _same(got.cpu().numpy(), want), (cid, PC.psd_line(c))


# ---- cross spectra -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", PC.case_ids("csd"))
def test_cross_spectra(torch, cid):
    c = PC.case("csd", cid)
    nb, F, K, outs = c["B"], c["F"], c["K"], c["outputs"]
    rng = np.random.default_rng(_seed(cid))
    nfft, scale = PC._nfft(K), 0.37 / F
    Xh, Yh = _spectra(rng, 1 if c.get("broadcast") else nb, F, K, True, pad=3), _spectra(rng, nb, F, K, True, pad=5)
    Xd, Yd = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
    X, Y = (Xd[0, :, :K] if c.get("broadcast") else Xd[..., :K]), Yd[..., :K]
    want = _csd_ref(Xh[..., :K], Yh[..., :K], scale, nfft, True)
    bigs = {n: torch.full((nb, K + 5), float(SENTINEL), device="cuda", dtype=torch.complex64 if B.CSD_OUTPUTS[n][1] else torch.float32)
            for n in outs}
    got = bhw.welch_csd(X, Y, scale, nfft=nfft, onesided=True, outputs=outs, out={n: bigs[n][:, :K] for n in outs})
    assert tuple(got) == tuple(outs)
    for name in outs:
        assert _same_out(bigs[name][:, :K], want[name]), (cid, name, PC.csd_line(c))
        assert bool((bigs[name][:, K:] == float(SENTINEL)).all()), (cid, name, "gaps")


# ---- STFT frames and Welch segments --------------------------------------------------------------------------------------------------

def _strided_rows(a, nb, stride, width):
    """Rows of `width` elements `stride` apart in the flat array a, as a view."""
    return np.lib.stride_tricks.as_strided(a, shape=(nb, width), strides=(stride * a.itemsize, a.itemsize))


def _pack_x(torch, x, s):
    """x (B, T, C) on the device with the signals s.x_stride floats apart, NaN in the gaps."""
    nb = x.shape[0]
    flat = np.full(nb * s.x_stride, np.nan, dtype=np.float32)
    _strided_rows(flat, nb, s.x_stride, x.shape[1] * x.shape[2])[:] = x.reshape(nb, -1)
    return torch.from_numpy(flat).cuda()


def _check_rows(buf, s, frames, want, tag):
    """The whole of y: every row of every signal against `want` (B, frames, n_fft, C), and every gap still the sentinel."""
    nb, ys, ybs, live = s.batch, s.y_stride, s.y_batch_stride, s.n_fft * s.channels
    rows = np.lib.stride_tricks.as_strided(buf, shape=(nb, frames, ys), strides=(ybs * 4, ys * 4, 4))
    assert _same(rows[:, :, :live], want.reshape(nb, frames, live)), tag
    assert np.all(rows[:, :, live:] == SENTINEL), (tag, "gap behind a row")
    assert np.all(_strided_rows(buf[frames * ys:], nb, ybs, ybs - frames * ys) == SENTINEL), (tag, "gap behind a signal")


@pytest.mark.parametrize("cid", PC.case_ids("stft"))
def test_stft_frames(torch, cid):
    c = PC.case("stft", cid)
    p = PC.params(c["setup"])
    s, L, frames, col0, pad = PC.stft_desc(c)
    rng = np.random.default_rng(_seed(cid))
    x = _stft_signal(rng, (c["B"], c["T"], c["C"]))
    want = _stft_frames_ref(x, _v(p, L), c["n_fft"], c["hop"], col0, pad, c["mode"])
    assert want.shape[1] == frames
    xd = _pack_x(torch, x, s)
    st, dev = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), torch.cuda.current_device()
    yd = torch.full((s.batch * s.y_batch_stride,), float(SENTINEL), device="cuda")
    B.check(B.lib().bhw_stft_frames_f32_device(ctypes.byref(p), L, dev, st, ctypes.byref(s), ctypes.c_void_p(xd.data_ptr()),
                                               ctypes.c_void_p(yd.data_ptr())))
    _check_rows(yd.cpu().numpy(), s, frames, want, (cid, PC.stft_line(c)))
    with bhw.ResidentTable(p) as tab:
        _classes_hold("stft", c, PC.stft_line(c, table=tab.handle))
        yd.fill_(float(SENTINEL))
        B.check(B.lib().bhw_stft_frames_f32_from_table(tab.handle, ctypes.byref(p), L, st, ctypes.byref(s), ctypes.c_void_p(xd.data_ptr()),
                                                       ctypes.c_void_p(yd.data_ptr())))
        _check_rows(yd.cpu().numpy(), s, frames, want, (cid, "table"))


def _segments_ref_in_chunks(x, v, nfft, hop, rows_per_chunk=1 << 18):
    """_segments_ref over the rows of one long signal in chunks (its mean restatement holds 64 binary64 partial sums per row)."""
    nb, T, C = x.shape
    L = len(v)
    F = 1 + (T - L) // hop
    if nb * F * C <= rows_per_chunk:
        return _segments_ref(x, v, nfft, hop, True)
    assert nb == 1
    out = np.empty((1, F, nfft, C), dtype=np.float32)
    for r0 in range(0, F, rows_per_chunk):
        r1 = min(F, r0 + rows_per_chunk)
        out[:, r0:r1] = _segments_ref(x[:, r0 * hop:(r1 - 1) * hop + L], v, nfft, hop, True)      # rows r0 .. r1 - 1 and no other
    return out


@pytest.mark.parametrize("cid", PC.case_ids("welch"))
def test_welch_segments(torch, cid):
    c = PC.case("welch", cid)
    p = PC.params(c["setup"])
    s, L, F = PC.welch_desc(c)
    rng = np.random.default_rng(_seed(cid))
    x = _welch_signal(rng, (c["B"], c["T"], c["C"]), special=True, offset=3e4)
    want = _segments_ref_in_chunks(x, _v(p, L), c["n_fft"], c["hop"])
    assert want.shape[1] == F
    xd = _pack_x(torch, x, s)
    st, dev = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), torch.cuda.current_device()
    yd = torch.full((s.batch * s.y_batch_stride,), float(SENTINEL), device="cuda")
    need = int(B.lib().bhw_welch_workspace_bytes(ctypes.byref(s), B.WELCH_DETREND_CONSTANT))
    assert need == c["B"] * F * c["C"] * 4
    ws = torch.empty(need // 4, dtype=torch.float32, device="cuda")
    tail = (ctypes.byref(s), B.WELCH_DETREND_CONSTANT, ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(yd.data_ptr()),
            ctypes.c_void_p(ws.data_ptr()), need)
    B.check(B.lib().bhw_welch_frames_f32_device(ctypes.byref(p), L, dev, st, *tail))
    _check_rows(yd.cpu().numpy(), s, F, want, (cid, PC.welch_line(c)))
    with bhw.ResidentTable(p) as tab:
        _classes_hold("welch", c, PC.welch_line(c, table=tab.handle))
        yd.fill_(float(SENTINEL))
        ws.fill_(7.0)
        B.check(B.lib().bhw_welch_frames_f32_from_table(tab.handle, ctypes.byref(p), L, st, *tail))
        _check_rows(yd.cpu().numpy(), s, F, want, (cid, "table"))


# ---- frames kernels: int32 power of two, int32 any length, float32 ---------------------------------------------------------------------

@pytest.mark.parametrize("cid", PC.case_ids("frames"))
def test_frames_kernels(torch, cid):
    c = PC.case("frames", cid)
    p = PC.params(c["setup"])
    kind, L, frames, hop, C = c["kind"], c["L"], c["frames"], c["hop"], c["C"]
    shift = p.dat_width - 1
    length = None if kind == "pow2" else L
    rng = np.random.default_rng(_seed(cid))
    n = ((frames - 1) * hop + L) * C
    live = L * C
    stride = live + 6 if c.get("padded") else live
    if kind == "f32":
        xh = _f32_signal(rng, n)
        want = _f32_frames_ref(xh, _v(p, L), hop, frames, C).reshape(frames, live)
        sentinel, dtype = float(SENTINEL), torch.float32
    else:
        xh = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
        w = bhw.generate(p, 0, L, length=length).cpu().numpy()
        want = (_frames_expected_pow2(w, xh, frames, hop, C, shift).reshape(frames, live) if kind == "pow2" else
                _frames_expected_len(w, xh, hop, frames, C, shift, live))
        sentinel, dtype = ISENTINEL, torch.int32
    x = torch.from_numpy(xh).cuda()

    def check(call, tag):
        out = torch.full((frames, stride), sentinel, dtype=dtype, device="cuda")
        call(p, x, hop, frames=frames, channels=C, shift=shift, y_stride=stride, length=length, out=out)
        got = out.cpu().numpy()
        if kind == "f32":
            assert _same(got[:, :live], want), tag
        else:
            assert np.array_equal(got[:, :live], want), tag
        assert np.all(got[:, live:] == sentinel), (tag, "gap behind a row")

    check(bhw.apply_frames, (cid, PC.frames_line(c)))
    with bhw.ResidentTable(p) as tab:
        _classes_hold("frames", c, PC.frames_line(c, table=tab.handle))
        check(tab.apply_frames, (cid, "table"))


# ---- overlap-add kernels ---------------------------------------------------------------------------------------------------------------

def _forced(torch, table, p, o, y, x, q, rx):
    B.check(B.lib().bhw_dbg_overlap_add_shape(table, ctypes.byref(p), y.device.index, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                                              ctypes.byref(o), ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(x.data_ptr()), q, rx))


def _one_term_overlap_add(torch, c, p):
    """hop = L: every output has one term, so the reference is exact and cheap on the device: the binary64 product of two float32
    values is exact, rounded once to float32; with the envelope division the binary64 quotient (y v) / (v v), +0.0 where v = 0, rounded
    once -- the arithmetic of test_gpu_f32._ola_ref, which the first and the last frames are also handed to on the host."""
    L, frames, normalize = c["L"], c["frames"], c["normalize"]
    assert c["hop"] == L and c["C"] == 1
    vh = _v(p, L)
    v64 = torch.from_numpy(vh.astype(np.float64)).cuda()
    g = torch.Generator(device="cuda").manual_seed(_seed(c["id"]))
    y = torch.randn((frames, L), device="cuda", generator=g) * 1000.0
    with bhw.ResidentTable(p) as tab:
        _classes_hold("ola", c, PC.ola_line(c, table=tab.handle))
        for call, tag in ((bhw.overlap_add, "library"), (tab.overlap_add, "table")):
            x = call(p, y, L, length=L, normalize=normalize).view(frames, L)
            step = 1 << 16
            for f0 in range(0, frames, step):                       # all of the output, a chunk of frames at a time
                S = y[f0:f0 + step].double() * v64 + 0.0            # the sum starts at +0.0: a product of -0.0 gives +0.0
                E = v64 * v64                                        # exact; the envelope of the one frame that reaches the output
                ref = (torch.where(E > 0, S / torch.where(E > 0, E, torch.ones_like(E)), torch.zeros_like(S)) if normalize else S).float()
                assert torch.equal(x[f0:f0 + step].view(torch.int32), ref.view(torch.int32)), (c["id"], tag, f0)
            for f0 in (0, frames - 64):                             # the device reference itself against the restatement
                yh = y[f0:f0 + 64].cpu().numpy()
                assert _same(x[f0:f0 + 64].cpu().numpy().reshape(-1, 1), _f32_ola_ref(yh[:, :, None], vh, L, 0, 64 * L, normalize)), (c["id"], tag)
            del x


@pytest.mark.parametrize("cid", PC.case_ids("ola"))
def test_overlap_add_kernels(torch, cid):
    c = PC.case("ola", cid)
    p = PC.params(c["setup"])
    kind, L, frames, hop, C, normalize = c["kind"], c["L"], c["frames"], c["hop"], c["C"], bool(c.get("normalize"))
    shift = p.dat_width - 1
    rng = np.random.default_rng(_seed(cid))
    if c.get("device_reference"):
        _one_term_overlap_add(torch, c, p)
        return
    if kind == "istft":
        s, _, _, col0, pad, T = PC.istft_desc(c)
        yh = _stft_signal(rng, (c["B"], frames, c["n_fft"], C), special=False)
        want = _istft_ola_ref(yh, _v(p, L), hop, col0, pad, T, normalize)
        yt = torch.from_numpy(yh).cuda()
        yt = torch.view_as_complex(yt) if C == 2 else yt[..., 0]
        with bhw.ResidentTable(p) as tab:
            _classes_hold("ola", c, PC.ola_line(c, table=tab.handle))
            for call, tag in ((bhw.istft_overlap_add, PC.ola_line(c)), (tab.istft_overlap_add, "table")):
                got = call(p, yt, c["n_fft"], hop, win_length=L, center=True, normalize=normalize)
                got = (torch.view_as_real(got) if C == 2 else got[..., None]).cpu().numpy()
                assert _same(got, want), (cid, tag)
        return
    live = L * C
    stride = live + 6 if c.get("padded") else live
    count = (frames - 1) * hop + L
    length = None if kind == "pow2" else L
    if kind == "f32":
        rows = rng.standard_normal((frames, stride)).astype(np.float32)
        rows[:, live:] = np.nan                                     # the padding is never read
        want = _f32_ola_ref(rows[:, :live].reshape(frames, L, C), _v(p, L), hop, 0, count, normalize)
    else:
        rows = rng.integers(-2 ** 31, 2 ** 31, size=(frames, stride), dtype=np.int64).astype(np.int32)
        w = bhw.generate(p, 0, L, length=length).cpu().numpy()
        want = (_ola_expected_pow2 if kind == "pow2" else _ola_expected_len)(w, rows, hop, C, shift)
    y = torch.from_numpy(rows).cuda()
    kw = dict(channels=C, shift=shift, y_stride=stride, length=length)
    if kind == "f32":
        kw["normalize"] = normalize
    with bhw.ResidentTable(p) as tab:
        if "force" in c:                                            # a forced plan shape shows in no describe line
            o = PC.ola_desc(c)
            for table, tag in ((None, "library"), (tab.handle, "table")):
                x = torch.full((count, C), ISENTINEL, dtype=torch.int32, device="cuda")
                _forced(torch, table, p, o, y, x, *c["force"])
                assert np.array_equal(x.cpu().numpy(), want), (cid, tag)
            return
        _classes_hold("ola", c, PC.ola_line(c, table=tab.handle))
        for call, tag in ((bhw.overlap_add, PC.ola_line(c)), (tab.overlap_add, "table")):
            got = call(p, y, hop, **kw).cpu().numpy().reshape(count, C)
            assert (_same(got, want) if kind == "f32" else np.array_equal(got, want)), (cid, tag)
