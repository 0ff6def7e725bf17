"""Weighted overlap-add on the GPU (bhw_overlap_add_device / bhw_overlap_add_from_table): bit-exact against numpy's wrapping int64
arithmetic (np.add.at) on the window bhw.generate returns, against the oracle window directly on a subset, as the transpose of
bhw_apply_frames_device, block by block through t0 / count, from resident tables in every format, in every forced plan shape, at
full size against torch's int64 arithmetic, under graph capture and from two streams at once."""
import ctypes
import itertools

import numpy as np
import pytest

import oracle_lib as O
import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

pytestmark = pytest.mark.gpu

WIN_OF_TERMS = {2: B.WIN_HANN, 3: B.WIN_BH3, 4: B.WIN_BH4, 5: B.WIN_BH5, 7: B.WIN_BH7}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _y(torch, frames, stride, seed, lo=-2 ** 31, hi=2 ** 31):
    rng = np.random.default_rng(seed)
    yh = rng.integers(lo, hi, size=(frames, stride), dtype=np.int64).astype(np.int32)
    return yh, torch.from_numpy(yh).cuda()


def _expected(w, yh, hop, C, shift, t0=0, count=None):
    """(count, C) int32: low32((sum of y * w over the frames reaching t) >> shift), the sum wrapping in numpy int64."""
    N = w.size
    frames = yh.shape[0]
    ext = (frames - 1) * hop + N
    count = ext - t0 if count is None else count
    prod = yh[:, :N * C].reshape(frames, N, C).astype(np.int64) * w.astype(np.int64)[None, :, None]
    acc = np.zeros((ext, C), dtype=np.int64)
    t = (np.arange(frames)[:, None] * hop + np.arange(N)[None, :]).ravel()
    np.add.at(acc, t, prod.reshape(-1, C))
    v = acc[t0:t0 + count] >> shift
    return (v & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _window(p):
    return bhw.generate(p, 0, 1 << p.phi_width).cpu().numpy()


def _lattice():
    """Models x rules x term counts x widths x phi_width, each with one rotated (hop, channels, shift, stride, range)."""
    out = []
    for i, (model, combine, nt, W, pw) in enumerate(itertools.product((B.MODEL_HLS, B.MODEL_CPP, B.MODEL_VHDL), (B.COMBINE_HLS, B.COMBINE_VHDL),
                                                                        (2, 3, 4, 5, 7), (8, 16, 24, 32), (4, 9, 12, 16))):
        N = 1 << pw
        hops = (1, 3, max(1, N // 4), N // 2, N, N + 5)
        out.append((model, combine, nt, W, pw, hops[i % 6], 1 + (i // 6) % 2, (0, W - 1, 62)[(i // 12) % 3], (i // 4) % 3 == 1, i % 5 == 2))
    return out


def test_sampled_lattice_is_bit_exact(torch):
    checked = 0
    for model, combine, nt, W, pw, hop, C, shift, padded, sub in _lattice():
        try:
            p = B.make_params(WIN_OF_TERMS[nt], pw, W, model=model, combine=combine, precision=3 if model == B.MODEL_VHDL else 1)
        except B.BhwError:
            continue                                  # a combination the library rejects for every call
        N = 1 << pw
        frames = 5 if pw < 16 else 3
        stride = N * C + (37 if padded else 0)
        yh, y = _y(torch, frames, stride, seed=checked)
        ext = (frames - 1) * hop + N
        t0, count = (ext // 3, ext // 3 + 1) if sub else (0, ext)
        x = bhw.overlap_add(p, y, hop, channels=C, shift=shift, t0=t0, count=count)
        assert tuple(x.shape) == ((count, 2) if C == 2 else (count,))
        want = _expected(_window(p), yh, hop, C, shift, t0, count).reshape(x.shape)
        assert np.array_equal(x.cpu().numpy(), want), (model, combine, nt, W, pw, hop, C, shift, padded, sub)
        checked += 1
    assert checked > 300


@pytest.mark.parametrize("model,W", [(B.MODEL_HLS, 32), (B.MODEL_CPP, 24), (B.MODEL_VHDL, 16)])
def test_against_the_oracle(torch, model, W):
    p = B.make_params(B.WIN_BH7, 10, W, model=model, combine=B.COMBINE_VHDL if model == B.MODEL_VHDL else B.COMBINE_HLS, precision=2)
    N, hop, frames = 1 << 10, 300, 9
    w = O.generate(O.from_bhw(p), 0, N)
    for C in (1, 2):
        yh, y = _y(torch, frames, N * C, seed=C)
        x = bhw.overlap_add(p, y, hop, channels=C, shift=W - 1)
        assert np.array_equal(x.cpu().numpy().reshape(-1, C), _expected(w, yh, hop, C, W - 1))


@pytest.mark.parametrize("pw,hop,C", [(10, 256, 1), (12, 1000, 2), (8, 3, 1), (9, 600, 1)])
def test_transpose_of_apply_frames(torch, pw, hop, C):
    """<overlap_add(y), s> == <y, apply_frames(s)> exactly with shift 0 and values small enough that nothing is truncated."""
    p = B.make_params(B.WIN_BH4, pw, 16)
    N, frames = 1 << pw, 7
    ext = (frames - 1) * hop + N
    yh, y = _y(torch, frames, N * C, seed=pw, lo=-8, hi=9)
    sh, s = _y(torch, 1, ext * C, seed=pw + 1, lo=-8, hi=9)
    x = bhw.overlap_add(p, y, hop, channels=C, shift=0).cpu().numpy().astype(np.int64).ravel()
    af = bhw.apply_frames(p, s.view(-1), hop, frames=frames, channels=C, shift=0).cpu().numpy().astype(np.int64).reshape(frames, -1)
    lhs = int(np.dot(x, sh.ravel().astype(np.int64)))
    rhs = int(np.sum(yh.astype(np.int64) * af))
    assert lhs == rhs and lhs != 0


@pytest.mark.parametrize("hop,C", [(1024, 1), (700, 2), (5, 1)])
def test_streaming_blocks_equal_one_call(torch, hop, C):
    """Outputs [T0, T1) from the frames that reach them (a frame sub-range passed as y, t0 relative to its first frame) equal the
    whole call, block by block."""
    p = B.make_params(B.WIN_BH7, 12, 32)
    N, frames = 1 << 12, 40 if hop > 100 else 300
    yh, y = _y(torch, frames, N * C, seed=hop)
    whole = bhw.overlap_add(p, y, hop, channels=C, shift=31)
    ext = (frames - 1) * hop + N
    blk = 3 * hop + 17
    parts = []
    for T0 in range(0, ext, blk):
        T1 = min(ext, T0 + blk)
        fa = max(0, -(-(T0 - N + 1) // hop))
        fb = min(frames - 1, (T1 - 1) // hop)
        parts.append(bhw.overlap_add(p, y[fa:fb + 1], hop, channels=C, shift=31, t0=T0 - fa * hop, count=T1 - T0))
    assert torch.equal(torch.cat(parts), whole)


def _table_weights(pw, W, model):
    sets = [B.make_params(B.WIN_BH7, pw, W, model=model)]
    for name in ("nuttall", "flat-top-2"):
        wt, _, aa = B.coeffs_preset(name, W)
        sets.append(B.make_params(wt, pw, W, model=model, aa=aa))
    return sets


@pytest.mark.parametrize("pw", [12, 26])
@pytest.mark.parametrize("model", [B.MODEL_HLS, B.MODEL_CPP])
def test_from_table_every_format(torch, pw, model):
    """Three weight sets over one table, for every table_format limit: the table kernel equals the library call.  The packed formats
    (delta16, residual, nibble, nibble + escapes with the cpp model) are taken by tiled tables at 32 bits (phi_width 26 here)."""
    W, N = 32, 1 << pw
    hop, frames = (N // 4 + 1, 6) if pw < 26 else (N // 2, 2)
    ps = _table_weights(pw, W, model)
    g = torch.Generator(device="cuda").manual_seed(pw + model)
    ys = {C: torch.randint(-2 ** 31, 2 ** 31, (frames, N * C), dtype=torch.int64, device="cuda", generator=g).int() for C in (1, 2)}
    seen = set()
    for fmt in (B.TABLE_BEST, B.TABLE_PLAIN, B.TABLE_DELTA16, B.TABLE_RESIDUAL, B.TABLE_NIBBLE, B.TABLE_NIBBLE_ESC):
        with bhw.ResidentTable(ps[0], table_format=fmt) as t:
            for i, p in enumerate(ps):
                C = 1 + (i + fmt) % 2
                d = t.describe_overlap_add(p, frames, hop, channels=C)
                assert d.startswith("overlap-add table: k_ola_table<"), d
                seen.add(d.split("<")[1].split(",")[0])
                got = t.overlap_add(p, ys[C], hop, channels=C, shift=W - 1)
                want = bhw.overlap_add(p, ys[C], hop, channels=C, shift=W - 1)
                assert torch.equal(got, want), (fmt, i)
    assert "0" in seen, seen
    if pw == 26:
        assert len(seen) >= 3, seen
        if model == B.MODEL_CPP:
            assert "5" in seen, seen                  # nibble + escapes


def _shape(torch, t, p, o, y, x, q, rx):
    B.check(B.lib().bhw_dbg_overlap_add_shape(t, ctypes.byref(p), y.device.index, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                                              ctypes.byref(o), ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(x.data_ptr()), q, rx))


@pytest.mark.parametrize("pw,hop,C", [(12, 1024, 1), (12, 3, 1), (10, 37, 2), (11, 1, 1), (9, 600, 2)])
def test_forced_plan_shapes_agree(torch, pw, hop, C):
    """Q = 1, the planner's Q, Q = 16, and the r-and-q lane layouts (1, 4, 64 lanes along r), direct and from a table, with a padded
    stride and a sub-range: one output."""
    p = B.make_params(B.WIN_BH5, pw, 24, model=B.MODEL_CPP)
    N, frames = 1 << pw, 9
    stride = N * C + 6
    yh, y = _y(torch, frames, stride, seed=pw + hop)
    ext = (frames - 1) * hop + N
    t0, count = ext // 5, ext - ext // 5 - 3
    want = torch.from_numpy(_expected(_window(p), yh, hop, C, 23, t0, count).ravel()).cuda()
    o = B.make_ola(frames, hop, count, t0=t0, channels=C, shift=23, y_stride=stride)
    with bhw.ResidentTable(p) as t:
        for table in (None, t.handle):
            for q, rx in ((0, 0), (1, 0), (16, 0), (0, 1), (3, 4), (0, 64), (1, 256)):
                x = torch.full((count * C,), 7, dtype=torch.int32, device="cuda")
                _shape(torch, table, p, o, y, x, q, rx)
                assert torch.equal(x, want), (table is None, q, rx)


def _torch_ola(torch, y, w, N, hop, shift, chunk=1024):
    frames = y.shape[0]
    ext = (frames - 1) * hop + N
    acc = torch.zeros(ext, dtype=torch.int64, device="cuda")
    wl = w.long()
    for f0 in range(0, frames, chunk):
        f1 = min(frames, f0 + chunk)
        idx = (torch.arange(f0, f1, device="cuda")[:, None] * hop + torch.arange(N, device="cuda")[None, :]).reshape(-1)
        acc.index_add_(0, idx, (y[f0:f1].long() * wl).reshape(-1))
    return (acc >> shift).int()


@pytest.mark.parametrize("pw,W,hop_div,frames", [(12, 32, 4, 1 << 14), (22, 32, 2, 16)])
def test_full_size(torch, pw, W, hop_div, frames):
    """S1 (BH-7 2^12 / 32 bits, hop N/4, 2^14 frames) and S4 (BH-7 2^22 / 32 bits, hop N/2, 16 frames) against torch's int64 products
    and index_add_ on the device, the library call and from a table."""
    p = B.make_params(B.WIN_BH7, pw, W)
    N = 1 << pw
    hop = N // hop_div
    g = torch.Generator(device="cuda").manual_seed(pw)
    y = torch.randint(-2 ** 31, 2 ** 31, (frames, N), dtype=torch.int64, device="cuda", generator=g).int()
    want = _torch_ola(torch, y, bhw.generate(p, 0, N), N, hop, W - 1, chunk=1024 if pw < 20 else 2)
    assert torch.equal(bhw.overlap_add(p, y, hop, shift=W - 1), want)
    with bhw.ResidentTable(p) as t:
        assert torch.equal(t.overlap_add(p, y, hop, shift=W - 1), want)


def test_graph_capture(torch):
    """Both calls captured with no bhw_prepare_device: replay equals eager."""
    p = B.make_params(B.WIN_BH7, 13, 32)
    N, hop, frames = 1 << 13, 1 << 11, 64
    yh, y = _y(torch, frames, N, seed=11)
    want = torch.from_numpy(_expected(_window(p), yh, hop, 1, 31).ravel()).cuda()
    with bhw.ResidentTable(p) as t:
        x = torch.zeros_like(want)
        t.overlap_add(p, y, hop, shift=31, out=x)          # warm-up outside the capture (torch's own allocator)
        assert torch.equal(x, want)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s):
            t.overlap_add(p, y, hop, shift=31, out=x)
        for _ in range(2):
            x.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(x, want)
    p2 = B.make_params(B.WIN_BH4, 13, 24, model=B.MODEL_CPP)
    assert B.describe_ola(p2, frames, hop).startswith("overlap-add direct: k_ola_direct")
    want2 = torch.from_numpy(_expected(_window(p2), yh, hop, 1, 23).ravel()).cuda()
    x2 = torch.zeros_like(want2)
    s = torch.cuda.Stream()
    graph2 = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph2, stream=s):
        bhw.overlap_add(p2, y, hop, shift=23, out=x2)
    for _ in range(2):
        x2.zero_()
        graph2.replay()
        torch.cuda.synchronize()
        assert torch.equal(x2, want2)


def test_two_streams_one_table(torch):
    p = B.make_params(B.WIN_BH7, 16, 32)
    wt, _, aa = B.coeffs_preset("nuttall", 32)
    q = B.make_params(wt, 16, 32, aa=aa)
    N, hop, frames = 1 << 16, 1 << 15, 48
    yh, y = _y(torch, frames, N, seed=12)
    wp = torch.from_numpy(_expected(_window(p), yh, hop, 1, 31).ravel()).cuda()
    wq = torch.from_numpy(_expected(_window(q), yh, hop, 1, 31).ravel()).cuda()
    with bhw.ResidentTable(p) as t:
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        outs = [torch.zeros_like(wp) for _ in range(2)]
        torch.cuda.synchronize()
        for _ in range(3):
            for s, o, pp in zip(streams, outs, (p, q)):
                with torch.cuda.stream(s):
                    t.overlap_add(pp, y, hop, shift=31, out=o)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], wp) and torch.equal(outs[1], wq)


def test_gaps_are_zero_and_taylor_is_unsupported(torch):
    p = B.make_params(B.WIN_HANN, 8, 16)
    N, hop, frames = 1 << 8, (1 << 8) + 40, 4
    yh, y = _y(torch, frames, N, seed=3)
    x = bhw.overlap_add(p, y, hop, shift=15).cpu().numpy()
    assert np.array_equal(x, _expected(_window(p), yh, hop, 1, 15).ravel())
    for f in range(frames - 1):
        assert (x[f * hop + N:(f + 1) * hop] == 0).all()
    for st, win in ((B.SIN_TAYLOR, B.WIN_HANN), (B.SIN_TAYLOR_ALL, B.WIN_BH7)):
        t = B.make_params(win, 8, 16, sin_type=st)
        with pytest.raises(B.BhwError) as e:
            bhw.overlap_add(t, y, hop)
        assert e.value.code == -2
