"""Overlapped-frame apply on the GPU (bhw_apply_frames_device / bhw_apply_frames_from_table): bit-exact against numpy's int64
arithmetic on the window bhw.generate returns (itself held to the oracle by the rest of the suite), against the oracle directly on a
subset, against one bhw_apply_device per frame, from resident tables in every format, with a padded output stride, at the headline
size, under graph capture and from two streams at once."""
import ctypes
import itertools

import numpy as np
import pytest

import oracle_lib as O
import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

pytestmark = pytest.mark.gpu

WIN_OF_TERMS = {2: B.WIN_HANN, 3: B.WIN_BH3, 4: B.WIN_BH4, 5: B.WIN_BH5, 7: B.WIN_BH7}
PER_FRAME, DIRECT = 2, 0          # BHWP_FRAMES_PER_FRAME, BHWP_FRAMES_DIRECT (bhw_plan.h)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _x(torch, frames, hop, N, C, seed):
    n = ((frames - 1) * hop + N) * C
    rng = np.random.default_rng(seed)
    xh = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
    return xh, torch.from_numpy(xh).cuda()


def _expected(w, xh, frames, hop, C, shift):
    """(frames, N, C) int32: low32((x * w[k]) >> shift) in numpy int64."""
    N = w.size
    idx = np.arange(frames)[:, None] * hop + np.arange(N)[None, :]
    xs = xh.reshape(-1, C)[idx].astype(np.int64)
    v = (xs * w.astype(np.int64)[None, :, None]) >> shift
    return (v & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _window(p):
    return bhw.generate(p, 0, 1 << p.phi_width).cpu().numpy()


def _lattice():
    """Models x rules x term counts x widths x phi_width, each with one (hop, channels, shift) of the issue's sets, rotated."""
    out = []
    for i, (model, combine, nt, W, pw) in enumerate(itertools.product((B.MODEL_HLS, B.MODEL_CPP, B.MODEL_VHDL), (B.COMBINE_HLS, B.COMBINE_VHDL),
                                                                        (2, 3, 4, 5, 7), (8, 16, 24, 32), (4, 9, 12, 16))):
        N = 1 << pw
        hops = (1, 3, max(1, N // 4), N // 2, N, N + 5)
        out.append((model, combine, nt, W, pw, hops[i % 6], 1 + (i // 6) % 2, (0, W - 1, 62)[(i // 12) % 3]))
    return out


def test_sampled_lattice_is_bit_exact(torch):
    checked = 0
    for model, combine, nt, W, pw, hop, C, shift in _lattice():
        try:
            p = B.make_params(WIN_OF_TERMS[nt], pw, W, model=model, combine=combine, precision=3 if model == B.MODEL_VHDL else 1)
        except B.BhwError:
            continue                                  # a combination the library rejects for every call
        N = 1 << pw
        frames = 5 if pw < 16 else 3
        xh, x = _x(torch, frames, hop, N, C, seed=checked)
        y = bhw.apply_frames(p, x, hop, frames=frames, channels=C, shift=shift)
        assert tuple(y.shape) == ((frames, N, 2) if C == 2 else (frames, N))
        want = _expected(_window(p), xh, frames, hop, C, shift).reshape(y.shape)
        assert np.array_equal(y.cpu().numpy(), want), (model, combine, nt, W, pw, hop, C, shift)
        checked += 1
    assert checked > 300


@pytest.mark.parametrize("sin_type,nt", [(B.SIN_TAYLOR, 2), (B.SIN_TAYLOR, 3), (B.SIN_TAYLOR_ALL, 5), (B.SIN_TAYLOR_ALL, 7)])
def test_taylor_sources_take_the_per_frame_route(torch, sin_type, nt):
    p = B.make_params(WIN_OF_TERMS[nt], 12, 16, sin_type=sin_type)
    N, hop, frames = 1 << 12, 1000, 6
    assert B.describe_frames(p, frames, hop).startswith("per-frame")
    xh, x = _x(torch, frames, hop, N, 1, seed=7)
    y = bhw.apply_frames(p, x, hop, shift=15)
    assert y.shape[0] == frames
    assert np.array_equal(y.cpu().numpy(), _expected(_window(p), xh, frames, hop, 1, 15)[:, :, 0])
    with pytest.raises(B.BhwError) as e:
        bhw.apply_frames(p, torch.zeros(2 * ((frames - 1) * hop + N), dtype=torch.int32, device="cuda"), hop, channels=2)
    assert e.value.code == -2


@pytest.mark.parametrize("model,W", [(B.MODEL_HLS, 32), (B.MODEL_CPP, 24), (B.MODEL_VHDL, 16)])
def test_against_the_oracle(torch, model, W):
    p = B.make_params(B.WIN_BH7, 10, W, model=model, combine=B.COMBINE_VHDL if model == B.MODEL_VHDL else B.COMBINE_HLS, precision=2)
    N, hop, frames = 1 << 10, 300, 9
    w = O.generate(O.from_bhw(p), 0, N)
    for C in (1, 2):
        xh, x = _x(torch, frames, hop, N, C, seed=C)
        y = bhw.apply_frames(p, x, hop, channels=C, shift=W - 1)
        assert np.array_equal(y.cpu().numpy().reshape(frames, N, C), _expected(w, xh, frames, hop, C, W - 1))


def _route(torch, p, f, x, y, route):
    dev = x.device.index
    B.check(B.lib().bhw_dbg_apply_frames_route(ctypes.byref(p), dev, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                                               ctypes.byref(f), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), route))


@pytest.mark.parametrize("pw,frames", [(12, 40), (18, 1), (18, 8)])
def test_each_frame_equals_the_existing_apply(torch, pw, frames):
    """Both routes of the planner -- the frames kernel and one bhw_apply_device per frame -- forced on the same shape, and the
    planner's own choice, against bhw_apply_device(p, n0 = 0, N, d_x + f * hop)."""
    p = B.make_params(B.WIN_BH7, pw, 32)
    N = 1 << pw
    hop = N // 2 + 3
    xh, x = _x(torch, frames, hop, N, 1, seed=pw + frames)
    want = torch.empty((frames, N), dtype=torch.int32, device="cuda")
    for i in range(frames):
        bhw.apply(p, x[i * hop:i * hop + N], shift=31, out=want[i])
    got = bhw.apply_frames(p, x, hop, shift=31)
    assert torch.equal(got, want)
    f = B.make_frames(frames, hop, shift=31)
    for route in (DIRECT, PER_FRAME):
        y = torch.full((frames, N), 7, dtype=torch.int32, device="cuda")
        _route(torch, p, f, x, y, route)
        assert torch.equal(y, want), route
    expect_route = "per-frame" if (pw >= 18 and frames < 3) else "frames kernel"      # BH-7 / 32 bits: the measured crossover
    assert B.describe_frames(p, frames, hop).startswith(expect_route)


def _table_weights(pw, W, model):
    sets = [B.make_params(B.WIN_BH7, pw, W, model=model)]
    for name in ("nuttall", "flat-top-2"):
        wt, _, aa = B.coeffs_preset(name, W)
        sets.append(B.make_params(wt, pw, W, model=model, aa=aa))
    return sets


@pytest.mark.parametrize("pw", [12, 16, 22, 26])
@pytest.mark.parametrize("model", [B.MODEL_HLS, B.MODEL_CPP])
def test_from_table_every_format(torch, pw, model):
    """Three weight sets over one table, for every table_format limit: the table kernel equals the library call.  The packed
    formats (delta16, residual, nibble, nibble + escapes) are taken by tiled tables at 32 bits (phi_width 26 here); below, plain."""
    W, N = 32, 1 << pw
    hop, frames = (N // 4 + 1, 6) if pw < 26 else (N // 2, 2)
    ps = _table_weights(pw, W, model)
    g = torch.Generator(device="cuda").manual_seed(pw + model)
    xs = {C: torch.randint(-2 ** 31, 2 ** 31, (((frames - 1) * hop + N) * C,), dtype=torch.int64, device="cuda", generator=g).int()
          for C in (1, 2)}
    seen = set()
    for fmt in (B.TABLE_BEST, B.TABLE_PLAIN, B.TABLE_DELTA16, B.TABLE_RESIDUAL, B.TABLE_NIBBLE, B.TABLE_NIBBLE_ESC):
        with bhw.ResidentTable(ps[0], table_format=fmt) as t:
            for i, p in enumerate(ps):
                C = 1 + (i + fmt) % 2
                d = t.describe_frames(p, frames, hop, channels=C)
                assert d.startswith("frames kernel: k_frames_table<"), d
                seen.add(d.split("<")[1].split(",")[0])
                got = t.apply_frames(p, xs[C], hop, channels=C, shift=W - 1)
                want = bhw.apply_frames(p, xs[C], hop, channels=C, shift=W - 1)
                assert torch.equal(got, want), (fmt, i)
    assert "0" in seen, seen
    if pw == 26:
        assert len(seen) >= 3, seen


@pytest.mark.parametrize("C", [1, 2])
def test_padded_stride_leaves_the_padding(torch, C):
    p = B.make_params(B.WIN_BH5, 11, 24)
    N, hop, frames = 1 << 11, 700, 7
    stride = N * C + 300
    xh, x = _x(torch, frames, hop, N, C, seed=3)
    out = torch.full((frames * stride,), -12345, dtype=torch.int32, device="cuda")
    y = bhw.apply_frames(p, x, hop, channels=C, y_stride=stride, out=out)
    assert tuple(y.shape) == (frames, stride)
    yh = y.cpu().numpy()
    assert np.array_equal(yh[:, :N * C].reshape(frames, N, C), _expected(_window(p), xh, frames, hop, C, 23))
    assert (yh[:, N * C:] == -12345).all()
    with bhw.ResidentTable(p) as t:
        out2 = torch.full((frames * stride,), -12345, dtype=torch.int32, device="cuda")
        assert torch.equal(t.apply_frames(p, x, hop, channels=C, y_stride=stride, out=out2), y)
    # an odd stride with two channels: the 4-byte form of the I/Q access
    if C == 2:
        out3 = torch.full((frames * (stride + 1),), -12345, dtype=torch.int32, device="cuda")
        y3 = bhw.apply_frames(p, x, hop, channels=2, y_stride=stride + 1, out=out3)
        assert torch.equal(y3[:, :stride], y)
        # and an x that is only 4-byte aligned
        xo = torch.empty(x.numel() + 1, dtype=torch.int32, device="cuda")[1:]
        xo.copy_(x)
        assert torch.equal(bhw.apply_frames(p, xo, hop, channels=2, y_stride=stride + 1, out=out3)[:, :stride], y)


def _torch_frames(torch, x, w, N, hop, frames, shift, chunk=1024):
    out = torch.empty((frames, N), dtype=torch.int32, device="cuda")
    wl = w.long()
    for f0 in range(0, frames, chunk):
        f1 = min(frames, f0 + chunk)
        xs = x[f0 * hop:(f1 - 1) * hop + N].unfold(0, N, hop).long()
        out[f0:f1] = ((xs * wl) >> shift).int()        # .int() keeps the low 32 bits
    return out


def test_headline_size(torch):
    """BH-7, N = 2^12, 32 bits, hop N/4, 2^14 frames (2^26 outputs): on the device against torch's int64 arithmetic."""
    p = B.make_params(B.WIN_BH7, 12, 32)
    N, hop, frames = 1 << 12, 1 << 10, 1 << 14
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randint(-2 ** 31, 2 ** 31, ((frames - 1) * hop + N,), dtype=torch.int64, device="cuda", generator=g).int()
    w = bhw.generate(p, 0, N)
    want = _torch_frames(torch, x, w, N, hop, frames, 31)
    assert torch.equal(bhw.apply_frames(p, x, hop, shift=31), want)
    with bhw.ResidentTable(p) as t:
        assert torch.equal(t.apply_frames(p, x, hop, shift=31), want)


def test_long_window_both_routes(torch):
    p = B.make_params(B.WIN_BH7, 22, 32)
    N, hop, frames = 1 << 22, 1 << 21, 4
    g = torch.Generator(device="cuda").manual_seed(6)
    x = torch.randint(-2 ** 31, 2 ** 31, ((frames - 1) * hop + N,), dtype=torch.int64, device="cuda", generator=g).int()
    want = _torch_frames(torch, x, bhw.generate(p, 0, N), N, hop, frames, 31, chunk=2)
    assert torch.equal(bhw.apply_frames(p, x, hop, shift=31), want)
    f = B.make_frames(frames, hop, shift=31)
    for route in (DIRECT, PER_FRAME):
        y = torch.zeros((frames, N), dtype=torch.int32, device="cuda")
        _route(torch, p, f, x, y, route)
        assert torch.equal(y, want), route


def test_graph_capture(torch):
    p = B.make_params(B.WIN_BH7, 13, 32)
    N, hop, frames = 1 << 13, 1 << 11, 64
    xh, x = _x(torch, frames, hop, N, 1, seed=11)
    want = torch.from_numpy(_expected(_window(p), xh, frames, hop, 1, 31)[:, :, 0]).cuda()
    with bhw.ResidentTable(p) as t:
        y = torch.zeros((frames, N), dtype=torch.int32, device="cuda")
        t.apply_frames(p, x, hop, shift=31, out=y)          # warm-up outside the capture (torch's own allocator)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        y.zero_()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s):
            t.apply_frames(p, x, hop, shift=31, out=y)
        for _ in range(2):
            y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, want)
    # a library call through the frames kernel (CORDIC source): nothing to prepare, no scratch
    p2 = B.make_params(B.WIN_BH4, 13, 24, model=B.MODEL_CPP)
    assert B.describe_frames(p2, frames, hop).startswith("frames kernel: k_frames_direct")
    want2 = torch.from_numpy(_expected(_window(p2), xh, frames, hop, 1, 23)[:, :, 0]).cuda()
    y2 = torch.zeros((frames, N), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    graph2 = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph2, stream=s):
        bhw.apply_frames(p2, x, hop, shift=23, out=y2)
    for _ in range(2):
        y2.zero_()
        graph2.replay()
        torch.cuda.synchronize()
        assert torch.equal(y2, want2)


def test_two_streams_one_table(torch):
    p = B.make_params(B.WIN_BH7, 16, 32)
    wt, _, aa = B.coeffs_preset("nuttall", 32)
    q = B.make_params(wt, 16, 32, aa=aa)
    N, hop, frames = 1 << 16, 1 << 15, 48
    xh, x = _x(torch, frames, hop, N, 1, seed=12)
    wp = torch.from_numpy(_expected(_window(p), xh, frames, hop, 1, 31)[:, :, 0]).cuda()
    wq = torch.from_numpy(_expected(_window(q), xh, frames, hop, 1, 31)[:, :, 0]).cuda()
    with bhw.ResidentTable(p) as t:
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        outs = [torch.zeros((frames, N), dtype=torch.int32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for _ in range(3):
            for s, o, pp in zip(streams, outs, (p, q)):
                with torch.cuda.stream(s):
                    t.apply_frames(pp, x, hop, shift=31, out=o)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], wp) and torch.equal(outs[1], wq)
