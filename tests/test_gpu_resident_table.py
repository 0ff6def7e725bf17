"""Resident CORDIC tables on the GPU: one table per configuration serves any weights, any range, the fused apply, ownership parts,
graph capture and concurrent readers, bit-identical to the rebuilt table strategy and to the oracle."""
import ctypes
import hashlib
import threading

import numpy as np
import pytest

import oracle_lib as O
from blackman_harris_win_amd import binding as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _md5(a):
    return hashlib.md5(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def _weights(pw, w, model, precision):
    """Built-in BH-7, Nuttall, flat-top (2), Hann, Hamming -- each with both cosine-sum rules: the run-time ports of one table."""
    sets = [(B.WIN_BH7, None), (B.WIN_HANN, None), (B.WIN_HAMMING, None)]
    for name in ("nuttall", "flat-top-2"):
        wt, _, aa = B.coeffs_preset(name, w)
        sets.append((wt, aa))
    out = []
    for win, aa in sets:
        for combine in (B.COMBINE_HLS, B.COMBINE_VHDL):
            out.append(B.make_params(win, pw, w, model=model, precision=precision, combine=combine, aa=aa))
    return out


def _rebuilt(p, n0, count):
    import blackman_harris_win_amd as bhw
    return bhw.generate(p, n0, count, algo=B.ALGO_TABLE)


# (model, phi_width, dat_width, precision, expected table format / layout, whole-period kernel)
SHAPES = [
    (B.MODEL_HLS, 26, 32, 1, "nibble, natural", "k_tile9"),
    (B.MODEL_CPP, 26, 32, 1, "nibble+esc, natural", "k_table_combine_tile"),
    (B.MODEL_HLS, 22, 24, 1, "", "k_t"),
    (B.MODEL_VHDL, 22, 24, 1, "", "k_t"),
    (B.MODEL_VHDL, 22, 24, 3, "", "k_t"),
    (B.MODEL_HLS, 18, 32, 1, "plain, natural", "k_table_combine_fold_t"),
    (B.MODEL_VHDL, 18, 32, 3, "plain, natural", "k_table_combine_fold"),
    (B.MODEL_CPP, 24, 16, 1, "plain, natural", "k_runlength_window"),
]


@pytest.mark.parametrize("model,pw,w,prec,layout,kernel", SHAPES)
def test_every_weight_set_from_one_table_equals_the_rebuilt_path_and_the_oracle(torch, reference_pins, model, pw, w, prec, layout, kernel):
    import blackman_harris_win_amd as bhw
    n = 1 << pw
    ps = _weights(pw, w, model, prec)
    with bhw.ResidentTable(ps[0]) as rt:
        line = rt.describe(ps[0], 0, n)
        assert layout in line and kernel in line, line
        for i, p in enumerate(ps):
            got = rt.generate(p, 0, n)
            assert torch.equal(got, _rebuilt(p, 0, n)), (i, line)
            if pw <= 24 and i in (0, 1, 7):                     # BH-7 both rules, Nuttall VHDL rule: the oracle itself
                assert np.array_equal(got.cpu().numpy(), O.generate_mt(O.from_bhw(p), 0, n)), i
        if model == B.MODEL_CPP and pw == 26:                   # C3 of BASELINE: the md5 of the reference's own cordic()
            assert _md5(rt.generate(ps[0], 0, n).cpu().numpy()) == reference_pins["windows"]["C3"]["md5"]


RAGGED = [(B.MODEL_HLS, 26, 32, 1), (B.MODEL_CPP, 26, 32, 1), (B.MODEL_VHDL, 22, 24, 3), (B.MODEL_HLS, 18, 32, 1), (B.MODEL_CPP, 24, 16, 1)]


@pytest.mark.parametrize("model,pw,w,prec", RAGGED)
def test_ragged_ranges_equal_the_oracle(torch, model, pw, w, prec):
    """Seeded n0 (also beyond 2^40), ranges across a period boundary, counts 1 .. N - 8: all through k_range_combine.  With the
    escape format (cpp model, 2^26 / 32 bits) the N - 8 range reads every table entry through harmonic 1, the listed ones included."""
    import blackman_harris_win_amd as bhw
    n = 1 << pw
    rng = np.random.default_rng(pw * 10 + model)
    ps = _weights(pw, w, model, prec)
    with bhw.ResidentTable(ps[0]) as rt:
        if model == B.MODEL_CPP and pw == 26:
            assert "nibble+esc" in rt.describe(ps[0], 0, n)
        for count in (1, 63, 4097, (1 << 20) + 3, n - 8):
            for n0 in (int(rng.integers(0, n)), (1 << 40) + int(rng.integers(0, 1 << 40)), n - count // 2 - 1):
                for p in (ps[0], ps[1], ps[7]):
                    assert "k_range_combine" in rt.describe(p, n0, count)
                    got = rt.generate(p, n0, count).cpu().numpy()
                    if count <= (1 << 20) + 3 or pw <= 22:
                        want = O.generate_mt(O.from_bhw(p), n0, count)
                    else:
                        want = _rebuilt(p, n0, count).cpu().numpy()       # (the rebuilt path is pinned against the oracle elsewhere)
                    assert np.array_equal(got, want), (count, n0, p.combine)
                if count == n - 8 and pw > 22:
                    break                                                  # one long range per shape is enough


def test_chunked_streaming_after_elaborate(torch):
    """A 2^22 window as 64 enable(2^16) chunks and one odd chunk; a change on the AA ports takes effect from the next chunk."""
    import blackman_harris_win_amd as bhw
    sel = bhw.WinSelector(PHI_WIDTH=22, DAT_WIDTH=24, WIN_TYPE="BH7TERM").elaborate()
    assert sel.table is not None and sel.table.nbytes > 0
    n = 1 << 22
    chunks = [sel.enable(1 << 16) for _ in range(64)]
    odd = sel.enable(12345)
    whole = torch.cat(chunks)
    assert torch.equal(whole, sel.window())
    want = O.generate_mt(O.from_bhw(sel.params), 0, n)
    assert np.array_equal(whole.cpu().numpy(), want)
    assert np.array_equal(odd.cpu().numpy(), want[:12345])
    _, _, aa = B.coeffs_preset("bh7-readme", 24)
    old = B.BhwParams.from_buffer_copy(sel.params)
    for k in range(7):
        sel.params.aa[k] = aa[k]
    nxt = sel.enable(5000)
    assert np.array_equal(nxt.cpu().numpy(), O.generate(O.from_bhw(sel.params), 12345, 5000))
    assert not np.array_equal(nxt.cpu().numpy(), O.generate(O.from_bhw(old), 12345, 5000))
    sel.release()
    assert sel.table is None
    assert np.array_equal(sel.enable(777).cpu().numpy(), O.generate(O.from_bhw(sel.params), 17345, 777))
    taylor = bhw.WinSelector(PHI_WIDTH=16, DAT_WIDTH=16, WIN_TYPE="HANN", SIN_TYPE="TAYLOR").elaborate()
    assert taylor.table is None                                            # nothing to keep for the Taylor source


@pytest.mark.parametrize("pw,w", [(22, 24), (18, 32), (26, 32)])
def test_apply_from_table_equals_the_fused_apply(torch, pw, w):
    import blackman_harris_win_amd as bhw
    n = 1 << pw
    p = B.make_params(B.WIN_BH7, pw, w)
    q = B.make_params(B.WIN_BH4, pw, w, combine=B.COMBINE_VHDL)
    gen = torch.Generator(device="cuda").manual_seed(pw)
    x = torch.randint(-(1 << 30), 1 << 30, (3 * n + 1000,), dtype=torch.int32, device="cuda", generator=gen)
    with bhw.ResidentTable(p) as rt:
        for pp in (p, q):
            for n0, cnt in ((0, 3 * n), (77, 3 * n + 1000), (n - 5, 4097), (12345, 1 << 16)):
                xs = x[:cnt]
                assert torch.equal(rt.apply(pp, xs, n0=n0, shift=w - 1), bhw.apply(pp, xs, n0=n0, shift=w - 1)), (pp.n_terms, n0, cnt)
        sel = bhw.WinSelector(PHI_WIDTH=pw, DAT_WIDTH=w, WIN_TYPE="BH7TERM").elaborate()
        y = sel.apply(x[:4096])
        assert torch.equal(y, bhw.apply(p, x[:4096], n0=0))
        sel.release()


def test_parts_from_one_table(torch):
    import blackman_harris_win_amd as bhw
    p = B.make_params(B.WIN_BH7, 26, 32)
    n = 1 << 26
    whole = _rebuilt(p, 0, n)
    with bhw.ResidentTable(p) as rt:
        for G in (2, 4, 8):
            out = torch.zeros(n, dtype=torch.int32, device="cuda")
            for g in range(G):
                rt.generate_part(p, g, G, out)
            assert torch.equal(out, whole), G
        sel = bhw.WinSelector(PHI_WIDTH=26, DAT_WIDTH=32, WIN_TYPE="BH7TERM").elaborate()
        out = torch.zeros(n, dtype=torch.int32, device="cuda")
        for g in range(4):
            sel.shard(g, 4, out=out, layout="interleaved")
        assert torch.equal(out, whole)
        sel.release()
    s = B.make_params(B.WIN_BH7, 18, 32)
    with bhw.ResidentTable(s) as rt:
        with pytest.raises(B.BhwError) as ei:
            rt.generate_part(s, 0, 2, torch.zeros(1 << 18, dtype=torch.int32, device="cuda"))
        assert ei.value.code == -2


def test_forced_formats_agree_and_hold_the_workspace_size(torch):
    import blackman_harris_win_amd as bhw
    p = B.make_params(B.WIN_BH7, 26, 32)
    n = 1 << 26
    ref = None
    for fmt in (B.TABLE_BEST, B.TABLE_PLAIN, B.TABLE_DELTA16, B.TABLE_RESIDUAL, B.TABLE_NIBBLE, B.TABLE_NIBBLE_ESC):
        with bhw.ResidentTable(p, table_format=fmt) as rt:
            got = torch.cat([rt.generate(p, 0, n), rt.generate(p, 999, 1 << 20)])
            if ref is None:
                ref = got
            assert torch.equal(got, ref), fmt
            ex = B.BhwExec()
            ex.struct_size = ctypes.sizeof(B.BhwExec)
            ex.algo = B.ALGO_TABLE
            ex.table_format = fmt
            assert rt.nbytes == B.lib().bhw_workspace_bytes_ex(ctypes.byref(p), 0, n, ctypes.byref(ex)), (fmt, rt.describe(p, 0, n))
            if fmt == B.TABLE_BEST:
                assert rt.nbytes <= 17 * 2 ** 20
            if fmt == B.TABLE_PLAIN:
                assert rt.nbytes == 8 * (n // 4)
    assert torch.equal(ref[:n], _rebuilt(p, 0, n))


def test_capture_on_a_never_prepared_stream(torch):
    import blackman_harris_win_amd as bhw
    L = B.lib()
    L.bhw_dbg_library_scratch_bytes.restype = ctypes.c_uint64
    L.bhw_dbg_library_scratch_bytes.argtypes = [ctypes.c_int, ctypes.c_void_p]
    p = B.make_params(B.WIN_BH7, 24, 32, model=B.MODEL_CPP)
    q = B.make_params(B.WIN_BH5, 24, 32, model=B.MODEL_CPP, combine=B.COMBINE_VHDL)
    n = 1 << 24
    dev = torch.cuda.current_device()
    x = torch.arange(-50000, 50000, dtype=torch.int32, device="cuda")
    want_w, want_a = _rebuilt(p, 0, n), bhw.apply(q, x, n0=5, shift=20)
    want_r = O.generate_mt(O.from_bhw(q), n - 33333, 70001)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with bhw.ResidentTable(p) as rt:
        with torch.cuda.stream(st):
            out_w = torch.zeros(n, dtype=torch.int32, device="cuda")
            out_r = torch.zeros(70001, dtype=torch.int32, device="cuda")
            out_a = torch.zeros_like(x)
            st.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st):
                rt.generate(p, 0, n, out=out_w)
                rt.generate(q, n - 33333, 70001, out=out_r)
                rt.apply(q, x, n0=5, shift=20, out=out_a)
            assert L.bhw_dbg_library_scratch_bytes(dev, ctypes.c_void_p(st.cuda_stream)) == 0
            for _ in range(2):
                out_w.zero_()
                out_r.zero_()
                out_a.zero_()
                graph.replay()
                st.synchronize()
                assert torch.equal(out_w, want_w)
                assert np.array_equal(out_r.cpu().numpy(), want_r)
                assert torch.equal(out_a, want_a)
            assert L.bhw_dbg_library_scratch_bytes(dev, ctypes.c_void_p(st.cuda_stream)) == 0
            del graph


def test_two_streams_and_two_threads_share_one_table(torch):
    import blackman_harris_win_amd as bhw
    n = 1 << 22
    p = B.make_params(B.WIN_BH7, 22, 24)
    wt, _, aa = B.coeffs_preset("nuttall", 24)
    q = B.make_params(wt, 22, 24, aa=aa, combine=B.COMBINE_VHDL)
    want = {0: _rebuilt(p, 0, n), 1: _rebuilt(q, 3, n)}
    errors = []
    with bhw.ResidentTable(p) as rt:
        def work(i, par, n0):
            try:
                st = torch.cuda.Stream()
                with torch.cuda.stream(st):
                    for _ in range(20):
                        got = rt.generate(par, n0, n)
                    st.synchronize()
                    if not torch.equal(got, want[i]):
                        errors.append(i)
            except Exception as e:   # noqa: BLE001 -- reported below
                errors.append(repr(e))
        ts = [threading.Thread(target=work, args=(0, p, 0)), threading.Thread(target=work, args=(1, q, 3))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    assert errors == []


def test_mismatched_generics_are_refused(torch):
    import blackman_harris_win_amd as bhw
    p = B.make_params(B.WIN_BH7, 20, 24)
    with bhw.ResidentTable(p) as rt:
        with pytest.raises(B.BhwError) as ei:
            rt.generate(B.make_params(B.WIN_BH7, 20, 25), 0, 16)
        assert ei.value.code == -1 and "dat_width" in ei.value.detail
