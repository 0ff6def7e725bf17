"""Windows of any length on the GPU (bhw_generate_len_* / bhw_apply_frames_len_* / bhw_overlap_add_len_*): L = 2^phi_width reproduces
the power-of-two calls bit for bit (through the existing routes and through the forced any-length kernels), other lengths match the bit
model restated here in NumPy over the oracle's (and the reference's) CORDIC, the frames and overlap-add calls match NumPy on that window,
the from-table calls match the library calls in every table format and replay from a HIP graph, and the side lobes meet the README."""
import ctypes

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import oracle_lib as O
from len_bit_model import combine, full_cos, model_window, thetas  # noqa: F401

pytestmark = pytest.mark.gpu

WIN_OF_TERMS = {2: B.WIN_HAMMING, 3: B.WIN_BH3, 4: B.WIN_BH4, 5: B.WIN_BH5, 7: B.WIN_BH7}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


class forced:
    """bhw_dbg_len_force_kernels: the *_len calls take the any-length kernels at L = 2^phi_width too."""

    def __enter__(self):
        self.prev = B.lib().bhw_dbg_len_force_kernels(1)

    def __exit__(self, *exc):
        B.lib().bhw_dbg_len_force_kernels(self.prev)


def _valid(p):
    return B.lib().bhw_params_validate(ctypes.byref(p)) == 0


# ---- the bit model, restated: len_bit_model.py (shared with test_gpu_table_source.py) ------------------------------------------------------

def _gen(p, L, n0, count):
    return bhw.generate(p, n0, count, length=L).cpu().numpy()


# ---- L = 2^phi_width: the power-of-two windows, bit for bit ----------------------------------------------------------------------

def _identity_lattice():
    for model in (B.MODEL_HLS, B.MODEL_CPP, B.MODEL_VHDL):
        for comb in (B.COMBINE_HLS, B.COMBINE_VHDL):
            for K in (2, 3, 4, 5, 7):
                for W in (8, 16, 24, 32):
                    p = B.make_params(WIN_OF_TERMS[K], 11, W, model=model, combine=comb, validate=False)
                    if _valid(p):
                        yield p


def test_power_of_two_length_is_the_existing_window(torch):
    N = 1 << 11
    rng = np.random.default_rng(1)
    xh = rng.integers(-2 ** 31, 2 ** 31, size=(N // 2) * 7 + N, dtype=np.int64).astype(np.int32)
    x = torch.from_numpy(xh).cuda()
    hop = N // 2
    y = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=(8, N), dtype=np.int64).astype(np.int32)).cuda()
    n = 0
    for p in _identity_lattice():
        sh = p.dat_width - 1
        want_g = bhw.generate(p, 3, 3 * N + 5)
        want_f = bhw.apply_frames(p, x, hop, shift=sh)
        want_o = bhw.overlap_add(p, y, hop, shift=sh)
        for force in (False, True):
            ctx = forced() if force else _Null()
            with ctx:
                assert torch.equal(bhw.generate(p, 3, 3 * N + 5, length=N), want_g), (p.model, p.combine, p.n_terms, p.dat_width, force)
                assert torch.equal(bhw.apply_frames(p, x, hop, shift=sh, length=N), want_f), (p.model, p.n_terms, p.dat_width, force)
                assert torch.equal(bhw.overlap_add(p, y, hop, shift=sh, length=N), want_o), (p.model, p.n_terms, p.dat_width, force)
        n += 1
    assert n >= 100
    p = B.make_params(B.WIN_BH7, 11, 32)
    with forced():
        assert B.describe_len(p, N).startswith("any-length route")
    assert B.describe_len(p, N).startswith("power-of-two route")


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


# ---- other lengths: the bit model -----------------------------------------------------------------------------------------------

def test_restatement_matches_the_oracle_at_power_of_two():
    for model in (B.MODEL_HLS, B.MODEL_CPP, B.MODEL_VHDL):
        for comb in (B.COMBINE_HLS, B.COMBINE_VHDL):
            for K, W in ((2, 16), (4, 24), (7, 32)):
                p = B.make_params(WIN_OF_TERMS[K], 12, W, model=model, combine=comb)
                N = 1 << 12
                assert np.array_equal(model_window(p, N, np.arange(N)), O.generate(O.from_bhw(p), 0, N)), (model, comb, K, W)


def _lengths(P):
    prime = next(q for q in range((1 << P) - 1, 0, -1) if all(q % d for d in range(2, int(q ** 0.5) + 1)))
    return [1, 3, 5, 400, 1000, (1 << P) - 1, 3 << (P - 2), prime]


@pytest.mark.parametrize("P", [12, 16])
def test_other_lengths_match_the_bit_model(torch, P):
    for model in (B.MODEL_HLS, B.MODEL_CPP, B.MODEL_VHDL):
        for comb in (B.COMBINE_HLS, B.COMBINE_VHDL):
            for K, W in ((3, 16), (5, 24), (7, 32)):
                p = B.make_params(WIN_OF_TERMS[K], P, W, model=model, combine=comb, validate=False)
                if not _valid(p):
                    continue
                with bhw.ResidentTable(p) as t:
                    for L in _lengths(P):
                        got = _gen(p, L, 0, L)
                        assert np.array_equal(got, model_window(p, L, np.arange(L))), (model, comb, K, W, L)
                        assert np.array_equal(t.generate(p, 0, L, length=L).cpu().numpy(), got), (model, comb, K, W, L)


@pytest.mark.parametrize("P,W", [(12, 16), (16, 24)])
def test_cpp_model_matches_the_reference_cordic(torch, P, W):
    """Model CPP with the cosines of the reference's own cordic() (oracle/_ref, compiled from the reference source)."""
    if not any(pp == P and ww == W for pp, ww, _ in O.ref_pairs()):
        pytest.fail(f"oracle/_ref lacks the ({P}, {W}) reference build")
    for K in (4, 7):
        p = B.make_params(WIN_OF_TERMS[K], P, W, model=B.MODEL_CPP)
        for L in (3, 400, 1000, (1 << P) - 1):
            assert np.array_equal(_gen(p, L, 0, L), model_window(p, L, np.arange(L), source="ref")), (K, L)


def test_range_semantics_and_symmetric_window(torch):
    p = B.make_params(B.WIN_BH7, 16, 32)
    for L in (400, 1000, 65521):
        w = model_window(p, L, np.arange(L))
        for n0, count in ((L + 17, 3 * L + 5), ((1 << 40) + 5, 2 * L + 1), (7, 5 * L)):
            got = _gen(p, L, n0, count)
            assert np.array_equal(got, w[(n0 + np.arange(count, dtype=np.uint64)) % L]), (L, n0, count)
        sym = bhw.window(p, L, sym=True).cpu().numpy()
        per = _gen(p, L - 1, 0, L - 1)
        assert sym.size == L and np.array_equal(sym[:-1], per) and sym[-1] == per[0]
        assert np.array_equal(bhw.window(p, L).cpu().numpy(), w)
        with bhw.ResidentTable(p) as t:
            assert np.array_equal(t.window(p, L, sym=True).cpu().numpy(), sym)
            assert np.array_equal(t.generate(p, (1 << 40) + 5, 2 * L + 1, length=L).cpu().numpy(),
                                  _gen(p, L, (1 << 40) + 5, 2 * L + 1))


# ---- frames and overlap-add at L = 400 and 1000 ---------------------------------------------------------------------------------

def _frames_expected(w, xh, hop, frames, C, shift, stride):
    L = w.size
    y = np.zeros((frames, stride), dtype=np.int32)
    idx = (np.arange(frames)[:, None] * hop + np.arange(L)[None, :])                    # (frames, L) time indices
    xv = xh.reshape(-1, C)[idx].astype(np.int64)                                        # (frames, L, C)
    v = (xv * w.astype(np.int64)[None, :, None]) >> shift
    y[:, :L * C] = (v & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(frames, L * C)
    return y


def _ola_expected(w, yh, hop, C, shift, t0=0, count=None):
    L = w.size
    frames = yh.shape[0]
    ext = (frames - 1) * hop + L
    count = ext - t0 if count is None else count
    prod = yh[:, :L * C].reshape(frames, L, C).astype(np.int64) * w.astype(np.int64)[None, :, None]
    acc = np.zeros((ext, C), dtype=np.int64)
    t = (np.arange(frames)[:, None] * hop + np.arange(L)[None, :]).ravel()
    np.add.at(acc, t, prod.reshape(-1, C))
    v = acc[t0:t0 + count] >> shift
    return (v & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


@pytest.mark.parametrize("L", [400, 1000])
def test_frames_and_overlap_add_match_numpy(torch, L):
    p = B.make_params(B.WIN_BH7, 16, 32)
    w = _gen(p, L, 0, L)
    rng = np.random.default_rng(L)
    frames = 37
    for hop in (160, L, L + 37):
        for C in (1, 2):
            for stride in (None, 512 * C if L == 400 else None):
                st = L * C if stride is None else stride
                xh = rng.integers(-2 ** 31, 2 ** 31, size=((frames - 1) * hop + L) * C, dtype=np.int64).astype(np.int32)
                y = bhw.apply_frames(p, torch.from_numpy(xh).cuda(), hop, channels=C, shift=31, y_stride=stride, length=L)
                want = _frames_expected(w, xh, hop, frames, C, 31, st)
                got = y.cpu().numpy().reshape(frames, -1)
                assert np.array_equal(got[:, :L * C], want[:, :L * C]), (hop, C, stride)
                assert y.shape == ((frames, L, 2) if C == 2 else (frames, L)) if stride is None else y.shape == (frames, st)
                yh = rng.integers(-2 ** 31, 2 ** 31, size=(frames, st), dtype=np.int64).astype(np.int32)
                yd = torch.from_numpy(yh).cuda()
                x = bhw.overlap_add(p, yd, hop, channels=C, shift=31, y_stride=st, length=L)
                assert np.array_equal(x.cpu().numpy().reshape(-1, C), _ola_expected(w, yh, hop, C, 31)), (hop, C, stride)
                # t0 / count blocks
                ext = (frames - 1) * hop + L
                for t0, count in ((ext // 3, ext // 3 + 1), (ext - 7, 7), (0, hop + 1)):
                    xb = bhw.overlap_add(p, yd, hop, channels=C, shift=31, y_stride=st, t0=t0, count=count, length=L)
                    assert np.array_equal(xb.cpu().numpy().reshape(-1, C), _ola_expected(w, yh, hop, C, 31, t0, count)), (hop, C, t0)


@pytest.mark.parametrize("L,hop", [(400, 160), (1000, 250), (1000, 1300)])
def test_overlap_add_is_the_transpose_of_frames(torch, L, hop):
    """<OLA(y), s> = <y, frames(s)> with values small enough that nothing wraps (shift 0)."""
    p = B.make_params(B.WIN_BH4, 14, 16)
    frames = 23
    rng = np.random.default_rng(hop)
    yh = rng.integers(-128, 128, size=(frames, L), dtype=np.int64).astype(np.int32)
    sh = rng.integers(-128, 128, size=(frames - 1) * hop + L, dtype=np.int64).astype(np.int32)
    ola = bhw.overlap_add(p, torch.from_numpy(yh).cuda(), hop, shift=0, length=L).cpu().numpy().astype(np.int64)
    fr = bhw.apply_frames(p, torch.from_numpy(sh).cuda(), hop, shift=0, length=L).cpu().numpy().astype(np.int64)
    assert int((ola * sh).sum()) == int((yh.astype(np.int64) * fr).sum())


# ---- from a resident table --------------------------------------------------------------------------------------------------------

FORMATS = (B.TABLE_PLAIN, B.TABLE_DELTA16, B.TABLE_RESIDUAL, B.TABLE_NIBBLE, B.TABLE_NIBBLE_ESC)


@pytest.mark.parametrize("P,model,W", [(16, B.MODEL_HLS, 32), (16, B.MODEL_VHDL, 32), (22, B.MODEL_CPP, 32), (22, B.MODEL_CPP, 25)],
                         ids=[f"16-{B.MODEL_HLS}", f"16-{B.MODEL_VHDL}", f"22-{B.MODEL_CPP}", f"22-{B.MODEL_CPP}-w25"])
def test_from_table_equals_library_in_every_format(torch, P, model, W):
    """W 32: the tables of these phase widths are plain under every limit.  cpp 22 / 25 takes the packed formats."""
    p = B.make_params(B.WIN_BH7, P, W, model=model)
    q = B.make_params(B.WIN_BH4, P, W, model=model, combine=B.COMBINE_VHDL)
    rng = np.random.default_rng(P)
    hop, frames = 160, 64
    xh = rng.integers(-2 ** 31, 2 ** 31, size=(frames - 1) * hop + 1000, dtype=np.int64).astype(np.int32)
    x = torch.from_numpy(xh).cuda()
    y = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=(frames, 1000), dtype=np.int64).astype(np.int32)).cuda()
    lens = (400, 1000, 3 << (P - 2))
    want = {(id(pp), L): bhw.generate(pp, 5, L + 300, length=L) for pp in (p, q) for L in lens}
    want_f = {id(pp): bhw.apply_frames(pp, x, hop, shift=31, length=1000) for pp in (p, q)}
    want_o = {id(pp): bhw.overlap_add(pp, y, hop, shift=31, length=1000) for pp in (p, q)}
    seen = set()
    for fmt in FORMATS:
        with bhw.ResidentTable(p, table_format=fmt) as t:
            for pp in (p, q):
                for L in lens:
                    assert torch.equal(t.generate(pp, 5, L + 300, length=L), want[(id(pp), L)]), (fmt, L)
                assert torch.equal(t.apply_frames(pp, x, hop, shift=31, length=1000), want_f[id(pp)]), fmt
                assert torch.equal(t.overlap_add(pp, y, hop, shift=31, length=1000), want_o[id(pp)]), fmt
            if P >= 22 and fmt == B.TABLE_NIBBLE:
                assert "split" in t.describe(p, 0, 1 << P) or "nibble" in t.describe(p, 0, 1 << P)
            d = B.describe_len(p, 1000, frames=B.make_frames(frames, hop), table=t.handle)
            assert d.startswith("any-length route") and "k_frames_table_len<" in d, d
            seen.add(d.split("k_frames_table_len<")[1].split(",")[0])
    if W < 32:
        assert len(seen) >= 3, seen


def test_from_table_calls_replay_from_a_graph(torch):
    p = B.make_params(B.WIN_BH7, 16, 32)
    L, hop, frames = 400, 160, 50
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=(frames - 1) * hop + L, dtype=np.int64).astype(np.int32)).cuda()
    y = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=(frames, L), dtype=np.int64).astype(np.int32)).cuda()
    with bhw.ResidentTable(p) as t:
        wg, wf, wo = t.generate(p, 7, 3 * L, length=L), t.apply_frames(p, x, hop, shift=31, length=L), t.overlap_add(p, y, hop, shift=31, length=L)
        og, of, oo = torch.zeros_like(wg), torch.zeros_like(wf), torch.zeros_like(wo)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s):
            t.generate(p, 7, 3 * L, out=og, length=L)
            t.apply_frames(p, x, hop, shift=31, out=of, length=L)
            t.overlap_add(p, y, hop, shift=31, out=oo, length=L)
        for _ in range(2):
            og.zero_(), of.zero_(), oo.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(og, wg) and torch.equal(of.view_as(wf), wf) and torch.equal(oo, wo)


# ---- quality ----------------------------------------------------------------------------------------------------------------------

def _sidelobe_db(w, pad=16):
    w = np.asarray(w, dtype=np.float64)
    spec = np.abs(np.fft.rfft(w, pad * len(w)))
    spec /= spec[0]
    i = 1
    while i + 1 < len(spec) and spec[i + 1] < spec[i]:
        i += 1
    return 20 * np.log10(spec[i:].max())


@pytest.mark.parametrize("win,level,tol", [(B.WIN_BH4, -92, 1.0), (B.WIN_BH5, -124, 2.5)])
def test_sidelobes_at_length_1000(torch, win, level, tol):
    aa = B.coeffs_from_float(win, 31 if win < 5 else 32)
    p = B.make_params(win, 24, 32, aa=aa)
    got = _sidelobe_db(bhw.window(p, 1000).cpu().numpy())
    assert abs(got - level) <= tol, got
