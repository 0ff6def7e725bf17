"""The fused log spectrogram, log-mel spectrogram and MFCC on the GPU (bhw_logspec_f32_*, bhw_logspec_mfft_f32_* through
bhw.log_spectrogram(_mixed), bhw.mfcc(_mixed) and their table= forms).

Log stage: for every case of tests/logspec_cases.py the output is compared with the numpy restatement (logspec_cases.log_ref) applied to
bhw.spectrogram(_mixed) of the same call on the same GPU: every word within one float32 ulp (the device's binary64 log is not
correctly rounded; a word can differ only where the binary64 value sits within that log's error of a float32 rounding boundary).  DCT
stage: bit for bit the binary64 chain (logspec_cases.dct_ref) over the log_spectrogram(_mixed) output of the same call.  Library form
against table form: word for word.  With BHW_LOGSPEC_RECORD=<file> the share of log words that are not bit-equal, and the end-to-end
errors, are written there as JSON (profiles/r40_logspec.json is such a record)."""
import json
import os

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B
from blackman_harris_win_amd.selector import fbank_bands

import logspec_cases as LC
import table_source_cases as TC

pytestmark = pytest.mark.gpu

SENTINEL = 12345.5
RECORD = {"log_stage": {}, "end_to_end": {}}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    yield torch
    path = os.environ.get("BHW_LOGSPEC_RECORD")
    if path:
        words = sum(v["words"] for v in RECORD["log_stage"].values())
        off = sum(v["not_bit_equal"] for v in RECORD["log_stage"].values())
        RECORD["log_stage_total"] = {"words": words, "not_bit_equal": off, "share": off / words if words else None}
        with open(path, "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


def _signal(nb, T, seed=0):
    """(nb, T) float32: noise of 1000 + tones of 1e3 and 1e-3 + an offset."""
    rng = np.random.default_rng(2000 + seed)
    n = np.arange(T, dtype=np.float64)
    x = rng.standard_normal((nb, T)) * 1000 + 1e3 * np.cos(2 * np.pi * 0.1234 * n) + 1e-3 * np.cos(2 * np.pi * 0.31 * n + 1.0) + 250.0
    return x.astype(np.float32)


def _bits(t):
    return t.contiguous().cpu().numpy().view(np.uint32)


def _same(a, b):
    """Word for word, a NaN equal to any NaN (the contract says a NaN passes through, not which)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _padded_out(torch, nb, frames, W):
    ys = W + LC.ROW_GAP
    buf = torch.full((nb, frames * ys + LC.SIGNAL_GAP), SENTINEL, device="cuda")
    return buf, buf[:, :frames * ys].view(nb, frames, ys)[:, :, :W]


def _gaps_intact(torch, buf, nb, frames, W):
    gaps = torch.ones_like(buf, dtype=torch.bool)
    gaps[:, :frames * (W + LC.ROW_GAP)].view(nb, frames, W + LC.ROW_GAP)[:, :, :W] = False
    return bool((buf[gaps] == SENTINEL).all())


_FBANKS, _DCTS = {}, {}


def _fbank(c):
    w = LC.bank(c)
    if w is None:
        return None
    key = (c["base"]["n_fft"], c["bank"])
    if key not in _FBANKS:
        _FBANKS[key] = bhw.FilterBank(w, device="cuda")
    return _FBANKS[key]


def _dct(c):
    d = LC.dct(c)
    if d is None:
        return None
    key = (d.shape, c["dct"])
    if key not in _DCTS:
        _DCTS[key] = bhw.DctMatrix(d, device="cuda")
    return _DCTS[key]


def _fronts(c):
    mixed = c["family"] == "mixed"
    return (bhw.spectrogram_mixed, bhw.log_spectrogram_mixed) if mixed else (bhw.spectrogram, bhw.log_spectrogram)


def _log_kw(c):
    log, floor, add = LC.LOGS[c["log"]]
    return dict(log=log, floor=floor, add=add)


@pytest.mark.parametrize("cid", LC.case_ids())
def test_log_within_one_ulp_and_dct_bit_for_bit(torch, cid):
    c = LC.case(cid)
    b = c["base"]
    p = LC.params(b["setup"])
    w, fb, dm = LC.bank(c), _fbank(c), _dct(c)
    nb, n_fft, hop, W, Wp = b["B"], b["n_fft"], b["hop"], LC.width(c), LC.parent_width(c)
    xh = _signal(nb, b["T"])
    if b.get("padded"):
        xbuf = torch.full((nb, b["T"] + 5), SENTINEL, device="cuda")
        xbuf[:, :b["T"]] = torch.from_numpy(xh).cuda()
        x = xbuf[:, :b["T"]]
    else:
        x = torch.from_numpy(xh).cuda()
    parent, front = _fronts(c)
    kw, lkw = LC.call_kw(c), _log_kw(c)
    mult, floor, add = LC.log_args(c)
    q = parent(p, x, n_fft, hop, fbank=fb, **kw).cpu().numpy()
    frames = q.shape[1]
    assert frames == LC.desc(c)[2] and q.shape == (nb, frames, Wp)
    # the log stage (of a DCT case too: the rows its DCT is taken over)
    g = front(p, x, n_fft, hop, fbank=fb, **lkw, **kw)
    gh = g.cpu().numpy()
    want = LC.log_ref(q, mult, floor, add)
    apart = LC.ulps_apart(gh, want)
    off = int((apart != 0).sum())
    print(f"logspec {cid}: {gh.size} log words, {off} not bit-equal ({off / gh.size:.2e}), at most {int(apart.max())} ulp apart")
    RECORD["log_stage"][cid] = {"words": int(gh.size), "not_bit_equal": off, "max_ulp": int(apart.max())}
    assert apart.max() <= 1, (cid, int(apart.max()))
    low = np.float32(mult * np.log(floor))
    if not add:
        clamped = q < floor
        assert LC.ulps_apart(gh[clamped], np.full(int(clamped.sum()), low, dtype=np.float32)).max(initial=0) <= 1, "a clamped word is the floor's log"
    if w is not None:
        empty = np.flatnonzero(np.diff(fbank_bands(w)[1].astype(np.int64)) == 0)
        assert LC.ulps_apart(gh[..., empty], np.full(gh[..., empty].shape, low, dtype=np.float32)).max(initial=0) <= 1, "an empty filter gives the floor's log"
    # the call of the case: library form, into padded strides where the case says so
    if b.get("padded"):
        buf, out = _padded_out(torch, nb, frames, W)
        got = front(p, x, n_fft, hop, fbank=fb, dct=dm, out=out, **lkw, **kw)
        assert got.data_ptr() == out.data_ptr() and _gaps_intact(torch, buf, nb, frames, W), "a gap was written"
    else:
        got = front(p, x, n_fft, hop, fbank=fb, dct=dm, **lkw, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (nb, frames, W)
    got_h = got.cpu().numpy()
    if dm is None:
        assert _same(got_h, gh), "the same call twice (packed and padded)"
    else:
        assert _same(got_h.reshape(-1, W), LC.dct_ref(gh.reshape(-1, Wp), LC.dct(c))), "the DCT is the binary64 chain over the log rows"
        if c.get("dct") == "identity":
            assert _same(got_h, gh), "the identity matrix gives the log rows back"
    with bhw.ResidentTable(p) as tab:
        d = LC.parse(LC.line(c, table=tab._live()))
        assert d["table"] and ("k_logspec_table" if c["family"] == "pow2" else "k_logspec_mfft_table") in d["kernels"], d["line"]
        gt = front(p, x, n_fft, hop, fbank=fb, dct=dm, table=tab, **lkw, **kw)
        torch.cuda.synchronize()
    assert np.array_equal(_bits(gt), _bits(got)), "library against table"


def _table_cases():
    out = []
    for j, table in enumerate(TC.TABLES):
        for weights in TC.ROTATION[table]:
            for front in ("spectrogram", "spectrogram_mixed"):
                out.append((table, weights, front, j))
    return out


@pytest.fixture(scope="module")
def tables(torch):
    built = {}
    for name, (model, pw, w, limit, _) in TC.TABLES.items():
        built[name] = bhw.ResidentTable(B.make_params(B.WIN_BH7, pw, w, model=TC.MODELS[model]), table_format=TC.LIMITS[limit])
    yield built
    for t in built.values():
        t.close()


def test_every_table_kernel_instance_runs(torch, tables):
    """Every k_logspec_table<FMT,NT,MODE> and k_logspec_mfft_table<FMT,NT,MODE> the describe line names for the tables and weight sets
    of tests/table_source_cases.py: an MFCC from the table equals the library form word for word."""
    seen = {"k_logspec_table": set(), "k_logspec_mfft_table": set()}
    for table, weights, front, j in _table_cases():
        mixed = front.endswith("_mixed")
        sh = TC.shape(TC.FRONT[front], table, j)
        n, L, hop = sh["n_fft"], sh["L"], sh["hop"]
        p = TC.params(table, weights)
        x = torch.from_numpy(_signal(TC.NB, (sh["frames"] - 1) * hop + n, seed=j)).cuda()
        key = (n, "mel20")
        if key not in _FBANKS:
            _FBANKS[key] = bhw.FilterBank(bhw.mel_weights(n, 20, 16000), device="cuda")
            _DCTS[key] = bhw.DctMatrix(bhw.dct_weights(7, 20), device="cuda")
        fb, dm = _FBANKS[key], _DCTS[key]
        kw = dict(win_length=L, center=False, detrend=sh["detrend"], fbank=fb, dct=dm, log="ln", floor=1e-6, add=True)
        lib = (bhw.mfcc_mixed if mixed else bhw.mfcc)(p, x, n, hop, **kw)
        tab = tables[table]
        got = (bhw.mfcc_mixed if mixed else bhw.mfcc)(p, x, n, hop, table=tab, **kw)
        assert np.array_equal(_bits(got), _bits(lib)), (table, weights, front)
        frames = lib.shape[1]
        s = B.make_stft(TC.NB, x.shape[1], frames, hop, n, col0=0 if sh["detrend"] else (n - L) // 2, shift=p.dat_width - 1)
        ls = B.make_logspec(1e-6, 1.0, add=True, coeffs=7, dct_rows=20)
        line = (B.describe_logspec_mfft if mixed else B.describe_logspec)(p, L, s, ls, detrend=sh["detrend"], fbank=fb.descriptor, table=tab._live())
        name = "k_logspec_mfft_table" if mixed else "k_logspec_table"
        triple = tuple(int(v) for v in LC.parse(line)["kernels"][name])
        assert triple == TC.triple(table, weights), (line, TC.triple(table, weights))
        seen[name].add(triple)
    torch.cuda.synchronize()
    want = {TC.triple(t, w) for t in TC.TABLES for w in TC.ROTATION[t]}
    assert seen["k_logspec_table"] == want and seen["k_logspec_mfft_table"] == want and len(want) >= 12


@pytest.mark.parametrize("mixed,n_fft,hop,L,filters,coeffs", [(False, 64, 16, 49, 10, 13), (False, 2048, 512, 2048, 128, 40), (True, 400, 160, 400, 80, 13)])
def test_a_row_depends_on_nothing_but_itself(torch, mixed, n_fft, hop, L, filters, coeffs):
    """A signal alone and as signal 37 of 64, shifted by three hops (another slot and another group), into padded strides, 1-D, and
    library against table: equal rows word for word, as log rows, log-bank rows and MFCCs."""
    p = B.make_params(B.WIN_BH7, 12, 32)
    T = 6 * n_fft + 40 * hop
    xh = (np.random.default_rng(7).standard_normal((64, T)) * 100 + 3).astype(np.float32)
    x = torch.from_numpy(xh).cuda()
    fbm = bhw.FilterBank(bhw.mel_weights(n_fft, filters, 16000), device="cuda")
    dm = bhw.DctMatrix(bhw.dct_weights(coeffs, filters), device="cuda")
    front = bhw.log_spectrogram_mixed if mixed else bhw.log_spectrogram
    for fb, dct in ((None, None), (fbm, None), (fbm, dm)):
        kw = dict(win_length=L, center=False, fbank=fb, dct=dct, log="log10", floor=1e-3)
        W = coeffs if dct is not None else filters if fb is not None else n_fft // 2 + 1
        alone = front(p, x[37:38].clone(), n_fft, hop, **kw)
        batch = front(p, x, n_fft, hop, **kw)
        assert tuple(batch.shape) == (64, alone.shape[1], W) and np.array_equal(_bits(alone[0]), _bits(batch[37]))
        shifted = front(p, x[37:38, 3 * hop:].clone(), n_fft, hop, **kw)
        assert shifted.shape[1] == alone.shape[1] - 3 and np.array_equal(_bits(shifted[0]), _bits(alone[0, 3:]))
        frames = alone.shape[1]
        buf, out = _padded_out(torch, 5, frames, W)
        front(p, x[35:40], n_fft, hop, out=out, **kw)
        assert np.array_equal(_bits(out[2]), _bits(alone[0])) and _gaps_intact(torch, buf, 5, frames, W)
        one = front(p, x[37], n_fft, hop, **kw)
        assert one.dim() == 2 and np.array_equal(_bits(one), _bits(alone[0]))
        with bhw.ResidentTable(p) as tab:
            assert np.array_equal(_bits(front(p, x[37:38].clone(), n_fft, hop, table=tab, **kw)), _bits(alone))
            torch.cuda.synchronize()


@pytest.mark.parametrize("mixed,n_fft", [(False, 256), (True, 240)])
def test_zeros_give_the_floors_log_and_a_nan_reaches_only_its_rows(torch, mixed, n_fft):
    p = B.make_params(B.WIN_BH7, 12, 32)
    L, hop, T = 200, 80, 4000
    w = bhw.mel_weights(n_fft, 80, 16000)
    fb = bhw.FilterBank(w, device="cuda")
    dm = bhw.DctMatrix(bhw.dct_weights(13, 80), device="cuda")
    front, parent = (bhw.log_spectrogram_mixed, bhw.spectrogram_mixed) if mixed else (bhw.log_spectrogram, bhw.spectrogram)
    for add in (False, True):
        for log, floor in (("db", 1e-10), ("ln", 2.0), (-3.0, 1e-3)):
            low = np.float32(LC.log_multiplier(log) * np.log(floor))
            for f in (None, fb):
                z = front(p, torch.zeros((2, T), device="cuda"), n_fft, hop, win_length=L, fbank=f, log=log, floor=floor, add=add).cpu().numpy()
                assert LC.ulps_apart(z, np.full(z.shape, low, dtype=np.float32)).max() <= 1, "a row of zeros gives the floor's log in every column"
                assert (z == z.flat[0]).all()
            z = front(p, torch.zeros((2, T), device="cuda"), n_fft, hop, win_length=L, fbank=fb, dct=dm, log=log, floor=floor, add=add)
            zl = front(p, torch.zeros((2, T), device="cuda"), n_fft, hop, win_length=L, fbank=fb, log=log, floor=floor, add=add)
            assert _same(z.cpu().numpy().reshape(-1, 13), LC.dct_ref(zl.cpu().numpy().reshape(-1, 80), dm.dense()))
    xh = (np.random.default_rng(3).standard_normal((3, T)) * 10 + 1).astype(np.float32)
    kw = dict(win_length=L, center=False, log="ln", floor=1e-6, add=True)
    for f, dct in ((None, None), (fb, None), (fb, dm)):
        clean = front(p, torch.from_numpy(xh).cuda(), n_fft, hop, fbank=f, dct=dct, **kw)
        for bad in (np.nan, np.inf):
            xn = xh.copy()
            t0 = 2000
            xn[1, t0] = bad
            xd = torch.from_numpy(xn).cuda()
            got = front(p, xd, n_fft, hop, fbank=f, dct=dct, **kw)
            frames, col0 = clean.shape[1], (n_fft - L) // 2
            hit = np.zeros((3, frames), dtype=bool)
            for fr in range(frames):
                hit[1, fr] = fr * hop + col0 <= t0 < fr * hop + col0 + L
            assert hit.sum() in (2, 3)
            assert np.array_equal(_bits(got)[~hit], _bits(clean)[~hit]), "a NaN or an infinity reaches only the rows whose window covers it"
            # carried as the formulas say: the log of the parent's words, then the chain
            q = parent(p, xd, n_fft, hop, win_length=L, center=False, fbank=f).cpu().numpy()
            g = LC.log_ref(q, 1.0, 1e-6, True)
            if dct is None:
                gh = got.cpu().numpy()
                assert np.array_equal(np.isnan(gh), np.isnan(g)) and np.array_equal(np.isposinf(gh), np.isposinf(g))
                assert LC.ulps_apart(gh, g).max() <= 1
                assert not np.isfinite(gh[hit][:, (np.diff(fbank_bands(w)[1].astype(np.int64)) > 0) if f is not None else slice(None)]).any()
            else:
                gl = front(p, xd, n_fft, hop, fbank=f, **kw).cpu().numpy()
                assert _same(got.cpu().numpy().reshape(-1, 13), LC.dct_ref(gl.reshape(-1, 80), dm.dense()))


def _log_domain_error(got, ref):
    """Per row the largest |got - ref|, then the largest row."""
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max(axis=-1).max())


@pytest.mark.parametrize("mixed,n_fft", [(True, 400), (False, 512)])
def test_end_to_end_within_twice_the_torch_route(torch, mixed, n_fft):
    """Noise scaled so the powers sit far above the floor, 400 / hop 160 (mixed) and 400 in 512 / hop 160, 80 mel, 13 coefficients,
    log = ln(q + 1e-6).  Metric: the largest absolute error of a row, in the log domain (the log-mel rows) and of the MFCCs, against a
    float64 reference computed from x (the float32 windowed rows stft_frames writes, transformed, squared, folded, logged and
    transformed in float64); bound: twice the same figure for the float32 torch route (torch.stft, abs() ** 2, matmul, log, matmul) on
    the same GPU.  Measured on an MI355X: see DESIGN.md section 40."""
    p = B.make_params(B.WIN_BH7, 12, 32)
    L, hop = 400, 160
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn((3, 16000), device="cuda", generator=g) * 100 + 5
    mel, dct = bhw.mel_weights(n_fft, 80, 16000), bhw.dct_weights(13, 80)
    fb, dm = bhw.FilterBank(mel, device="cuda"), bhw.DctMatrix(dct, device="cuda")
    front = bhw.log_spectrogram_mixed if mixed else bhw.log_spectrogram
    kw = dict(win_length=L, fbank=fb, log="ln", floor=1e-6, add=True)
    got_log, got_mfcc = front(p, x, n_fft, hop, **kw), (bhw.mfcc_mixed if mixed else bhw.mfcc)(p, x, n_fft, hop, dct=dm, **kw)
    v = bhw.window(p, L, dtype=torch.float32)
    S = torch.stft(x, n_fft, hop, L, window=v, center=True, pad_mode="reflect", return_complex=True)
    route_log = torch.log(torch.matmul((S.abs() ** 2).transpose(-1, -2), torch.from_numpy(mel).cuda()) + 1e-6)
    route_mfcc = torch.matmul(route_log, torch.from_numpy(dct).cuda())
    assert got_log.shape == route_log.shape and got_mfcc.shape == route_mfcc.shape and got_mfcc.is_contiguous()
    rows = bhw.stft_frames(p, x, n_fft, hop, win_length=L).cpu().numpy().astype(np.float64)
    ref_log = np.log((np.abs(np.fft.rfft(rows, axis=-1)) ** 2) @ mel.astype(np.float64) + 1e-6)
    ref_mfcc = ref_log @ dct.astype(np.float64)
    for name, got, route, ref in (("log-mel", got_log, route_log, ref_log), ("mfcc", got_mfcc, route_mfcc, ref_mfcc)):
        err, yard = _log_domain_error(got.cpu().numpy(), ref), _log_domain_error(route.cpu().numpy(), ref)
        print(f"logspec end to end {L} / {n_fft} / {hop}, 80 mel, 13 coefficients, {name}: fused {err:.3e}, torch route {yard:.3e}, ratio {err / yard:.3f}")
        RECORD["end_to_end"][f"{n_fft}-{name}"] = {"fused": err, "torch_route": yard}
        assert err <= 2.0 * yard, (name, err, yard)


def test_python_errors(torch):
    p = B.make_params(B.WIN_HANN, 10, 16)
    x = torch.zeros((2, 4000), device="cuda")
    xc = torch.zeros((2, 4000), dtype=torch.complex64, device="cuda")
    for fn, n in ((bhw.log_spectrogram, 64), (bhw.log_spectrogram_mixed, 60)):
        with pytest.raises(ValueError, match="real input"):
            fn(p, xc, n, 16)
    with pytest.raises(ValueError, match="log_spectrogram_mixed"):
        bhw.log_spectrogram(p, x, 400, 160)
    with pytest.raises(ValueError, match="bhw.log_spectrogram "):
        bhw.log_spectrogram_mixed(p, x, 512, 160)
    with pytest.raises(ValueError, match="power of two"):
        bhw.log_spectrogram(p, x, 8, 4)
    with pytest.raises(ValueError, match="2\\^a"):
        bhw.log_spectrogram_mixed(p, x, 442, 160)
    fb = bhw.FilterBank(bhw.mel_weights(64, 10, 16000), device="cuda")
    dm = bhw.DctMatrix(bhw.dct_weights(5, 10), device="cuda")
    assert (dm.filters, dm.coeffs, dm.dense().shape, dm.dense().dtype) == (10, 5, (10, 5), np.float32)
    with pytest.raises(ValueError, match="33 bins"):
        bhw.log_spectrogram(p, x, 128, 16, fbank=fb)
    with pytest.raises(ValueError, match="DctMatrix"):
        bhw.log_spectrogram(p, x, 64, 16, fbank=fb, dct=torch.zeros((10, 5), device="cuda"))
    with pytest.raises(ValueError, match="pass fbank"):
        bhw.log_spectrogram(p, x, 64, 16, dct=dm)
    with pytest.raises(ValueError, match="11 rows"):
        bhw.mfcc(p, x, 64, 16, fbank=fb, dct=bhw.DctMatrix(bhw.dct_weights(5, 11), device="cuda"))
    with pytest.raises(ValueError, match="above n_fft"):
        bhw.mfcc(p, x, 16, 8, fbank=bhw.FilterBank(np.ones((9, 17), dtype=np.float32), device="cuda"),
                 dct=bhw.DctMatrix(np.ones((17, 2), dtype=np.float32), device="cuda"))
    with pytest.raises(ValueError, match="CUDA device"):
        bhw.DctMatrix(bhw.dct_weights(5, 10), device="cpu")
    with pytest.raises(ValueError, match="finite"):
        bhw.DctMatrix(np.full((3, 2), np.nan), device="cuda")
    with pytest.raises(ValueError, match="dense"):
        bhw.DctMatrix(np.zeros(5), device="cuda")
    other = bhw.DctMatrix(bhw.dct_weights(5, 10), device="cuda")
    other.device = torch.device("cuda", 1)                                       # a matrix that claims another device
    with pytest.raises(ValueError, match="the DCT matrix is on"):
        bhw.mfcc(p, x, 64, 16, fbank=fb, dct=other)
    for bad in (dict(floor=0.0), dict(floor=-1.0), dict(floor=float("inf")), dict(log="log2"), dict(log=0.0)):
        with pytest.raises(ValueError, match="floor|log must be"):
            bhw.log_spectrogram(p, x, 64, 16, **bad)
    frames = 1 + 4000 // 16
    with pytest.raises(ValueError, match="out must be"):
        bhw.mfcc(p, x, 64, 16, fbank=fb, dct=dm, out=torch.zeros((2, frames, 10), device="cuda"))
    with pytest.raises(ValueError, match="ResidentTable"):
        bhw.mfcc(p, x, 64, 16, fbank=fb, dct=dm, table=object())
    ok = bhw.mfcc(p, x, 64, 16, fbank=fb, dct=dm, out=torch.ones((2, frames, 5), device="cuda"))
    assert tuple(ok.shape) == (2, frames, 5)
    torch.cuda.synchronize()


def test_graph_capture(torch):
    """The four forms captured with no warm call -- library and table, log-mel and MFCC, both radix families; replayed on new data the
    results equal eager calls."""
    p = B.make_params(B.WIN_BH4, 12, 24)
    L, hop, T, nb = 400, 160, 16000, 4
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((nb, T), device="cuda", generator=g) + 5.0
    fbs = {n: bhw.FilterBank(bhw.mel_weights(n, 80, 16000), device="cuda") for n in (400, 512)}     # built before the capture
    dm = bhw.DctMatrix(bhw.dct_weights(13, 80), device="cuda")
    kw = dict(win_length=L, log="ln", floor=1e-6, add=True)

    def calls(tab):
        return [bhw.log_spectrogram(p, x, 512, hop, fbank=fbs[512], **kw), bhw.mfcc(p, x, 512, hop, fbank=fbs[512], dct=dm, **kw),
                bhw.log_spectrogram_mixed(p, x, 400, hop, fbank=fbs[400], **kw), bhw.mfcc_mixed(p, x, 400, hop, fbank=fbs[400], dct=dm, **kw),
                bhw.log_spectrogram(p, x, 512, hop, fbank=fbs[512], table=tab, **kw), bhw.mfcc(p, x, 512, hop, fbank=fbs[512], dct=dm, table=tab, **kw),
                bhw.log_spectrogram_mixed(p, x, 400, hop, fbank=fbs[400], table=tab, **kw),
                bhw.mfcc_mixed(p, x, 400, hop, fbank=fbs[400], dct=dm, table=tab, **kw)]

    with bhw.ResidentTable(p) as tab:
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                outs = calls(tab)
        torch.cuda.current_stream().wait_stream(s)
        x.copy_(torch.randn((nb, T), device="cuda", generator=g) * 3.0 - 2.0)
        for o in outs:
            o.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        eager = calls(tab)
        for o, e in zip(outs, eager):
            assert torch.equal(o, e)
        assert tuple(outs[1].shape) == (nb, 1 + T // hop, 13) and tuple(outs[2].shape) == (nb, 1 + T // hop, 80)
        torch.cuda.synchronize()
