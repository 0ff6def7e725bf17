"""The fused max-hold / min-hold traces for real input on the GPU, both families (bhw_hold_fft_f32_* and bhw_hold_mfft_f32_* through
bhw.hold_fft, bhw.hold_fft_mixed, bhw.hold_fused, bhw.hold_fused_mixed and their ResidentTable forms).

The gate is exact and has no tolerance: with S = bhw.spectrogram(...) (or spectrogram_mixed) of the same call, the traces must be
(S.amax(-2).double() * sk).float() and the same with amin, bit for bit, at every number of frames -- a maximum has no order of
summation.  sk is the per-bin binary64 factor of include/bhw.h: scale * 2.0 for the doubled bins (every bin but 0 and n_fft / 2 under
onesided_doubling), else scale.  For every case of tests/hold_real_cases.py: library and table, the traces each way, the doubling both
ways.  Around it: the extrema of the references are spread over all frames (so no test passes because the extremum sat in slot 0),
planted loud and quiet frames at the edges of a chunk and a block, dead slots of ragged cases, independence of the batch and the
form, NaN and infinity as amax / amin treat them, zeros, sentinels, graph capture with no warm call, and the scipy-shaped fronts
beside welch_fused's mean.

The signals are real noise from a seeded CPU generator, so the seeds can be (and were) checked without a GPU."""
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import hold_real_cases as H

pytestmark = pytest.mark.gpu

CHUNK, BLOCK = B.WELCH_FFT_CHUNK, B.WELCH_BLOCK
SENTINEL = 12345.5
# The seed of a case's noise.  For the cases with F <= 40 and B * K >= 8 F every frame of the reference must be the argmax of some bin
# and the argmin of some bin.  Checked on the CPU on windowed torch.fft.rfft rows of the same noise: with seed 0 the frame with the
# fewest bins to its name has 12 (n1024, n1000, n400-detrend), 26 (n512-detrend), 36 and 37 (n4050, n4096), 65 and 88 (n1536, n2048),
# so every such case keeps seed 0; the assertion itself is on the GPU reference, in the gate.
SEEDS = {"fft-n1024-1x21-padded": 0, "fft-n2048-2x18": 0, "fft-n4096-detrend-1x35": 0, "fft-n128-2x1": 0, "fft-n512-detrend-2x15": 0,
         "mfft-n1000-1x21-padded": 0, "mfft-n1536-2x18-form1": 0, "mfft-n4050-detrend-1x35": 0, "mfft-n400-2x1": 0,
         "mfft-n400-detrend-2x15": 0}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _noise(torch, nb, T, seed):
    """(B, T) float32 on the device: noise of 1000 from a seeded CPU generator."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((nb, T), generator=g, dtype=torch.float32) * 1000).cuda()


def _fns(fam, tab=None):
    """(hold, spectrogram) of a family: the library forms, or the table's hold."""
    src = tab if tab is not None else bhw
    if fam == "fft":
        return src.hold_fft, bhw.spectrogram
    return src.hold_fft_mixed, bhw.spectrogram_mixed


def _kw(c):
    if c["detrend"]:
        return dict(win_length=c["L"], center=False, detrend=True)
    return dict(win_length=c["L"], center=bool(c["mode"]), pad_mode=c["mode"] or "reflect", detrend=False)


def _sk(torch, n, scale, doubled):
    """The per-bin binary64 factor of the contract: scale * 2.0 where bhw_psd_doubled holds (every bin but 0 and n_fft / 2), else scale."""
    K = n // 2 + 1
    sk = torch.full((K,), float(scale), dtype=torch.float64, device="cuda")
    if doubled:
        sk[1:K - 1] = float(scale) * 2.0
    return sk


def _want(S, sk):
    """The contract on the power rows S (..., F, K): the reduction over the frames, times s_k in binary64, rounded once."""
    return (S.amax(-2).double() * sk).float(), (S.amin(-2).double() * sk).float()


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """Bit for bit where neither is a NaN, and a NaN exactly where the other has one (any quiet NaN)."""
    import torch
    if a.shape != b.shape:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool((na == nb).all()) and bool((_bits(a)[~na] == _bits(b)[~nb]).all())


def _x_of(torch, c):
    return _noise(torch, c["B"], H._MOD[c["family"]].frames_to_samples(c), SEEDS.get(c["id"], 0))


# ---- the gate ----------------------------------------------------------------------------------------------------------------------------

def test_the_seeded_cases_are_exactly_those_the_condition_names():
    named = set()
    for c in H.CASES:
        _, _, F, _ = H.desc(c["family"], c)
        if F <= 40 and c["B"] * (c["n_fft"] // 2 + 1) >= 8 * F:
            named.add(c["id"])
    assert named == set(SEEDS)


@pytest.mark.parametrize("cid", H.case_ids())
def test_every_case_equals_amax_and_amin_of_the_power_rows_bit_for_bit(torch, cid):
    c = H.case(cid)
    fam, n, nb = c["family"], c["n_fft"], c["B"]
    K = n // 2 + 1
    p = H.params(c["setup"])
    _, _, F, _ = H.desc(fam, c)
    x = _x_of(torch, c)
    scale = 1.0 / (3.7 * F)
    hold, spectro = _fns(fam)
    S = spectro(p, x, n, c["hop"], **_kw(c))                           # the rows the contract is stated on
    assert S.shape == (nb, F, K) and S.dtype == torch.float32
    if F <= 40 and nb * K >= 8 * F:
        # the extrema of the REFERENCE are spread: every frame is the argmax of some bin and the argmin of some bin
        assert cid in SEEDS
        assert set(S.argmax(-2).flatten().tolist()) == set(range(F)), cid
        assert set(S.argmin(-2).flatten().tolist()) == set(range(F)), cid
    ragged = F % CHUNK != 0
    with bhw.ResidentTable(p) as tab:
        d = H.parse(fam, H.line(fam, c, table=tab._live()))
        assert d["table"] and d["frames"] == F
        for doubled in (True, False):
            wmax, wmin = _want(S, _sk(torch, n, scale, doubled))
            for form, fn in (("library", hold), ("table", _fns(fam, tab)[0])):
                for traces in H.TRACES:
                    if c.get("padded") and form == "library":
                        buf = torch.full((2, nb, K + 5), SENTINEL, device="cuda")
                        outs = dict(out_max=buf[0, :, :K] if traces != "min" else None, out_min=buf[1, :, :K] if traces != "max" else None)
                        pmax, pmin = fn(p, x, n, c["hop"], scale, onesided_doubling=doubled, traces=traces, **outs, **_kw(c))
                        assert bool((buf[:, :, K:] == SENTINEL).all()), "a gap was written"
                        if traces == "max":
                            assert bool((buf[1] == SENTINEL).all()), "the trace not asked for was written"
                        if traces == "min":
                            assert bool((buf[0] == SENTINEL).all()), "the trace not asked for was written"
                    else:
                        pmax, pmin = fn(p, x, n, c["hop"], scale, onesided_doubling=doubled, traces=traces, **_kw(c))
                    assert (pmax is None) == (traces == "min") and (pmin is None) == (traces == "max"), (cid, traces)
                    if pmax is not None:
                        assert pmax.dtype == torch.float32 and torch.equal(pmax, wmax), (cid, form, doubled, traces, "max")
                    if pmin is not None:
                        assert pmin.dtype == torch.float32 and torch.equal(pmin, wmin), (cid, form, doubled, traces, "min")
                        if ragged:                                     # a dead slot is a zero row: one read of it and the minimum is 0
                            assert bool((pmin[wmin > 0] > 0).all()) and bool((wmin > 0).any()), (cid, form, doubled)


@pytest.mark.parametrize("fam,n,hop,nb", [("fft", 64, 64, 2), ("mfft", 200, 208, 2), ("fft", 512, 512, 2)])
def test_planted_loud_and_quiet_frames_at_the_edges_of_a_chunk_and_a_block(torch, fam, n, hop, nb):
    """Disjoint frames (hop >= L), no detrend, F = 259; the samples of ONE frame times 2^10, then times 2^-10: that frame is the
    maximum (the minimum) of most bins -- asserted on the reference -- and the traces still equal it everywhere.  64: a group holds
    whole chunks; 200: lane values are carried over a run; 512: bin M is reduced aside on lane 0."""
    p = H.params(0)
    F = BLOCK + 3
    K = n // 2 + 1
    hold, spectro = _fns(fam)
    kw = dict(win_length=n, center=False, detrend=False)
    base = _noise(torch, nb, (F - 1) * hop + n, 7)
    sk = _sk(torch, n, 0.25, True)
    with bhw.ResidentTable(p) as tab:
        for f in (0, CHUNK - 1, CHUNK, BLOCK, F - 1):
            for gain, pick in ((2.0 ** 10, "argmax"), (2.0 ** -10, "argmin")):
                x = base.clone()
                x[:, f * hop:f * hop + n] *= gain
                S = spectro(p, x, n, hop, **kw)
                assert S.shape == (nb, F, K)
                where = getattr(S, pick)(-2)
                assert int((where == f).sum()) > nb * K // 2, (fam, f, pick)
                wmax, wmin = _want(S, sk)
                for fn in (hold, _fns(fam, tab)[0]):
                    pmax, pmin = fn(p, x, n, hop, 0.25, **kw)
                    assert torch.equal(pmax, wmax) and torch.equal(pmin, wmin), (fam, f, pick)


# ---- independence, specials, sentinels -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam,n,L,hop,F", [("fft", 64, 50, 16, 40), ("fft", 512, 400, 160, 40), ("fft", 4096, 4096, 1024, 20),
                                           ("mfft", 60, 50, 16, 40), ("mfft", 400, 400, 160, 40), ("mfft", 1536, 1536, 512, 20)])
def test_a_signal_alone_and_as_number_37_of_64_give_the_same_words(torch, fam, n, L, hop, F):
    p = H.params(0)
    K = n // 2 + 1
    x = _noise(torch, 64, (F - 1) * hop + n, n)
    kw = dict(win_length=L, detrend=False)
    hold, _ = _fns(fam)
    M, m = hold(p, x, n, hop, 0.01, **kw)
    one = hold(p, x[37], n, hop, 0.01, **kw)
    assert one[0].shape == (K,) and torch.equal(one[0], M[37]) and torch.equal(one[1], m[37])
    a, b = hold(p, x[37:38], n, hop, 0.01, **kw)
    assert torch.equal(a[0], M[37]) and torch.equal(b[0], m[37])
    with bhw.ResidentTable(p) as tab:
        th = _fns(fam, tab)[0]
        Mt, mt = th(p, x, n, hop, 0.01, **kw)
        assert torch.equal(Mt, M) and torch.equal(mt, m)
        a, b = th(p, x[37], n, hop, 0.01, **kw)
        assert torch.equal(a, M[37]) and torch.equal(b, m[37])


@pytest.mark.parametrize("cid", ["fft-n64-3x17", "fft-n512-l400-3x259", "fft-n128-l100-detrend-2x33", "mfft-n50-3x17", "mfft-n400-3x259",
                                 "mfft-n96-l80-detrend-2x33"])
def test_nan_and_infinity_are_amax_and_amins(torch, cid):
    c = H.case(cid)
    fam, n = c["family"], c["n_fft"]
    p = H.params(c["setup"])
    hold, spectro = _fns(fam)
    x = _x_of(torch, c)
    sk = _sk(torch, n, 0.5, True)
    cm, cn = hold(p, x, n, c["hop"], 0.5, **_kw(c))
    assert bool(torch.isfinite(cm).all()) and bool(torch.isfinite(cn).all())
    bad = c["B"] - 1
    keep = [b for b in range(c["B"]) if b != bad]
    for value in (float("nan"), float("inf")):
        y = x.clone()
        y[bad, y.shape[1] // 2] = value                               # one sample of one signal
        wmax, wmin = _want(spectro(p, y, n, c["hop"], **_kw(c)), sk)
        pmax, pmin = hold(p, y, n, c["hop"], 0.5, **_kw(c))
        assert bool((torch.isnan(pmax) == torch.isnan(wmax)).all()) and bool((torch.isnan(pmin) == torch.isnan(wmin)).all()), cid
        assert _same(pmax, wmax) and _same(pmin, wmin), cid
        assert bool((torch.isnan(pmax) == torch.isnan(pmin)).all()), "a NaN power makes both traces NaN"
        assert torch.equal(pmax[keep], cm[keep]) and torch.equal(pmin[keep], cn[keep]), cid
        assert not bool(torch.isfinite(pmax[bad]).any()), cid
        if value != value:
            # the NaN reaches some frame of every bin of its own signal: exactly that signal's bins are NaN, in both traces
            assert bool(torch.isnan(pmax[bad]).all()) and bool(torch.isnan(pmin[bad]).all()) and not bool(torch.isnan(pmax[keep]).any()), cid
        # each trace alone sees the same NaNs: the minimum takes them from the maximum inside the kernel
        only_min = hold(p, y, n, c["hop"], 0.5, traces="min", **_kw(c))[1]
        assert _same(only_min, wmin), cid


@pytest.mark.parametrize("cid", ["fft-n16-2x70", "fft-n256-l200-detrend-2x40", "fft-n4096-detrend-1x35", "mfft-n18-l13-detrend-2x70",
                                 "mfft-n400-3x259", "mfft-n4050-detrend-1x35"])
def test_zeros_in_give_positive_zero_out(torch, cid):
    c = H.case(cid)
    p = H.params(c["setup"])
    x = torch.zeros((c["B"], H._MOD[c["family"]].frames_to_samples(c)), dtype=torch.float32, device="cuda")
    for doubled in (True, False):
        for t in _fns(c["family"])[0](p, x, c["n_fft"], c["hop"], 0.25, onesided_doubling=doubled, **_kw(c)):
            assert bool((_bits(t) == 0).all()), cid                   # +0.0: not -0.0, not a denormal


@pytest.mark.parametrize("cid", ["fft-n64-3x17", "fft-n512-l400-3x259", "mfft-n50-3x17", "mfft-n400-3x259", "mfft-n1536-2x18-form1"])
def test_sentinels_around_the_outputs_in_the_gaps_and_behind_the_workspace_are_untouched(torch, cid):
    c = H.case(cid)
    fam, n, nb = c["family"], c["n_fft"], c["B"]
    K = n // 2 + 1
    p = H.params(c["setup"])
    hold, _ = _fns(fam)
    x = _x_of(torch, c)
    need = H.HOLD_WS[fam](H.desc(fam, c)[0]) // 8
    assert need == H.WF.workspace_doubles(nb, c["F"], K)
    want = hold(p, x, n, c["hop"], 0.5, **_kw(c))
    for traces in H.TRACES:
        buf = torch.full((2, nb + 2, K + 7), SENTINEL, device="cuda")          # a row before and behind each output, a gap in each row
        ws = torch.full((need + 3,), SENTINEL, dtype=torch.float64, device="cuda")
        outs = dict(out_max=buf[0, 1:nb + 1, :K] if traces != "min" else None, out_min=buf[1, 1:nb + 1, :K] if traces != "max" else None)
        pmax, pmin = hold(p, x, n, c["hop"], 0.5, traces=traces, workspace=ws[:need], **outs, **_kw(c))
        torch.cuda.synchronize()
        for i, (got, w) in enumerate(((pmax, want[0]), (pmin, want[1]))):
            if got is None:
                assert bool((buf[i] == SENTINEL).all()), "the trace not asked for was written"
                continue
            assert got.data_ptr() == buf[i, 1].data_ptr() and torch.equal(got, w)
            assert bool((buf[i, 0] == SENTINEL).all()) and bool((buf[i, nb + 1] == SENTINEL).all()) and bool((buf[i, :, K:] == SENTINEL).all())
        assert bool((ws[need:] == SENTINEL).all()), "the workspace's end was written"
        assert not bool((ws[:need] == SENTINEL).any()), "a chunk or block pair was not written"
    with pytest.raises(ValueError, match="workspace"):
        hold(p, x, n, c["hop"], 0.5, workspace=ws[:need - 1], **_kw(c))
    with pytest.raises(ValueError, match="out_min is given but traces='max'"):
        hold(p, x, n, c["hop"], 0.5, traces="max", out_min=torch.empty((nb, K), device="cuda"), **_kw(c))
    with pytest.raises(ValueError, match="out_max must be"):
        hold(p, x, n, c["hop"], 0.5, out_max=torch.empty((nb, K + 1), device="cuda"), **_kw(c))
    with pytest.raises(ValueError, match="same row stride"):
        hold(p, x, n, c["hop"], 0.5, out_max=torch.empty((nb, K), device="cuda"), out_min=torch.empty((nb, K + 4), device="cuda")[:, :K], **_kw(c))


def test_what_the_calls_refuse_names_the_call_that_takes_it(torch):
    p = H.params(0)
    x = _noise(torch, 2, 8000, 3)
    with pytest.raises(ValueError, match="n_fft 400 is mixed-radix: hold_fft_mixed / hold_fused_mixed transform it"):
        bhw.hold_fft(p, x, 400, 160)
    with pytest.raises(ValueError, match="n_fft 512 is a power of two: hold_fft / hold_fused transform it"):
        bhw.hold_fft_mixed(p, x, 512, 160)
    z = torch.complex(x, x)
    with pytest.raises(ValueError, match="hold_fft_iq / hold_fused_iq"):
        bhw.hold_fft(p, z, 512, 160)
    with pytest.raises(ValueError, match="hold_fft_iq_mixed / hold_fused_iq_mixed"):
        bhw.hold_fused_mixed(p, z, length=400)
    with pytest.raises(ValueError, match="complex64"):                  # hold_fft_iq refuses real input as before
        bhw.hold_fft_iq(p, x, 512, 160)


# ---- graph capture -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam,n", [("fft", 256), ("mfft", 400)])
def test_the_library_form_is_captured_with_no_warm_call_on_a_two_block_shape(torch, fam, n):
    """Outputs and workspace given: the call neither allocates nor synchronises, so its FIRST call may be the captured one; the kernel
    and both join launches are in the graph.  The parameters are this test's own, so that no earlier call warmed them."""
    p = B.make_params(B.WIN_BH5, 11, 27)
    hop, nb, F = 96, 3, BLOCK + 44
    K = n // 2 + 1
    T = (F - 1) * hop + n
    hold, spectro = _fns(fam)
    x = _noise(torch, nb, T, 21)
    ws = torch.empty(H.HOLD_WS[fam](B.make_stft(nb, T, F, hop, n)) // 8, dtype=torch.float64, device="cuda")
    om, on = torch.full((nb, K), -1.0, device="cuda"), torch.full((nb, K), -1.0, device="cuda")
    kw = dict(win_length=n, center=False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            pmax, pmin = hold(p, x, n, hop, 0.125, out_max=om, out_min=on, workspace=ws, **kw)
    torch.cuda.current_stream().wait_stream(s)
    assert pmax.data_ptr() == om.data_ptr() and pmin.data_ptr() == on.data_ptr()
    x.copy_(_noise(torch, nb, T, 22) * 3.0)
    graph.replay()
    torch.cuda.synchronize()
    em, en = hold(p, x, n, hop, 0.125, **kw)                             # the eager result on the new data
    assert torch.equal(pmax, em) and torch.equal(pmin, en)
    wmax, wmin = _want(spectro(p, x, n, hop, **kw), _sk(torch, n, 0.125, True))
    assert torch.equal(pmax, wmax) and torch.equal(pmin, wmin) and bool((pmin > 0).all())


# ---- the scipy-shaped fronts ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam,nfft", [("fft", 512), ("mfft", 400)])
def test_hold_fused_brackets_welch_fused_and_is_hold_fft_at_the_per_frame_scale(torch, fam, nfft):
    p = B.make_params(B.WIN_BH7, 12, 32)
    hop, nb, fs = 150, 3, 30720.0
    K = nfft // 2 + 1
    fused, hold, welch = ((bhw.hold_fused, bhw.hold_fft, bhw.welch_fused) if fam == "fft" else
                          (bhw.hold_fused_mixed, bhw.hold_fft_mixed, bhw.welch_fused_mixed))
    for L, detrends in ((360, ("constant",)), (nfft, ("constant", False))):
        F = 21 if L < nfft else 300                                   # one block and two
        T = (F - 1) * hop + L + 17
        x = _noise(torch, nb, T, 40)
        sums = bhw.window_sums(p, L, f32=True)
        for scaling in ("density", "spectrum"):
            for detrend in detrends:
                kw = dict(length=L, noverlap=L - hop, nfft=nfft, detrend=detrend, scaling=scaling)
                f, pmax, pmin = fused(p, x, fs, **kw)
                fw, Pxx = welch(p, x, fs, **kw)
                assert f is fw                                        # welch_fused's tensor: the same cache, the same key
                wm, wn = hold(p, x, nfft, hop, B.welch_scale(sums, 1, fs, scaling), win_length=L, detrend=detrend == "constant")
                assert pmax.shape == (nb, K) and torch.equal(pmax, wm) and torch.equal(pmin, wn), (L, scaling, detrend)
                # two float32 roundings on a trace, one on the mean, and F * 2^-53 on its sum: 2^-22 covers them
                lo, hi = pmin.double() * (1 - 2.0 ** -22), pmax.double() * (1 + 2.0 ** -22)
                assert bool((lo <= Pxx.double()).all()) and bool((Pxx.double() <= hi).all()), (L, scaling, detrend)
                assert bool((pmin < pmax).all())
    # a 1-D x gives 1-D traces; one trace alone; the table's form
    f, pmax, pmin = fused(p, x[0], fs, length=nfft, traces="max")
    assert pmax.shape == (K,) and pmin is None and f.shape == (K,)
    with bhw.ResidentTable(p) as tab:
        tf = tab.hold_fused if fam == "fft" else tab.hold_fused_mixed
        ft, tmax, tmin = tf(p, x, fs, length=nfft, noverlap=nfft - hop)
        fl, lmax, lmin = fused(p, x, fs, length=nfft, noverlap=nfft - hop)
        assert torch.equal(ft, fl) and torch.equal(tmax, lmax) and torch.equal(tmin, lmin)
        assert tf(p, x, fs, length=nfft, noverlap=nfft - hop)[0] is ft
    with pytest.raises(ValueError, match="traces must be"):
        fused(p, x, fs, length=nfft, traces="median")
    with pytest.raises(TypeError):
        fused(p, x, fs, length=nfft, average="median")
