"""Every SciPy-shaped spectral front on the GPU against the float64 restatements of SciPy of tests/spectral_front_cases.py (themselves
held to SciPy by tests/test_spectral_front_cases.py), bin by bin on flat spectra: welch (fft="torch" and "fused", real and complex
input), welch_fused, welch_fused_mixed, welch_fused_iq, welch_fused_iq_mixed, hold_fused and its three siblings, cross_spectra (both
routes), csd, coherence, transfer_function and the *_fused forms of the four, each as the library call and as the ResidentTable method.

Per case and front: the library form and the table form are equal word for word; so is the 1-D form against row 0, or the row-strided x
against the contiguous one (the case's layout says which); the I/Q fronts run fftshift both ways and the shifted result is fftshift of
the unshifted one word for word.  The window given to the reference is bhw.window(p, L, dtype=float32) of the same parameters.

Gates, both: the RMS figure at most 2x the yardstick's, the maximum at most 4x the yardstick's maximum, the yardstick being the
torch-only float32 route on the same GPU through the same metric (unfold, subtract the mean, multiply, torch.fft, abs() ** 2, then mean /
amax / amin in float64; the cross spectra from the same float32 spectra in complex128).  2x is the project's standing gate against a
float32 library route; 4x on a maximum of B K draws allows for the spread of an extreme value between two honest float32 routes; what
the suite is after (a doubling, a scale, a frame count, a bin, a conjugate) is at least 0.1 in these metrics.  The yardstick itself
must stay under 64 caps (cap = 2^-24 log2 nfft) in every case, six times the CPU stand-in's worst figure (10.6 caps, a max-hold), so
that a broken yardstick cannot pass everything.  Bins 0 and nfft / 2 of the one-sided fronts have a line of their own, held to those
64 caps (see _gate).  Pxy and H1 are gated in the coherent cases only (spectral_front_cases.INCOHERENT).  The fused cross spectra take
nfft up to 2048: at 4096 cross_spectra_fused must refuse and cross_spectra runs both of its routes.  Every figure is printed before
anything is asserted: fused, yardstick, ratio, fused / cap; profiles/r32_spectral_fronts.txt keeps one run's lines.

Broken on purpose in a scratch copy, each caught: the Nyquist exception of the doubling dropped (all 36 one-sided cases of the welch
and hold tests, at the edge-bin line and the maximum; no I/Q case); S1^2 and S2 swapped in welch_scale (every case); L // 2 + 1 as the
default overlap (the `defaults` case of every size and family, and nothing else); the other factor of Pxy conjugated (every cross case:
H1 off by 2.0 in the printed line, csd(x, x)'s -0.0).  Zero-padding around the segment is a linear phase that cancels in |X|^2 and in
conj(X) Y: no output of these fronts can show it, and tests/test_spectral_front_cases.py proves that on the references."""
import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import plan_cases as PC
import spectral_front_cases as C

pytestmark = pytest.mark.gpu

RMS_GATE, MAX_GATE, YARDSTICK_CAPS = 2.0, 4.0, 64.0


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_TABLES, _STATES = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_tables():
    yield
    for t in _TABLES.values():
        t.close()
    _TABLES.clear()
    _STATES.clear()


def _params(setup):
    win, P, W, kw = PC.SETUPS[setup]
    return B.make_params(win, P, W, **kw)


def _state(torch, cid):
    """The inputs, window, references and yardstick of case `cid`, computed once and shared by the tests of the case."""
    if cid in _STATES:
        return _STATES[cid]
    c = C.case(cid)
    p = _params(c["setup"])
    if c["setup"] not in _TABLES:
        _TABLES[c["setup"]] = bhw.ResidentTable(p)
    xh, yh = C.signals(c)
    v = bhw.window(p, c["L"], dtype=torch.float32)
    st = dict(c=c, p=p, table=_TABLES[c["setup"]], v=v, x=torch.from_numpy(xh).cuda(), y=None if yh is None else torch.from_numpy(yh).cuda())
    st["ref"] = C.references(c, v.cpu().numpy(), xh, yh)
    st["yard"] = _yardstick(torch, c, st["x"], st["y"], v)
    st["fails"] = []
    _STATES[cid] = st
    return st


def _strided(torch, t):
    return torch.from_numpy(C.strided(t.cpu().numpy())).cuda()[:, :t.shape[-1]]


def _double(P, n):
    P[..., 1:] *= 2.0
    if n % 2 == 0:
        P[..., -1] /= 2.0
    return P


def _yardstick(torch, c, x, y, v):
    """The torch-only float32 route: references()'s keys as NumPy float64 / complex128."""
    L, hop, n = c["L"], c["hop"], c["nfft"]
    vd = v.double()
    scale = 1.0 / (c["fs"] * float((vd * vd).sum())) if c["scaling"] == "density" else 1.0 / float(vd.sum()) ** 2

    def spectra(t):
        seg = t.unfold(-1, L, hop)
        if c["detrend"]:
            seg = seg - seg.mean(-1, keepdim=True)
        seg = seg * v
        return torch.fft.fft(seg, n=n) if c["iq"] else torch.fft.rfft(seg, n=n)

    X = spectra(x)
    assert X.dtype == torch.complex64 and X.shape[-2] == c["F"]
    S = (X.abs() ** 2).double() * scale
    S = (torch.fft.fftshift(S, dim=-1) if c["fftshift"] else S) if c["iq"] else _double(S, n)
    # a float32 route returns float32: the sums are binary64, what comes back is rounded once, as the library's outputs are
    out = {"mean": S.mean(-2).float().cpu().numpy(), "max": S.amax(-2).float().cpu().numpy(), "min": S.amin(-2).float().cpu().numpy()}
    if y is not None:
        Xd, Yd = X.to(torch.complex128), spectra(y).to(torch.complex128)
        pxy = _double((Xd.conj() * Yd).mean(-2) * scale, n)
        pxx = _double((Xd.real ** 2 + Xd.imag ** 2).mean(-2) * scale, n)
        pyy = _double((Yd.real ** 2 + Yd.imag ** 2).mean(-2) * scale, n)
        cross = {"pxy": pxy, "pxx": pxx, "pyy": pyy, "coherence": pxy.abs() ** 2 / (pxx * pyy), "h1": pxy / pxx}
        out["cross"] = {k: t.to(torch.complex64 if t.is_complex() else torch.float32).cpu().numpy() for k, t in cross.items()}
    return out


# ---- call forms ----------------------------------------------------------------------------------------------------------------------

def _words(torch, t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.uint8)


def _same(torch, a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(_words(torch, a[k]), _words(torch, b[k])), (what, k)


def _forms(torch, st, name, call, two=False):
    """call(obj, p, x[, y]) -> dict of tensors ("freqs" and the outputs).  Runs the library form and the table form on the contiguous
    (3, T) rows, and the 1-D form or the row-strided form where the case's layout names it, all equal word for word; returns the
    library form's dict on the rows."""
    c, p = st["c"], st["p"]
    ins = (st["x"], st["y"]) if two else (st["x"],)
    lib = call(bhw, p, *ins)
    _same(torch, lib, call(st["table"], p, *ins), f"{c['id']} {name}: the ResidentTable form")
    if c["layout"] == "1d":
        row0 = {k: (t if k == "freqs" or t is None else t[0]) for k, t in lib.items()}
        _same(torch, row0, call(bhw, p, *(t[0] for t in ins)), f"{c['id']} {name}: the 1-D form against row 0")
        _same(torch, row0, call(st["table"], p, *(t[0] for t in ins)), f"{c['id']} {name}: the 1-D table form against row 0")
    elif c["layout"] == "strided":
        wide = tuple(_strided(torch, t) for t in ins)
        assert all(not t.is_contiguous() for t in wide)
        _same(torch, lib, call(bhw, p, *wide), f"{c['id']} {name}: row-strided x against contiguous x")
        _same(torch, lib, call(st["table"], p, *wide), f"{c['id']} {name}: row-strided x, table form")
    return lib


def _freqs(torch, st, f):
    c = st["c"]
    assert f.dtype == torch.float64 and np.allclose(f.cpu().numpy(), st["ref"]["freqs"], rtol=0, atol=1e-15 * c["fs"] * c["nfft"]), c["id"]


# ---- gates ---------------------------------------------------------------------------------------------------------------------------

def _gate(st, front, quantity, got, yard, edge=False):
    """Prints the line of (front, quantity) and records what misses a gate; the test asserts at its end, after every line is out.
    edge: the line of bins 0 and nfft / 2 alone, 2 B = 6 draws (B = 3 for an odd nfft).  The ratio gates rest on many draws: the RMS of
    six draws of one honest route against six of another scatters by a factor of two either way at a few cases in a hundred (the
    square root of an F(6, 6) variate), so these bins are held to the allowance of an honest float32 route itself, YARDSTICK_CAPS caps,
    on the fused figure as on the yardstick's.  A doubling or a missed doubling there is 0.5 or 1.0: four orders above."""
    c = st["c"]
    cap = C.cap(c)
    (gm, gr), (ym, yr) = got, yard
    ratio = lambda a, b: a / b if b > 0 else (0.0 if a == 0 else float("inf"))      # noqa: E731
    print(f"{c['id']} {front} {quantity}: fused max {gm:.3e} rms {gr:.3e}, yardstick max {ym:.3e} rms {yr:.3e}, ratio max "
          f"{ratio(gm, ym):.2f} rms {ratio(gr, yr):.2f}, fused / cap max {gm / cap:.2f} rms {gr / cap:.2f}")
    if ym > YARDSTICK_CAPS * cap:
        st["fails"].append(f"{front} {quantity}: the yardstick's maximum is {ym / cap:.1f} caps, above {YARDSTICK_CAPS}")
    if edge:
        if gm > YARDSTICK_CAPS * cap:
            st["fails"].append(f"{front} {quantity}: max {gm:.3e} is {gm / cap:.1f} caps, above {YARDSTICK_CAPS}")
        return
    if gr > RMS_GATE * yr:
        st["fails"].append(f"{front} {quantity}: rms {gr:.3e} above {RMS_GATE} x the yardstick's {yr:.3e}")
    if gm > MAX_GATE * ym:
        st["fails"].append(f"{front} {quantity}: max {gm:.3e} above {MAX_GATE} x the yardstick's {ym:.3e}")


def _done(st):
    fails, st["fails"] = st["fails"], []
    assert not fails, "\n".join([st["c"]["id"]] + fails)


def _np(t):
    return t.cpu().numpy()


def _gate_psd(st, front, P, key="mean", ref=None, yard=None):
    """The mean PSD (or Pxx / Pyy) of a front through rel, and bins 0 and nfft / 2 of a one-sided front on their own."""
    c = st["c"]
    ref = st["ref"][key] if ref is None else ref
    yard = st["yard"][key] if yard is None else yard
    P = _np(P)
    _gate(st, front, key, C.rel(P, ref), C.rel(yard, ref))
    if not c["iq"]:
        e = C.edge_bins(c)
        _gate(st, front, f"{key}, bins {e}", C.rel(P[:, e], ref[:, e]), C.rel(yard[:, e], ref[:, e]), edge=True)


# ---- the mean ------------------------------------------------------------------------------------------------------------------------

def _welch_call(name, **extra):
    def call(obj, p, x):
        f, P = getattr(obj, name)(p, x, call.fs, **call.kw, **extra)
        return {"freqs": f, "pxx": P}
    return call


def _bind(call, c):
    call.fs, call.kw = c["fs"], C.kwargs(c)
    return call


@pytest.mark.parametrize("cid", C.case_ids())
def test_welch_fronts_equal_scipy_bin_by_bin(torch, cid):
    st = _state(torch, cid)
    c = st["c"]
    fronts = [n for n in C.FRONTS[c["family"]] if n.startswith("welch")]
    assert fronts
    for name in fronts:
        if name == "welch":
            routes = ("torch",) if c["iq"] or c["torch_only"] else ("torch", "fused")
            for fft in routes:
                res = _forms(torch, st, f"welch[{fft}]", _bind(_welch_call("welch", fft=fft), c))
                P, f = res["pxx"], res["freqs"]
                if c["iq"]:
                    # complex input: the two-sided spectrum whatever return_onesided says, as scipy does; the case's shift is the test's
                    assert P.shape == (C.NB, c["nfft"])
                    two = _bind(_welch_call("welch", fft=fft, return_onesided=False), c)(bhw, st["p"], st["x"])
                    _same(torch, res, two, f"{cid} welch: return_onesided is ignored for complex input")
                    if c["fftshift"]:
                        P, f = torch.fft.fftshift(P, dim=-1), torch.fft.fftshift(f)
                _freqs(torch, st, f)
                _gate_psd(st, f"welch[{fft}]", P)
        elif not c["torch_only"]:
            if c["iq"]:
                res = _forms(torch, st, name, _bind(_welch_call(name, fftshift=c["fftshift"]), c))
                other = _bind(_welch_call(name, fftshift=not c["fftshift"]), c)(bhw, st["p"], st["x"])
                plain, shifted = (other, res) if c["fftshift"] else (res, other)
                _same(torch, shifted, {k: torch.fft.fftshift(t, dim=-1) for k, t in plain.items()},
                      f"{cid} {name}: fftshift=True is fftshift of fftshift=False")
            else:
                res = _forms(torch, st, name, _bind(_welch_call(name), c))
            _freqs(torch, st, res["freqs"])
            _gate_psd(st, name, res["pxx"])
    _done(st)


# ---- the traces ------------------------------------------------------------------------------------------------------------------------

def _hold_call(name, **extra):
    def call(obj, p, x):
        f, pmax, pmin = getattr(obj, name)(p, x, call.fs, **call.kw, **extra)
        return {"freqs": f, "max": pmax, "min": pmin}
    return call


@pytest.mark.parametrize("cid", C.case_ids(fused_only=True))
def test_hold_fronts_equal_scipys_spectrogram_reduced_over_time(torch, cid):
    st = _state(torch, cid)
    c, ref, yard = st["c"], st["ref"], st["yard"]
    (name,) = [n for n in C.FRONTS[c["family"]] if n.startswith("hold_fused")]
    extra = {"fftshift": c["fftshift"]} if c["iq"] else {}
    res = _forms(torch, st, name, _bind(_hold_call(name, traces=c["traces"], **extra), c))
    if c["iq"]:
        other = _bind(_hold_call(name, traces=c["traces"], fftshift=not c["fftshift"]), c)(bhw, st["p"], st["x"])
        plain, shifted = (other, res) if c["fftshift"] else (res, other)
        _same(torch, shifted, {k: None if t is None else torch.fft.fftshift(t, dim=-1) for k, t in plain.items()},
              f"{cid} {name}: fftshift=True is fftshift of fftshift=False")
    _freqs(torch, st, res["freqs"])
    asked = {"both": ("max", "min"), "max": ("max",), "min": ("min",)}[c["traces"]]
    slack = YARDSTICK_CAPS * C.cap(c)
    for key in ("max", "min"):
        if key not in asked:
            assert res[key] is None, (cid, key)
            continue
        P = _np(res[key])
        _gate(st, name, f"{key}-hold", C.hold_rel(P, ref[key], ref["mean"]), C.hold_rel(yard[key], ref[key], ref["mean"]))
        if not c["iq"]:
            e = C.edge_bins(c)
            _gate(st, name, f"{key}-hold, bins {e}", C.hold_rel(P[:, e], ref[key][:, e], ref["mean"][:, e]),
                  C.hold_rel(yard[key][:, e], ref[key][:, e], ref["mean"][:, e]), edge=True)
        # the traces bracket the reference mean bin by bin (one segment: all three are one number, to a float32 route's error)
        if key == "max":
            assert (P.astype(np.float64) >= ref["mean"] * (1.0 - slack)).all(), (cid, "pmax below the reference mean")
        else:
            assert (P.astype(np.float64) <= ref["mean"] * (1.0 + slack)).all(), (cid, "pmin above the reference mean")
    _done(st)


# ---- the cross spectra -----------------------------------------------------------------------------------------------------------------

def _cross_call(name, **extra):
    def call(obj, p, x, y):
        f, r = getattr(obj, name)(p, x, y, call.fs, **call.kw, **extra)
        return dict(r, freqs=f)
    return call


def _single_call(name, output, **extra):
    def call(obj, p, x, y):
        f, t = getattr(obj, name)(p, x, y, call.fs, **call.kw, **extra)
        return {"freqs": f, output: t}
    return call


def _gate_cross(st, front, res):
    c, ref, yard = st["c"], st["ref"]["cross"], st["yard"]["cross"]
    for key, metric in C.CROSS_METRICS.items():
        if key not in res or (key in ("pxy", "h1") and not c["coherent"]):
            continue
        if key in ("pxx", "pyy"):
            _gate_psd(st, front, res[key], key, ref[key], yard[key])
            continue
        _gate(st, front, key, metric(_np(res[key]), ref[key]), metric(yard[key], ref[key]))
        if key == "pxy":
            e = C.edge_bins(c)
            _gate(st, front, f"pxy, bins {e}", C.rel(_np(res[key])[:, e], ref[key][:, e]), C.rel(yard[key][:, e], ref[key][:, e]), edge=True)


@pytest.mark.parametrize("cid", C.case_ids("real"))
def test_cross_fronts_equal_scipy_bin_by_bin(torch, cid):
    st = _state(torch, cid)
    c, ref = st["c"], st["ref"]["cross"]
    routes = ("torch",) if c["torch_only"] else ("torch", "fused")
    fused = not c["torch_only"] and c["nfft"] <= C.CSD_FUSED_MAX_N
    for fft in routes:
        res = _forms(torch, st, f"cross_spectra[{fft}]", _bind(_cross_call("cross_spectra", fft=fft), c), two=True)
        assert set(res) == {"freqs", "pxy", "pxx", "pyy", "coherence", "h1"}
        _freqs(torch, st, res["freqs"])
        _gate_cross(st, f"cross_spectra[{fft}]", res)
    one = routes[c["pos"] % len(routes)]
    for name, output in (("csd", "pxy"), ("coherence", "coherence"), ("transfer_function", "h1")):
        res = _forms(torch, st, f"{name}[{one}]", _bind(_single_call(name, output, fft=one), c), two=True)
        _freqs(torch, st, res["freqs"])
        _gate_cross(st, f"{name}[{one}]", res)
    if fused:
        res = _forms(torch, st, "cross_spectra_fused", _bind(_cross_call("cross_spectra_fused"), c), two=True)
        _freqs(torch, st, res["freqs"])
        _gate_cross(st, "cross_spectra_fused", res)
        for name, output in (("csd_fused", "pxy"), ("coherence_fused", "coherence"), ("transfer_function_fused", "h1")):
            res = _forms(torch, st, name, _bind(_single_call(name, output), c), two=True)
            _freqs(torch, st, res["freqs"])
            _gate_cross(st, name, res)
    elif not c["torch_only"]:
        with pytest.raises(ValueError, match="2048"):                     # two operands side by side: documented, and named in the refusal
            bhw.cross_spectra_fused(st["p"], st["x"], st["y"], c["fs"], **C.kwargs(c))
    # csd(x, y) is the conjugate of csd(y, x); csd(x, x) is welch(x) with a +0.0 imaginary part; the sign of Pxy's phase is scipy's
    kw = C.kwargs(c)
    csds = [("csd", dict(fft=one))] + ([("csd_fused", {})] if fused else [])
    for name, extra in csds:
        front = getattr(bhw, name)
        pxy = _np(front(st["p"], st["x"], st["y"], c["fs"], **kw, **extra)[1])
        pyx = _np(front(st["p"], st["y"], st["x"], c["fs"], **kw, **extra)[1])
        pxx = _np(front(st["p"], st["x"], st["x"], c["fs"], **kw, **extra)[1])
        if pxx.imag.any() or np.signbit(pxx.imag).any():
            st["fails"].append(f"{name}(x, x): the imaginary part is not +0.0 in every bin")
        _gate(st, f"{name}(x, x)", "real part against welch", C.rel(pxx.real, ref["pxx"]), C.rel(st["yard"]["cross"]["pxx"], ref["pxx"]))
        if not c["coherent"]:
            continue
        _gate(st, f"conj {name}(y, x)", "pxy", C.rel(np.conj(pyx), ref["pxy"]), C.rel(st["yard"]["cross"]["pxy"], ref["pxy"]))
        if ref["pxy"].shape[-1] > 2:
            inner = slice(1, -1) if c["nfft"] % 2 == 0 else slice(1, None)
            clear = np.abs(ref["pxy"].imag[:, inner]) >= 0.1 * np.abs(ref["pxy"][:, inner])
            for b in range(C.NB):
                k = 1 + int(np.argmax(np.where(clear[b], np.abs(ref["h1"][b, inner]), 0.0)))
                assert clear[b, k - 1], (cid, b, k)
                if np.sign(pxy[b, k].imag) != np.sign(ref["pxy"][b, k].imag):
                    st["fails"].append(f"{name}: the phase of Pxy at signal {b}, bin {k} (the largest |H1|) has the sign opposite to scipy's")
    _done(st)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def test_what_scipy_does_silently_or_is_not_built_is_refused(torch):
    """T < L: scipy shrinks nperseg with a warning, the library documents no such thing and refuses.  noverlap >= length, detrend="linear"
    and average="median" raise."""
    rng = np.random.default_rng(1)
    inputs = {"real": 16, "mixed": 18, "iq": 16, "iq_mixed": 18}
    for family, n in inputs.items():
        p = _params(0)
        xh = rng.standard_normal((2, 4 * n)) + (1j * rng.standard_normal((2, 4 * n)) if family.startswith("iq") else 0.0)
        x = torch.from_numpy(xh.astype(np.complex64 if family.startswith("iq") else np.float32)).cuda()
        with bhw.ResidentTable(p) as tab:
            for obj in (bhw, tab):
                for name in C.FRONTS[family]:
                    front = getattr(obj, name)
                    two = name.split("_")[0] in ("cross", "csd", "coherence", "transfer")
                    call = (lambda t, **kw: front(p, t, t, **kw)) if two else (lambda t, **kw: front(p, t, **kw))
                    call(x, length=n)                                     # the call itself is sound
                    with pytest.raises(ValueError, match="zero segments"):
                        call(x[:, :n - 1], length=n)
                    with pytest.raises(ValueError, match="zero segments"):
                        call(x[0, :n - 1], length=n)
                    for nov in (n, n + 1):
                        with pytest.raises(ValueError, match="noverlap"):
                            call(x, length=n, noverlap=nov)
                    with pytest.raises(ValueError, match="detrend"):
                        call(x, length=n, detrend="linear")
                    if name == "welch":
                        with pytest.raises(ValueError, match="average"):
                            call(x, length=n, average="median")
