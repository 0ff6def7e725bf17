"""Every float and fused FFT front from a resident table of every packed format (GPU).  The cases, their coverage rules and the window
lengths that reach listed entries of the nibble + escapes table are tests/table_source_cases.py's (proved on the CPU by
test_table_source_cases.py); the tables are built once per module.  Each case asserts

  1. that describe_*(..., table=handle) names k_<front>_table<FMT,NT,MODE> with the triple the case expects and the table's own describe
     names the expected format: the instance ran;
  2. that the from-table result equals the library form of the same call word for word (integer views: NaN and -0 count).  The library
     form runs the direct CORDIC chains and shares no table code.  A failure names the front, the configuration, the first differing
     output index and the first window index at which the table's float window differs from the library's.

Per table, once per (weight set, L) and not per front, the float window the table yields -- read as stft_frames of an all-ones signal at
center=False -- equals fl32(w) * 2^-shift with w from the CPU bit model (len_bit_model.py over the oracle's CORDIC), independently of
both kernels.  Once per fused family the library-form result of the nibble table's case meets the family's float64 gate, so two equal
wrong answers cannot pass: the forward spectra fft_sweep_rows.row_error <= cap (and twice torch.fft's error on the same rows), the
inverses signal_error <= cap, and the Welch, hold and cross-spectra calls the exact contracts that tie them to those spectra (welch_psd /
welch_csd up to 16 frames, amax / amin of the power rows), with the gated spectrum of the same arguments beside them."""
import re

import numpy as np
import pytest

import blackman_harris_win_amd as bhw
from blackman_harris_win_amd import binding as B

import fft_sweep_rows as R
import len_bit_model as LB
import table_source_cases as C

pytestmark = pytest.mark.gpu

SCALE = 1e-3
CSD_OUTPUTS = ("pxy", "pxx", "pyy", "coherence", "h1")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def tables(torch):
    """{name: ResidentTable}, each built once under its format limit."""
    built = {}
    for name, (model, pw, w, limit, _) in C.TABLES.items():
        built[name] = bhw.ResidentTable(B.make_params(B.WIN_BH7, pw, w, model=C.MODELS[model]), table_format=C.LIMITS[limit])
    yield built
    for t in built.values():
        t.close()


# ---- geometry, inputs and calls ------------------------------------------------------------------------------------------------------

def _iq(front):
    return front["family"] in ("cfft", "cmfft")


def _geometry(c, front):
    """(nb, T, pad, col0) of the forward call of case c: T such that the call forms c["frames"] frames and two samples are left over."""
    n, L, hop, F = c["n_fft"], c["L"], c["hop"], c["frames"]
    nb = 1 if c["whole"] else C.NB
    if c["detrend"] or front["kind"] == "welch_frames":
        return nb, (F - 1) * hop + L + 2, 0, 0
    pad = n // 2 if c["center"] else 0
    return nb, (F - 1) * hop + n - 2 * pad + 2, pad, (n - L) // 2


def _forward_desc(c, front, p):
    nb, T, pad, col0 = _geometry(c, front)
    return B.make_stft(nb, T, c["frames"], c["hop"], c["n_fft"], col0=col0, pad=pad, pad_mode=B.PAD_REFLECT if pad else 0,
                       channels=2 if _iq(front) else 1, shift=p.dat_width - 1)


def _inverse_desc(c, front, p):
    n, L, hop, F = c["n_fft"], c["L"], c["hop"], c["frames"]
    pad = n // 2 if c["center"] else 0
    nb = 1 if c["whole"] else C.NB
    return B.make_stft(nb, n + hop * (F - 1) - 2 * pad, F, hop, n, col0=(n - L) // 2, pad=pad, channels=2 if _iq(front) else 1,
                       shift=p.dat_width - 1)


def _randn(torch, c, shape, dtype=None, salt=0):
    g = torch.Generator(device="cuda").manual_seed(c["seed"] * 7 + salt)
    if dtype == "int32":
        return torch.randint(-2 ** 31, 2 ** 31, shape, dtype=torch.int64, device="cuda", generator=g).int()
    x = torch.randn(shape, dtype=torch.float32, device="cuda", generator=g) * 1000.0
    if dtype == "complex":
        return torch.complex(x, torch.randn(shape, dtype=torch.float32, device="cuda", generator=g) * 1000.0)
    return x


_banks = {}


def _bank(n_fft):
    if n_fft not in _banks:
        _banks[n_fft] = bhw.FilterBank(bhw.mel_weights(n_fft, 12, 16000.0), device="cuda")
    return _banks[n_fft]


def _inputs(torch, c, front, p):
    """The tensors of case c, made once and handed to both forms."""
    kind, n, L, hop, F = front["kind"], c["n_fft"], c["L"], c["hop"], c["frames"]
    nb = 1 if c["whole"] else C.NB
    if kind == "frames_f32":
        return (_randn(torch, c, ((F - 1) * hop + L,)),)
    if kind == "ola_f32":
        return (_randn(torch, c, (F, L)),)
    if kind == "frames_len":
        return (_randn(torch, c, ((F - 1) * hop + L,), "int32"),)
    if kind == "ola_len":
        return (_randn(torch, c, (F, L), "int32"),)
    if kind in ("generate_len", "window_sums"):
        return ()
    if kind == "istft_ola":
        return (_randn(torch, c, (nb, F, n)),)
    if kind == "inverse":
        Y = _randn(torch, c, (nb, F, n if _iq(front) else n // 2 + 1), "complex") * 0.1
        if not _iq(front):
            Y[..., 0] = Y[..., 0].real
            Y[..., -1] = Y[..., -1].real
        return (Y,)
    T = _geometry(c, front)[1]
    x = _randn(torch, c, (nb, T), "complex" if _iq(front) else None)
    if kind == "csd":
        return (x, 0.7 * x + _randn(torch, c, (nb, T), salt=1))
    return (x,)


def _call(obj, c, front, p, inputs):
    """The front of case c on obj (the module: the library form; a ResidentTable: the table form): a list of tensors, or a dict of
    numbers for window_sums."""
    kind, n, L, hop, kw = front["kind"], c["n_fft"], c["L"], c["hop"], front["kw"]
    length = None if kw.get("pow2") else L
    if kind == "frames_f32":
        return [obj.apply_frames(p, inputs[0], hop, length=length)]
    if kind == "ola_f32":
        return [obj.overlap_add(p, inputs[0], hop, length=length, normalize=bool(kw.get("normalize")))]
    if kind == "frames_len":
        return [obj.apply_frames(p, inputs[0], hop, shift=p.dat_width - 1, length=L)]
    if kind == "ola_len":
        return [obj.overlap_add(p, inputs[0], hop, shift=p.dat_width - 1, length=L)]
    if kind == "generate_len":
        return [obj.generate(p, 5, 2 * L + 300, length=L)]
    if kind == "window_sums":
        return obj.window_sums(p, L, f32=bool(c["seed"] % 2))
    if kind == "stft_frames":
        return [obj.stft_frames(p, inputs[0], n, hop, win_length=L, center=c["center"])]
    if kind == "istft_ola":
        return [obj.istft_overlap_add(p, inputs[0], n, hop, win_length=L, center=c["center"], normalize=bool(c["seed"] % 2))]
    if kind == "welch_frames":
        return [obj.welch_frames(p, inputs[0], L, hop, nfft=n, detrend="constant")]     # (without detrending: stft_frames' kernel)
    name = front["name"]
    if kind == "forward":
        if kw.get("bank"):
            return [obj.spectrogram(p, inputs[0], n, hop, win_length=L, center=c["center"], detrend=c["detrend"], fbank=_bank(n))]
        return [getattr(obj, name)(p, inputs[0], n, hop, win_length=L, center=c["center"], detrend=c["detrend"])]
    if kind == "inverse":
        return [getattr(obj, name)(p, inputs[0], n, hop, win_length=L, center=True, normalize=bool(c["seed"] % 2))]
    if kind == "welch":
        return [getattr(obj, name)(p, inputs[0], n, hop, SCALE, win_length=L, center=False, detrend=c["detrend"])]
    if kind == "hold":
        return list(getattr(obj, name)(p, inputs[0], n, hop, SCALE, win_length=L, center=False, detrend=c["detrend"]))
    if kind == "csd":
        r = obj.csd_fft(p, inputs[0], inputs[1], n, hop, SCALE, outputs=CSD_OUTPUTS, win_length=L, center=False, detrend=c["detrend"])
        return [r[k] for k in CSD_OUTPUTS]
    raise ValueError(kind)


def _describe(c, front, p, handle):
    """The describe line of the table form of case c."""
    kind, n, L, hop, F, kw = front["kind"], c["n_fft"], c["L"], c["hop"], c["frames"], front["kw"]
    if kind == "frames_f32":
        return B.describe_f32(p, None if kw.get("pow2") else L, frames=B.make_frames(F, hop, shift=p.dat_width - 1), table=handle)
    if kind == "ola_f32":
        return B.describe_f32(p, None if kw.get("pow2") else L, ola=B.make_ola(F, hop, (F - 1) * hop + L, shift=p.dat_width - 1),
                              normalize=bool(kw.get("normalize")), table=handle)
    if kind == "frames_len":
        return B.describe_len(p, L, frames=B.make_frames(F, hop, shift=p.dat_width - 1), table=handle)
    if kind == "ola_len":
        return B.describe_len(p, L, ola=B.make_ola(F, hop, (F - 1) * hop + L, shift=p.dat_width - 1), table=handle)
    if kind == "generate_len":
        return B.describe_len(p, L, n0=5, count=2 * L + 300, table=handle)
    if kind == "window_sums":
        return B.describe_welch(p, L, sums_f32=bool(c["seed"] % 2), table=handle)
    if kind == "stft_frames":
        return B.describe_stft(p, L, _forward_desc(c, front, p), table=handle)
    if kind == "istft_ola":
        return B.describe_stft(p, L, _inverse_desc(c, front, p), inverse=True, normalize=bool(c["seed"] % 2), table=handle)
    if kind == "welch_frames":
        return B.describe_welch(p, L, stft=_forward_desc(c, front, p), detrend=True, table=handle)
    fam = {"fft": "fft", "mfft": "mfft", "cfft": "cfft", "cmfft": "cmfft", "csd": "fft"}[front["family"]]
    power = front["name"].startswith("spectrogram")
    if kind == "forward":
        s = _forward_desc(c, front, p)
        if fam == "fft" and power:
            return B.describe_spectrogram(p, L, s, detrend=c["detrend"], fbank=_bank(n).descriptor if kw.get("bank") else None, table=handle)
        if fam == "fft":
            return B.describe_stft_fft(p, L, s, detrend=c["detrend"], table=handle)
        return getattr(B, f"describe_stft_{fam}")(p, L, s, detrend=c["detrend"], power=power, table=handle)
    if kind == "inverse":
        return getattr(B, f"describe_istft_{fam}")(p, L, _inverse_desc(c, front, p), normalize=bool(c["seed"] % 2), table=handle)
    if kind in ("welch", "hold"):
        return getattr(B, f"describe_{kind}_{fam}")(p, L, _forward_desc(c, front, p), detrend=c["detrend"], table=handle)
    if kind == "csd":
        return B.describe_csd_fft(p, L, _forward_desc(c, front, p), detrend=c["detrend"], outputs=CSD_OUTPUTS, table=handle)
    raise ValueError(kind)


def _words(torch, t):
    """t as int32 words: a complex tensor as its (re, im) pairs."""
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.int32).reshape(-1)


def _float_window(torch, obj, p, L):
    """The float window of obj (the module or a table) as the float fronts see it: stft_frames of ones at center=False, one row."""
    return obj.stft_frames(p, torch.ones(L, dtype=torch.float32, device="cuda"), L, 1, center=False).reshape(-1)


def _first_window_difference(torch, t, p, L):
    a, b = _words(torch, _float_window(torch, t, p, L)), _words(torch, _float_window(torch, bhw, p, L))
    bad = (a != b).nonzero()
    return int(bad[0]) if bad.numel() else None


# ---- 1 and 2: the instance, and the library form word for word ---------------------------------------------------------------------------

@pytest.mark.parametrize("cid", C.case_ids())
def test_from_table_equals_library(torch, tables, cid):
    c = C.case(cid)
    front, t = C.FRONT[c["front"]], tables[c["table"]]
    p = C.params(c["table"], c["weights"])
    fmt, nt, mode = c["triple"]
    what = f"{c['front']} on table {c['table']} {C.TABLES[c['table']]} with {c['weights']}, n_fft {c['n_fft']} L {c['L']} hop {c['hop']}"
    own = t.describe(p, 0, 1 << p.phi_width)
    assert own.startswith("resident table[%s," % C.FMT_NAME[fmt]), (what, own)
    line = _describe(c, front, p, t.handle)
    m = re.search(re.escape(front["kernel"]) + r"(?:_len)?<(\d+),(\d+),(\d+)>", line)
    assert m and tuple(int(v) for v in m.groups()) == (fmt, nt, mode), (what, (fmt, nt, mode), line)
    inputs = _inputs(torch, c, front, p)
    want = _call(bhw, c, front, p, inputs)
    got = _call(t, c, front, p, inputs)
    if isinstance(want, dict):
        assert got == want, (what, got, want)
        return
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None) and g.shape == w.shape and g.dtype == w.dtype, (what, i)
        gw, ww = _words(torch, g), _words(torch, w)
        if not torch.equal(gw, ww):
            bad = int((gw != ww).nonzero()[0])
            floats = 2 if g.is_complex() else 1
            index = tuple(int(v) for v in np.unravel_index(bad // floats, tuple(g.shape)))
            pytest.fail(f"{what}: output {i} differs from the library form first at index {index} (word {bad} of {gw.numel()}, "
                        f"{int((gw != ww).sum())} words differ): table {int(gw[bad]):#x}, library {int(ww[bad]):#x}; the table's float window "
                        f"first differs from the library's at window index {_first_window_difference(torch, t, p, c['L'])}")


# ---- 3: the float window of every table against the CPU bit model ------------------------------------------------------------------------

@pytest.mark.parametrize("table", list(C.TABLES))
def test_float_window_is_the_bit_model(torch, tables, table):
    t = tables[table]
    pairs = C.window_pairs(table)
    assert pairs
    for weights, L in pairs:
        p = C.params(table, weights)
        want = LB.float_window(p, L)
        got = _float_window(torch, t, p, L).cpu().numpy()
        same = got.view(np.uint32) == want.view(np.uint32)
        assert same.all(), (f"table {table} {C.TABLES[table]} with {weights}, L {L}: the float window differs from fl32(w) * 2^-shift first at "
                            f"window index {int(np.argmin(same))} ({int((~same).sum())} of {L} differ): table {got[np.argmin(same)]!r}, "
                            f"bit model {want[np.argmin(same)]!r}")


# ---- 4: the library form against float64, once per fused family ---------------------------------------------------------------------------

def _gate_setup(torch, fam):
    c = C.case(C.gate_cases()[fam])
    front = C.FRONT[c["front"]]
    assert c["table"] == "nibble" and not c["detrend"] and c["frames"] <= 16
    p = C.params(c["table"], c["weights"])
    return c, front, p, LB.float_window(p, c["L"])


def _forward_spectrum(torch, c, front, p, v, center):
    """The library-form spectrum of case c's arguments (stft, stft_mixed, stft_iq or stft_iq_mixed by the family), held to the float64
    gate of the forward sweep: returns (x, Y)."""
    iq, n, L, hop = _iq(front), c["n_fft"], c["L"], c["hop"]
    stft = {"fft": bhw.stft, "csd": bhw.stft, "mfft": bhw.stft_mixed, "cfft": bhw.stft_iq, "cmfft": bhw.stft_iq_mixed}[front["family"]]
    nb, T, pad, col0 = _geometry(dict(c, center=center), front)
    x = _randn(torch, c, (nb, T), "complex" if iq else None)
    Y = stft(p, x, n, hop, win_length=L, center=center)
    assert Y.shape[-2] == c["frames"]
    g, xh = dict(n_fft=n, hop=hop, col0=col0, pad=pad, frames=c["frames"]), x.cpu().numpy()
    if iq:
        # one coefficient for both parts of a sample: two real products (a complex product would add signed zeros of its own)
        rows = np.empty((nb, c["frames"], n), dtype=np.complex64)
        rows.real, rows.imag = R.frames(np.ascontiguousarray(xh.real), v, g), R.frames(np.ascontiguousarray(xh.imag), v, g)
    else:
        rows = R.frames(xh, v, g)
    parent = bhw.stft_frames(p, x, n, hop, win_length=L, center=center)
    assert np.array_equal(np.ascontiguousarray(parent.cpu().numpy()).view(np.uint32), np.ascontiguousarray(rows).view(np.uint32)), \
        "the library's rows are the restated rows of the CPU bit model's window"
    ref = (np.fft.fft if iq else np.fft.rfft)(rows.astype(np.complex128 if iq else np.float64), axis=-1)
    yard = (torch.fft.fft if iq else torch.fft.rfft)(parent, dim=-1).cpu().numpy()
    err, yerr = R.row_error(Y.cpu().numpy(), ref), R.row_error(yard, ref)
    print(f"{front['fused']} n_fft {n} L {L}: forward spectrum error {err:.3e}, torch.fft {yerr:.3e}, cap {R.cap(n):.3e}")
    assert err <= R.gate(n, 0) and err <= 2.0 * yerr, (front["fused"], err, yerr, R.cap(n))
    return x, Y


@pytest.mark.parametrize("fam", [f for f in C.FUSED_FAMILIES if f.startswith("forward")])
def test_library_forward_meets_the_float64_gate(torch, fam):
    c, front, p, v = _gate_setup(torch, fam)
    _forward_spectrum(torch, c, front, p, v, c["center"])


@pytest.mark.parametrize("fam", [f for f in C.FUSED_FAMILIES if f.startswith("inverse")])
def test_library_inverse_meets_the_float64_gate(torch, fam):
    c, front, p, v = _gate_setup(torch, fam)
    iq, n, L, hop, F = _iq(front), c["n_fft"], c["L"], c["hop"], c["frames"]
    (Y,) = _inputs(torch, c, front, p)
    normalize = bool(c["seed"] % 2)
    got = getattr(bhw, front["name"])(p, Y, n, hop, win_length=L, center=True, normalize=normalize).cpu().numpy()
    Yh = Y.cpu().numpy().astype(np.complex128)
    rows = np.fft.ifft(Yh, n=n, axis=-1) if iq else np.fft.irfft(Yh, n=n, axis=-1)
    pad, col0 = n // 2, (n - L) // 2
    g = dict(hop=hop, col0=col0, t0=pad - col0, T=n + hop * (F - 1) - 2 * pad, normalize=normalize)
    ref = R.overlap_add64(rows, v, g)
    err = max(R.signal_error(got[b], ref[b]) for b in range(got.shape[0]))
    print(f"{fam} n_fft {n} L {L}: error {err:.3e}, cap {R.cap(n):.3e}")
    assert err <= R.cap(n), (fam, err, R.cap(n))


@pytest.mark.parametrize("fam", [f for f in C.FUSED_FAMILIES if f.split("-")[0] in ("welch", "hold", "csd")])
def test_library_welch_hold_and_csd_are_tied_to_a_gated_spectrum(torch, fam):
    c, front, p, v = _gate_setup(torch, fam)
    iq, n, L, hop = _iq(front), c["n_fft"], c["L"], c["hop"]
    x, Y = _forward_spectrum(torch, c, front, p, v, False)
    kw = dict(win_length=L, center=False)
    if front["kind"] == "welch":
        P = getattr(bhw, front["name"])(p, x, n, hop, SCALE, **kw)
        want = bhw.welch_psd(Y, SCALE, nfft=n, onesided=not iq)
        assert torch.equal(_words(torch, P), _words(torch, want)), fam
    elif front["kind"] == "hold":
        S = Y.real.double() ** 2 + Y.imag.double() ** 2                  # both squares exact in binary64, one rounding, one rounding
        S = S.float()
        sk = torch.full((S.shape[-1],), SCALE, dtype=torch.float64, device="cuda")
        if not iq:
            sk[1:-1] *= 2.0
        pmax, pmin = getattr(bhw, front["name"])(p, x, n, hop, SCALE, **kw)
        assert torch.equal(_words(torch, pmax), _words(torch, (S.amax(-2).double() * sk).float())), fam
        assert torch.equal(_words(torch, pmin), _words(torch, (S.amin(-2).double() * sk).float())), fam
    else:
        y = 0.7 * x + _randn(torch, c, tuple(x.shape), salt=1)
        Yy = bhw.stft(p, y, n, hop, **kw)
        got = bhw.csd_fft(p, x, y, n, hop, SCALE, outputs=CSD_OUTPUTS, **kw)
        want = bhw.welch_csd(Y, Yy, SCALE, nfft=n, outputs=CSD_OUTPUTS)
        for k in CSD_OUTPUTS:
            assert torch.equal(_words(torch, got[k]), _words(torch, want[k])), (fam, k)
