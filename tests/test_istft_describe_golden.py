"""Every word of the describe lines and of the refusals of the four fused inverse fronts -- bhw_istft_{fft,mfft,cfft,cmfft}_f32_* --
held to tests/golden/istft_describe.json, which was recorded through binding.py by this file's collect() at commit b1159b7 ("Test
every float and fused FFT front from tables of every packed format"), the parent of the change that gave these calls one span plan,
one descriptor check, one io check and one describe formatter.  No GPU: the describe calls are host arithmetic, and a refused call
stops before any HIP call (the addresses below are never dereferenced; a call that passes every check is asked through its
from-table form without a table and stops at "table is NULL").

Describe lines, direct route, per family at an n_fft with 16 or more rows side by side and at one with fewer (32 and 512; 20 and
400 for the mixed-radix families; 2025, odd, for cmfft as well): samples 0; one frame; a signal of one span; several spans per
signal with a halo, set by the halo (batch 3 x 200 frames) and by the grid target (batch 64 x 4096 frames); hop > L, a gap; a hop
clamped by t0 + samples; hop 1 with L = n_fft and batch 1, where the halo sets S, under 256 groups run and the "heavy overlap" tail
is printed; non-zero col0 and pad with L < n_fft; and, at samples 0 and at the halo-set spans, BHW_OLA_NORMALIZE and (I/Q)
BHW_CFFT_SHIFT alone and together.  The table route's line needs a table handle: tests/test_gpu_table_source.py holds it.

Refusals: each refusal of each call once, by return code and bhw_last_error() text.  A foreign flag bit answers at different steps
in the two pairs -- the real pair before the descriptor is read, the I/Q pair after the overlap-add's descriptor checks -- which the
"foreign flag, hop 0" case pins.

Misspelling "spans of S" in the shared describe formatter makes this test fail first at "cfft n_fft=32 col0 pad" (the fixture's
keys are sorted) with 91 of the 119 lines wrong, and misspelling "aligned" in the shared io check's "d_Y is not 8-byte aligned" at
"cfft d_Y misaligned": in each case all four families fail."""
import ctypes
import json
import os

from blackman_harris_win_amd import binding as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "istft_describe.json")
SIZES = {"fft": (32, 512), "mfft": (20, 400), "cfft": (32, 512), "cmfft": (20, 400, 2025)}
IQ = ("cfft", "cmfft")
Y, X = 0x10000000, 0x80000000


def _stft(fam, n_fft, batch, frames, hop, samples, **kw):
    return B.make_stft(batch, samples, frames, hop, n_fft, channels=2 if fam in IQ else 1, shift=31, **kw)


def _describe_cases(fam, n):
    """name -> (L, descriptor)"""
    q, h = max(n // 4, 1), n // 2
    return {
        "samples 0": (n, _stft(fam, n, 1, 0, q, 0)),
        "one frame": (n, _stft(fam, n, 1, 1, q, n)),
        "one span": (n, _stft(fam, n, 1, 4, q, 4 * q)),
        "halo spans": (n, _stft(fam, n, 3, 200, q, 199 * q + n)),
        "grid spans": (n, _stft(fam, n, 64, 4096, q, 4095 * q + n)),
        "gap": (h, _stft(fam, n, 2, 5, n, 4 * n + h)),
        "hop clamped": (n, _stft(fam, n, 1, 1, 10 * n, h)),
        "heavy overlap": (n, _stft(fam, n, 1, 1 << 18, 1, (1 << 18) - 1 + n)),
        "col0 pad": (h, _stft(fam, n, 2, 50, max(h // 4, 1), 49 * max(h // 4, 1) + h, col0=n // 4, pad=h)),
    }


def _describe_lines(params):
    out = {}
    for fam, sizes in SIZES.items():
        fn = getattr(B, f"describe_istft_{fam}")
        toggles = [dict(normalize=True)]
        if fam in IQ:
            toggles += [dict(fftshift=True), dict(normalize=True, fftshift=True)]
        for n in sizes:
            for name, (length, s) in _describe_cases(fam, n).items():
                for kw in [{}] + (toggles if name in ("samples 0", "halo spans") else []):
                    key = f"{fam} n_fft={n} {name}" + "".join(f" {k}" for k in sorted(kw))
                    out[key] = fn(params, length, s, **kw)
    return out


def _call(params, fam, length, s, *, flags=1, y=Y, x=X):
    """The from-table call without a table: (return code, bhw_last_error())."""
    fn = getattr(B.lib(), f"bhw_istft_{fam}_f32_from_table")
    rc = fn(None, ctypes.byref(params), int(length), None, ctypes.byref(s) if s is not None else None, flags, ctypes.c_void_p(y),
            ctypes.c_void_p(x))
    return [rc, B.lib().bhw_last_error().decode()]


def _refusals(params):
    out = {}
    for fam, sizes in SIZES.items():
        n, iq = sizes[1], fam in IQ
        hop, frames, batch = n // 4, 40, 3
        row = 2 * n if iq else n + 2                                         # floats of a spectrum row
        ysig = (frames - 1) * row + row

        def mk(n_fft=n, **kw):
            s = _stft(fam, n_fft, batch, frames, hop, (frames - 1) * hop + n_fft)
            for k, v in kw.items():
                setattr(s, k, v)
            return s

        s = mk()
        cases = {
            "passes": (n, s, {}),
            "samples 0 passes": (n, mk(samples=0, frames=0), dict(y=0, x=0)),
            "descriptor NULL": (n, None, {}),
            "struct_size": (n, mk(struct_size=4), {}),
            "hop 0": (n, mk(hop=0), {}),
            "foreign flag": (n, s, dict(flags=8 | 1)),
            "foreign flag, hop 0": (n, mk(hop=0), dict(flags=8 | 1)),
            "channels": (n, mk(channels=1 if iq else 2), {}),
            "n_fft 16384": (16, mk(1 << 14), {}),
            "n_fft 48": (16, mk(48), {}),
            "n_fft 512": (16, mk(512), {}),
            "n_fft 42": (14, mk(42), {}),
            "n_fft 45": (15, mk(45), {}),
            "n_fft 6000": (16, mk(6000), {}),
            "y_stride small": (n, mk(y_stride=row - 2), {}),
            "y_stride odd": (n, mk(y_stride=row + 1), {}),
            "y_batch_stride small": (n, mk(y_batch_stride=ysig - 2), {}),
            "y_batch_stride odd": (n, mk(y_batch_stride=ysig + 1), {}),
            "Y row extent": (n, mk(y_stride=1 << 60), {}),
            "Y NULL": (n, s, dict(y=0)),
            "x NULL": (n, s, dict(x=0)),
            "d_Y misaligned": (n, s, dict(y=Y + 4)),
            "d_x misaligned": (n, s, dict(x=X + 2)),
            "x extent": (n, mk(x_stride=1 << 59), {}),
            "Y extent": (n, mk(y_batch_stride=1 << 59), {}),
            "wraps": (n, s, dict(x=(1 << 64) - 4096)),
            "overlap": (n, s, dict(x=Y + 8)),
        }
        for name, (length, desc, kw) in cases.items():
            out[f"{fam} {name}"] = _call(params, fam, length, desc, **kw)
    return out


def collect():
    params = B.make_params(B.WIN_BH4, 24, 32)
    return {"describe": _describe_lines(params), "refusals": _refusals(params)}


def test_describe_lines_and_refusals_are_the_recorded_ones():
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    got = collect()
    for part in ("describe", "refusals"):
        assert got[part].keys() == golden[part].keys()
        for key, want in golden[part].items():
            assert got[part][key] == want, key


def test_the_recorded_cases_are_the_ones_named():
    """The fixture holds what the case names promise: the heavy-overlap tail, a non-zero share of repeats, every family's passing
    call and no refusal met twice under different names within a family."""
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    for key, line in golden["describe"].items():
        assert ("heavy overlap: the halo sets S" in line) == key.endswith("heavy overlap"), key
        if " halo spans" in key or " grid spans" in key:
            assert " 1 spans per signal" not in line and ", 0% of the transforms repeated" not in line, key
        assert ("nothing (samples 0)" in line) == (" samples 0" in key), key
    for fam in SIZES:
        assert golden["refusals"][f"{fam} passes"][1] == "table is NULL"
        assert golden["refusals"][f"{fam} samples 0 passes"][1] == "table is NULL"
        refused = [tuple(v) for k, v in golden["refusals"].items() if k.startswith(fam + " ") and " passes" not in k]
        assert all(rc != 0 for rc, _ in refused)
