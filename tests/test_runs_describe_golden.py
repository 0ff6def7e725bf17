"""Every word of the describe lines and of the output-side refusals of the fused calls whose kernels own runs -- bhw_welch_{fft,
mfft,cfft,cmfft}_f32_* and bhw_hold_{fft,mfft,cfft,cmfft}_f32_* -- held to tests/golden/runs_describe.json, which was recorded
through binding.py at commit 849aa5e ("Hold every SciPy-shaped spectral front to SciPy, bin by bin"), the parent of the change that
gave these calls one run plan, one output-side check and one describe tail.  No GPU: the describe calls are host arithmetic, and a
refused call stops before any HIP call (the addresses below are never dereferenced; a call that passes every check is asked through
its from-table form without a table and stops at "table is NULL").

Describe lines, direct route: frames 0, 1, 16, 17 and 257 (nothing; one chunk; two chunks; two blocks) x batch 1 and 3 x an n_fft
with 16 or more rows side by side and one with fewer (32 and 512; 20 and 400 for the mixed-radix families), and at (frames 0,
batch 1) and (frames 257, batch 3) each of detrending, BHW_CFFT_SHIFT (I/Q) and a single trace (hold) alone and all together.
Refusals: each output-side refusal of each call once, by code and message.  The 2^34 case records what a caller sees: the input
side's bound on batch * frames * n_fft answers before the output side's on the chunk sums, which no descriptor reaches alone.
Changing one word of the shared describe tail ("chunks" in describe_runs_tail) makes this test fail at its first line with frames."""
import ctypes
import json
import os

from blackman_harris_win_amd import binding as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "runs_describe.json")
SIZES = {"fft": (32, 512), "mfft": (20, 400), "cfft": (32, 512), "cmfft": (20, 400)}
IQ = ("cfft", "cmfft")
HOP = 7
X, P, P2, W = 0x10000000, 0x80000000, 0x90000000, 0x40000000


def _stft(fam, n_fft, frames, batch, **kw):
    samples = (max(frames, 1) - 1) * HOP + n_fft
    return B.make_stft(batch, samples, frames, HOP, n_fft, channels=2 if fam in IQ else 1, shift=31, **kw)


def _describe_lines(params):
    out = {}
    for kind in ("welch", "hold"):
        for fam, sizes in SIZES.items():
            fn = getattr(B, f"describe_{kind}_{fam}")
            toggles = [dict(detrend=True)]
            if fam in IQ:
                toggles.append(dict(fftshift=True))
            if kind == "hold":
                toggles.append(dict(traces="max"))
            if len(toggles) > 1:
                toggles.append({k: v for t in toggles for k, v in t.items()})
            for n_fft in sizes:
                cases = [(frames, batch, {}) for frames in (0, 1, 16, 17, 257) for batch in (1, 3)]
                cases += [(frames, batch, t) for frames, batch in ((0, 1), (257, 3)) for t in toggles]
                for frames, batch, kw in cases:
                    key = f"{kind}_{fam} n_fft={n_fft} frames={frames} batch={batch}" + "".join(f" {k}={v}" for k, v in sorted(kw.items()))
                    out[key] = fn(params, n_fft, _stft(fam, n_fft, frames, batch), **kw)
    return out


def _call(params, kind, fam, s, *, flags=1, scale=1.0, psd=1, x=X, p=P, p2=P2, p_stride=0, ws=W, ws_bytes=None):
    """The from-table call without a table: (return code, bhw_last_error())."""
    fn = getattr(B.lib(), f"bhw_{kind}_{fam}_f32_from_table")
    if ws_bytes is None:
        ws_bytes = getattr(B, f"{kind}_{fam}_workspace_bytes")(s)
    args = [None, ctypes.byref(params), int(s.n_fft), None, ctypes.byref(s), flags, scale]
    if fam not in IQ:
        args.append(psd)
    args += [ctypes.c_void_p(x), ctypes.c_void_p(p)]
    if kind == "hold":
        args.append(ctypes.c_void_p(p2))
    args += [p_stride, ctypes.c_void_p(ws), ws_bytes]
    rc = fn(*args)
    return [rc, B.lib().bhw_last_error().decode()]


def _refusals(params):
    out = {}
    for kind in ("welch", "hold"):
        for fam, sizes in SIZES.items():
            n = sizes[1]
            bins = n if fam in IQ else n // 2 + 1
            mk = lambda **kw: _stft(fam, n, kw.pop("frames", 40), kw.pop("batch", 3), **kw)         # noqa: E731
            s = mk()
            xbytes = 4 * (2 if fam in IQ else 1) * (2 * s.samples + s.samples)                    # three packed signals
            need = getattr(B, f"{kind}_{fam}_workspace_bytes")(s)
            cases = {
                "passes": (s, {}),
                "y_stride": (mk(y_stride=3), {}),
                "y_batch_stride": (mk(y_batch_stride=7), {}),
                "power flag": (s, dict(flags=2 | 1)),
                "scale nan": (s, dict(scale=float("nan"))),
                "scale inf": (s, dict(scale=float("inf"))),
                "p_stride": (s, dict(p_stride=bins - 1)),
                "2^34": (mk(batch=1 << 20, frames=2048), {}),
                "x NULL": (s, dict(x=0)),
                "P NULL": (s, dict(p=0, p2=0)),
                "P misaligned": (s, dict(p=P + 2)),
                "x misaligned": (s, dict(x=X + 1)),
                "workspace NULL": (s, dict(ws=0)),
                "workspace misaligned": (s, dict(ws=W + 4)),
                "workspace short": (s, dict(ws_bytes=need - 1)),
                "extent": (mk(x_stride=1 << 59), {}),
                "wraps": (s, dict(x=(1 << 64) - 4096)),
                "x P overlap": (s, dict(p=X + xbytes - 4)),
                "workspace x overlap": (s, dict(ws=X + 8)),
                "workspace P overlap": (s, dict(ws=P - need + 8)),
            }
            if fam not in IQ:
                cases["psd_flags"] = (s, dict(psd=2))
            if kind == "hold":
                cases["P2 misaligned"] = (s, dict(p2=P2 + 2))
                cases["x P2 overlap"] = (s, dict(p2=X + xbytes - 4))
                cases["P P2 overlap"] = (s, dict(p2=P + 4 * bins))
                cases["workspace P2 overlap"] = (s, dict(ws=P2 - need + 8))
                cases["one trace passes"] = (s, dict(p=0))
            for name, (desc, kw) in cases.items():
                out[f"{kind}_{fam} {name}"] = _call(params, kind, fam, desc, **kw)
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
