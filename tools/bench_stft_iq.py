#!/usr/bin/env python3
"""The fused window + complex FFT kernel for I/Q input (bhw_stft_cfft_f32_* / bhw.stft_iq / bhw.spectrogram_iq) on one GPU, one
process.  Prints one JSON record and writes it to --out (profiles/r17_stft_iq.json by default).

Legs: the shapes of section 18's T1 and N64, complex64
  T1c batch   BH-4, P 24, 32 b; B 64, T 160 000 complex, L 400 in rows of 512, hop 160 (998 segments per signal), detrended
  N64c short  BH-4, P 24, 32 b; B 64, T 160 000 complex, L = nfft 64, hop 32 (4 999 segments per signal), detrended
Variants: the fused call from a table and in library form; the two-step route of the same process, welch_frames + torch.fft.fft,
together and each alone; the power form; a plain copy of the call's bytes (read B * T * 8, write B * F * nfft * 8: one copy_ of half
that many bytes each way).
Accuracy: per leg, the largest relative l2 row error of the fused spectrum and of torch.fft.fft over the same float32 rows, against
numpy.fft.fft in float64 (the figures of tests/test_gpu_stft_iq.py on the benchmarked shapes; 2 000 - 4 000 rows).
Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events, the variants of a leg alternated step
by step, after a clock ramp; times are per call (median, min, max over --steps).

    python tools/bench_stft_iq.py [--steps 10] [--reps 20] [--out FILE] [--quick]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import blackman_harris_win_amd as bhw  # noqa: E402
from blackman_harris_win_amd import binding as B  # noqa: E402


def timed(fns, steps, reps, warm=2):
    for f in fns.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(steps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) / reps)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ts.items()}


def legs():
    return {"T1c": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 400, 512, 160),
            "N64c": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 64, 64, 32)}


def ramp():
    """A second of work in front of the timed region: the clock has ramped when the first leg starts."""
    a = torch.randn((4096, 4096), device="cuda")
    for _ in range(40):
        a = (a @ a).clamp_(-1, 1)
    torch.cuda.synchronize()


def row_errors(Y, rows):
    Y, rows = Y.reshape(-1, Y.shape[-1]), rows.reshape(-1, rows.shape[-1])
    ref = np.fft.fft(rows.astype(np.complex128), axis=-1)
    nr = np.sqrt((np.abs(ref) ** 2).sum(-1))
    ne = np.sqrt((np.abs(Y.astype(np.complex128) - ref) ** 2).sum(-1))
    return float((ne[nr > 0] / nr[nr > 0]).max())


def accuracy_signal(nb, T, seed=3):
    """Complex noise + tones of 1e3 and 1e-3 + an offset: the structure of section 18's signal in both parts."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = torch.arange(T, device="cuda", dtype=torch.float64)
    x = torch.view_as_complex(torch.randn((nb, T, 2), device="cuda", generator=g, dtype=torch.float64)) \
        + 1e3 * torch.exp(2j * np.pi * 0.1234 * n) + 1e-3 * torch.exp(-2j * np.pi * 0.31 * n) + (0.5 - 0.25j)
    return x.to(torch.complex64)


def fused_leg(name, p, nb, T, L, nfft, hop, steps, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((nb, T, 2), device="cuda", generator=g)) + (3.0 - 1.0j)
    F = 1 + (T - L) // hop
    rec = {"leg": name, "B": nb, "T": T, "L": L, "nfft": nfft, "hop": hop, "frames": F}
    with bhw.ResidentTable(p) as t:
        seg = torch.empty((nb, F, nfft), dtype=torch.complex64, device="cuda")
        mean = torch.empty(nb * F * 2, device="cuda")
        Y = torch.empty((nb, F, nfft), dtype=torch.complex64, device="cuda")
        P = torch.empty((nb, F, nfft), device="cuda")
        bytes_in, bytes_out = nb * T * 8, nb * F * nfft * 8
        half = (bytes_in + bytes_out) // 2 // 4
        src, dst = torch.empty(half, device="cuda"), torch.empty(half, device="cuda")
        kw = dict(win_length=L, center=False, detrend=True)
        r = timed({"fused_table": lambda: t.stft_iq(p, x, nfft, hop, out=Y, **kw),
                   "fused_library": lambda: bhw.stft_iq(p, x, nfft, hop, out=Y, **kw),
                   "two_step": lambda: torch.fft.fft(t.welch_frames(p, x, L, hop, nfft=nfft, out=seg, workspace=mean), dim=-1),
                   "welch_frames": lambda: t.welch_frames(p, x, L, hop, nfft=nfft, out=seg, workspace=mean),
                   "fft_alone": lambda: torch.fft.fft(seg, dim=-1),
                   "power_table": lambda: t.spectrogram_iq(p, x, nfft, hop, out=P, **kw),
                   "copy_of_its_bytes": lambda: dst.copy_(src)}, steps, reps)
        rec["plan"] = B.describe_stft_cfft(p, L, B.make_stft(nb, T, F, hop, nfft, channels=2, shift=p.dat_width - 1), detrend=True, table=t.handle)
        m = {k: v["median_ms"] for k, v in r.items()}
        rec.update({"times": r, "bytes_in": bytes_in, "bytes_out": bytes_out,
                    "fused_over_two_step": m["fused_table"] / m["two_step"], "fused_below_two_step": m["fused_table"] < m["two_step"],
                    "library_over_table": m["fused_library"] / m["fused_table"],
                    "power_over_fused": m["power_table"] / m["fused_table"],
                    "fused_over_copy": m["fused_table"] / m["copy_of_its_bytes"],
                    "fused_GBps": (bytes_in + bytes_out) / m["fused_table"] / 1e6,
                    "fused_GFLOPs": 5.0 * nfft * np.log2(nfft) * nb * F / m["fused_table"] / 1e6})
        # accuracy on the leg's shape: 2 signals, at most 2000 rows each
        xa = accuracy_signal(min(nb, 2), min(T, L + 1999 * hop))
        rows = t.welch_frames(p, xa, L, hop, nfft=nfft)
        e_fused = row_errors(t.stft_iq(p, xa, nfft, hop, **kw).cpu().numpy(), rows.cpu().numpy())
        e_rocfft = row_errors(torch.fft.fft(rows, dim=-1).cpu().numpy(), rows.cpu().numpy())
        rec["accuracy"] = {"rows": int(rows.shape[0] * rows.shape[1]), "fused_rel_l2": e_fused, "rocfft_rel_l2": e_rocfft, "ratio": e_fused / e_rocfft,
                           "bound": 2.0, "cap": 2.0 ** -24 * float(np.log2(nfft)), "met": e_fused <= 2.0 * e_rocfft}
    return rec


def resources():
    path = os.path.join(ROOT, "blackman_harris_win_amd", "kernel_resources.json")
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        res = json.load(f)
    out = {}
    for k, v in res.items():
        if k.startswith("k_stft_cfft"):
            key = json.dumps({n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "SGPRs Spill", "ScratchSize", "Occupancy", "LDS Size")}, sort_keys=True)
            out.setdefault(key, []).append(k)
    return [{"figures": json.loads(k), "instances": len(v), "example": v[0],
             "note": "LDS Size is the static part (the direct form's ROM); the row buffers and twiddles are dynamic: the plan line's bytes"}
            for k, v in out.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_stft_iq.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written (a profiler run)")
    a = ap.parse_args()
    steps, reps = (2, 3) if a.quick else (a.steps, a.reps)
    ramp()
    rec = {"device": torch.cuda.get_device_name(0), "steps": steps, "reps": reps, "legs": [], "kernel_resources": resources()}
    for name, (p, nb, T, L, nfft, hop) in legs().items():
        rec["legs"].append(fused_leg(name, p, nb, T, L, nfft, hop, steps, reps))
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec))
    if not a.quick:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
