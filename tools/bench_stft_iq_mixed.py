#!/usr/bin/env python3
"""The mixed-radix fused window + complex FFT kernel for I/Q input (bhw_stft_cmfft_f32_* / bhw.stft_iq_mixed /
bhw.spectrogram_iq_mixed) on one GPU, one process.  Prints one JSON record and writes it to --out
(profiles/r26_stft_iq_mixed.json by default).  The protocol is that of tools/bench_stft_iq.py and tools/bench_stft_mixed.py.

Legs, complex64, BH-4, P 24, 32 b
  A400   B 64, T 160 000, L = n_fft 400, hop 160 (998 segments per signal), detrended
  A400p  the power form of A400, against the two-step route followed by |Y|^2
  L2000  B 1, T 2^24, L = n_fft 2000, hop 500 (33 551 frames), no padding, no detrending (stft_frames is the two-step route's first call)
  M1536  B 64, T 160 000, L = n_fft 1536, hop 384 (413 segments per signal), detrended
  S96    B 64, T 160 000, L = n_fft 96, hop 48 (3 332 segments per signal), detrended
Variants: the fused call from a table and in library form; the two-step route of the same process, welch_frames (or stft_frames) +
torch.fft.fft, together and each alone, with its own spread; a plain copy of the call's bytes (read B * T * 8, write the output's
bytes: one copy_ of half that many bytes each way).
Accuracy: per leg, the largest relative l2 row error of the fused spectrum and of torch.fft.fft (rocFFT) over the same float32 rows,
against numpy.fft.fft in float64, and the fused error as a share of rocFFT's.
Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events, the variants of a leg alternated step
by step, after a clock ramp; times are per call (median, min, max over --steps).

    python tools/bench_stft_iq_mixed.py [--steps 10] [--reps 20] [--out FILE] [--quick]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import blackman_harris_win_amd as bhw  # noqa: E402
from blackman_harris_win_amd import binding as B  # noqa: E402
from bench_stft_iq import accuracy_signal, ramp, row_errors, timed  # noqa: E402


def legs():
    p = B.make_params(B.WIN_BH4, 24, 32)
    # name: (params, B, T, n_fft, hop, detrend, power)
    return {"A400": (p, 64, 160000, 400, 160, True, False), "A400p": (p, 64, 160000, 400, 160, True, True),
            "L2000": (p, 1, 1 << 24, 2000, 500, False, False), "M1536": (p, 64, 160000, 1536, 384, True, False),
            "S96": (p, 64, 160000, 96, 48, True, False)}


def fused_leg(name, p, nb, T, n, hop, detrend, power, steps, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((nb, T, 2), device="cuda", generator=g)) + (3.0 - 1.0j)
    F = 1 + (T - n) // hop
    rec = {"leg": name, "B": nb, "T": T, "L": n, "nfft": n, "hop": hop, "frames": F, "detrend": detrend, "power": power}
    with bhw.ResidentTable(p) as t:
        seg = torch.empty((nb, F, n), dtype=torch.complex64, device="cuda")
        mean = torch.empty(nb * F * 2, device="cuda")
        out = torch.empty((nb, F, n), dtype=torch.float32 if power else torch.complex64, device="cuda")
        bytes_in, bytes_out = nb * T * 8, out.numel() * out.element_size()
        half = (bytes_in + bytes_out) // 2 // 4
        src, dst = torch.empty(half, device="cuda"), torch.empty(half, device="cuda")
        kw = dict(win_length=n, center=False, detrend=detrend)
        if detrend:
            def frames_call():
                return t.welch_frames(p, x, n, hop, nfft=n, out=seg, workspace=mean)
        else:
            def frames_call():
                return t.stft_frames(p, x, n, hop, win_length=n, center=False, out=seg)
        if power:
            def two_step():
                return torch.view_as_real(torch.fft.fft(frames_call(), dim=-1)).square().sum(-1)
            fused_t, fused_l = t.spectrogram_iq_mixed, bhw.spectrogram_iq_mixed
        else:
            def two_step():
                return torch.fft.fft(frames_call(), dim=-1)
            fused_t, fused_l = t.stft_iq_mixed, bhw.stft_iq_mixed
        r = timed({"fused_table": lambda: fused_t(p, x, n, hop, out=out, **kw),
                   "fused_library": lambda: fused_l(p, x, n, hop, out=out, **kw),
                   "two_step": two_step,
                   "frames_alone": frames_call,
                   "fft_alone": lambda: torch.fft.fft(seg, dim=-1),
                   "copy_of_its_bytes": lambda: dst.copy_(src)}, steps, reps)
        rec["plan"] = B.describe_stft_cmfft(p, n, B.make_stft(nb, T, F, hop, n, channels=2, shift=p.dat_width - 1), detrend=detrend, power=power,
                                            table=t.handle)
        m = {k: v["median_ms"] for k, v in r.items()}
        rec.update({"times": r, "bytes_in": bytes_in, "bytes_out": bytes_out,
                    "fused_over_two_step": m["fused_table"] / m["two_step"], "fused_below_two_step": m["fused_table"] < m["two_step"],
                    "fused_over_two_step_range": [r["fused_table"]["min_ms"] / r["two_step"]["max_ms"],
                                                  r["fused_table"]["max_ms"] / r["two_step"]["min_ms"]],
                    "library_over_table": m["fused_library"] / m["fused_table"],
                    "fused_over_copy": m["fused_table"] / m["copy_of_its_bytes"],
                    "fused_GBps": (bytes_in + bytes_out) / m["fused_table"] / 1e6,
                    "fused_GFLOPs": 5.0 * n * np.log2(n) * nb * F / m["fused_table"] / 1e6})
        # accuracy on the leg's shape: 2 signals, at most 2000 rows each
        xa = accuracy_signal(min(nb, 2), min(T, n + 1999 * hop))
        rows = t.welch_frames(p, xa, n, hop, nfft=n) if detrend else t.stft_frames(p, xa, n, hop, win_length=n, center=False)
        e_fused = row_errors(t.stft_iq_mixed(p, xa, n, hop, **kw).cpu().numpy(), rows.cpu().numpy())
        e_rocfft = row_errors(torch.fft.fft(rows, dim=-1).cpu().numpy(), rows.cpu().numpy())
        rec["accuracy"] = {"rows": int(rows.shape[0] * rows.shape[1]), "fused_rel_l2": e_fused, "rocfft_rel_l2": e_rocfft, "ratio": e_fused / e_rocfft,
                           "bound": 2.0, "cap": 2.0 ** -24 * float(np.log2(n)), "met": e_fused <= 2.0 * e_rocfft}
    return rec


def resources():
    path = os.path.join(ROOT, "blackman_harris_win_amd", "kernel_resources.json")
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        res = json.load(f)
    out = {}
    for k, v in res.items():
        if k.startswith("k_stft_cmfft"):
            key = json.dumps({n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "SGPRs Spill", "ScratchSize", "Occupancy", "LDS Size")}, sort_keys=True)
            out.setdefault(key, []).append(k)
    return [{"figures": json.loads(k), "instances": len(v), "example": v[0],
             "note": "LDS Size is the static part (the direct form's ROM); the row buffers and twiddles are dynamic: the plan line's bytes"}
            for k, v in out.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_stft_iq_mixed.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written (a profiler run)")
    a = ap.parse_args()
    steps, reps = (2, 3) if a.quick else (a.steps, a.reps)
    ramp()
    rec = {"device": torch.cuda.get_device_name(0), "steps": steps, "reps": reps, "legs": [], "kernel_resources": resources()}
    for name, (p, nb, T, n, hop, detrend, power) in legs().items():
        rec["legs"].append(fused_leg(name, p, nb, T, n, hop, detrend, power, steps, reps))
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec))
    if not a.quick:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
