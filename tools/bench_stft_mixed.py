#!/usr/bin/env python3
"""The mixed-radix fused window + FFT kernel (bhw_stft_mfft_f32_* / bhw.stft_mixed / bhw.spectrogram_mixed) on one GPU, one process, on
the protocol of tools/bench_stft_fft.py.  Prints one JSON record and writes it to --out (profiles/r19_stft_mixed.json by default).

Legs:
  W1 speech  BH-4, P 24, 32 b; B 64, T 160 000, L = n_fft 400, hop 160 (998 segments per signal)
  W2 long    BH-7, P 12, 32 b; B 1, T 2^24, L = n_fft 4000, hop 1000 (16 774 segments)
  W3 short   BH-4, P 24, 32 b; B 64, T 160 000, L = n_fft 96, hop 48 (3 332 segments per signal)
Per leg: the fused call from a table and in the library form (detrended segments, and the centred STFT) against the two-step route of
the same process -- welch_frames or stft_frames, then torch.fft.rfft -- and against a plain copy of its bytes (read B * T * 4, write
B * F * K * 8: one copy_ of half that many bytes each way).  On W1 also today's workaround, bhw.stft at 400 / 512, and
spectrogram_mixed with the 80-mel bank against bhw.spectrogram at 400 / 512 with its bank.
Accuracy: per leg, the largest relative l2 row error of the fused spectrum and of torch.fft.rfft over the same float32 rows, against
numpy.fft.rfft in float64 (a sample of the rows).
Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events, the variants of a leg alternated step
by step, after a clock ramp; times are per call (median, min, max over --steps).

    python tools/bench_stft_mixed.py [--steps 10] [--reps 20] [--out FILE] [--quick]
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
    return {"W1": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 400, 160),
            "W2": (B.make_params(B.WIN_BH7, 12, 32), 1, 1 << 24, 4000, 1000),
            "W3": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 96, 48)}


def ramp():
    """A second of work in front of the timed region: the clock has ramped when the first leg starts."""
    a = torch.randn((4096, 4096), device="cuda")
    for _ in range(40):
        a = (a @ a).clamp_(-1, 1)
    torch.cuda.synchronize()


def row_errors(Y, rows):
    Y, rows = Y.reshape(-1, Y.shape[-1]), rows.reshape(-1, rows.shape[-1])
    ref = np.fft.rfft(rows.astype(np.float64), axis=-1)
    nr = np.sqrt((np.abs(ref) ** 2).sum(-1))
    ne = np.sqrt((np.abs(Y.astype(np.complex128) - ref) ** 2).sum(-1))
    return float((ne[nr > 0] / nr[nr > 0]).max())


def accuracy_signal(nb, T, seed=3):
    """Noise + tones of 1e3 and 1e-3 + an offset: the signal of tools/bench_stft_fft.py."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = torch.arange(T, device="cuda", dtype=torch.float64)
    x = torch.randn((nb, T), device="cuda", generator=g, dtype=torch.float64) + 1e3 * torch.cos(2 * np.pi * 0.1234 * n) \
        + 1e-3 * torch.cos(2 * np.pi * 0.31 * n + 1.0) + 0.5
    return x.float()


def mixed_leg(name, p, nb, T, n, hop, steps, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((nb, T), device="cuda", generator=g) + 3.0
    L = n
    F = 1 + (T - L) // hop
    K = n // 2 + 1
    rec = {"leg": name, "B": nb, "T": T, "L": L, "nfft": n, "hop": hop, "frames": F}
    with bhw.ResidentTable(p) as t:
        seg = torch.empty((nb, F, n), device="cuda")
        mean = torch.empty(nb * F, device="cuda")
        Y = torch.empty((nb, F, K), dtype=torch.complex64, device="cuda")
        segc = t.stft_frames(p, x, n, hop)
        Yc = torch.empty((nb, segc.shape[1], K), dtype=torch.complex64, device="cuda")
        bytes_in, bytes_out = nb * T * 4, nb * F * K * 8
        half = (bytes_in + bytes_out) // 2 // 4
        src, dst = torch.empty(half, device="cuda"), torch.empty(half, device="cuda")
        kw = dict(center=False, detrend=True)
        fns = {"fused_table": lambda: t.stft_mixed(p, x, n, hop, out=Y, **kw),
               "fused_library": lambda: bhw.stft_mixed(p, x, n, hop, out=Y, **kw),
               "two_step": lambda: torch.fft.rfft(t.welch_frames(p, x, L, hop, nfft=n, out=seg, workspace=mean), dim=-1),
               "welch_frames": lambda: t.welch_frames(p, x, L, hop, nfft=n, out=seg, workspace=mean),
               "rfft_alone": lambda: torch.fft.rfft(seg, dim=-1),
               "fused_centred": lambda: t.stft_mixed(p, x, n, hop, out=Yc),
               "two_step_centred": lambda: torch.fft.rfft(t.stft_frames(p, x, n, hop, out=segc), dim=-1),
               "copy_of_its_bytes": lambda: dst.copy_(src)}
        if name == "W1":
            # today's workaround (other bins: 257 of them), and the mel front end at both sizes
            Fc = segc.shape[1]
            Y512 = torch.empty((nb, Fc, 257), dtype=torch.complex64, device="cuda")
            fb400 = bhw.FilterBank(bhw.mel_weights(400, 80, 16000), device="cuda")
            fb512 = bhw.FilterBank(bhw.mel_weights(512, 80, 16000), device="cuda")
            M = torch.empty((nb, Fc, 80), device="cuda")
            Pw = torch.empty((nb, Fc, K), device="cuda")
            fns.update({"stft_400_in_512": lambda: t.stft(p, x, 512, hop, win_length=400, out=Y512),
                        "mel_mixed_400": lambda: t.spectrogram_mixed(p, x, n, hop, fbank=fb400, out=M),
                        "mel_pow2_400_in_512": lambda: t.spectrogram(p, x, 512, hop, win_length=400, fbank=fb512, out=M),
                        "power_mixed_400": lambda: t.spectrogram_mixed(p, x, n, hop, out=Pw)})
        r = timed(fns, steps, reps)
        s = B.make_stft(nb, T, F, hop, n, shift=p.dat_width - 1)
        rec["plan"] = B.describe_stft_mfft(p, L, s, detrend=True, table=t.handle)
        m = {k: v["median_ms"] for k, v in r.items()}
        rec.update({"times": r, "bytes_in": bytes_in, "bytes_out": bytes_out,
                    "a_fused_over_two_step": m["fused_table"] / m["two_step"], "a_met": m["fused_table"] < m["two_step"],
                    "a_library_over_two_step": m["fused_library"] / m["two_step"],
                    "a_centred_fused_over_two_step": m["fused_centred"] / m["two_step_centred"],
                    "b_fused_over_copy": m["fused_table"] / m["copy_of_its_bytes"],
                    "fused_GBps": (bytes_in + bytes_out) / m["fused_table"] / 1e6,
                    "fused_GFLOPs": 2.5 * n * np.log2(n) * nb * F / m["fused_table"] / 1e6})
        if name == "W1":
            rec["workaround"] = {"mixed_400_over_pow2_400_in_512": m["fused_centred"] / m["stft_400_in_512"],
                                 "mel_mixed_400_over_mel_pow2_512": m["mel_mixed_400"] / m["mel_pow2_400_in_512"]}
        # accuracy on the leg's shape: a sample of the rows (at most 2000 rows of two signals)
        xa = accuracy_signal(min(nb, 2), min(T, L + 1999 * hop))
        rows = t.welch_frames(p, xa, L, hop, nfft=n)
        e_fused = row_errors(t.stft_mixed(p, xa, n, hop, **kw).cpu().numpy(), rows.cpu().numpy())
        e_rocfft = row_errors(torch.fft.rfft(rows, dim=-1).cpu().numpy(), rows.cpu().numpy())
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
        if k.startswith("k_stft_mfft"):
            key = json.dumps({n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy", "LDS Size")},
                             sort_keys=True)
            out.setdefault(key, []).append(k)
    return [{"figures": json.loads(k), "instances": len(v), "example": v[0],
             "note": "LDS Size is the static part (the direct form's ROM); the row buffers and twiddles are dynamic: the plan line's bytes"}
            for k, v in out.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_stft_mixed.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written (a profiler run)")
    a = ap.parse_args()
    steps, reps = (2, 3) if a.quick else (a.steps, a.reps)
    ramp()
    rec = {"device": torch.cuda.get_device_name(0), "steps": steps, "reps": reps, "legs": [], "kernel_resources": resources()}
    for name, (p, nb, T, n, hop) in legs().items():
        rec["legs"].append(mixed_leg(name, p, nb, T, n, hop, steps, reps))
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec))
    if not a.quick:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
