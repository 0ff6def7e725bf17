#!/usr/bin/env python3
"""The fused window + FFT kernel (bhw_stft_fft_f32_* / bhw.stft / fft="fused") on one GPU, one process.  Prints one JSON record and
writes it to --out (profiles/r14_stft_fft.json by default).

Legs: section 15's T1 and T2, plus a short transform
  T1 batch   BH-4, P 24, 32 b; B 64, T 160 000, L 400 in rows of 512, hop 160 (998 segments per signal)
  T2 long    BH-7, P 12, 32 b; B 1, T 2^24, L = nfft 4096, hop 1024 (16 381 segments)
  N64 short  BH-4, P 24, 32 b; B 64, T 160 000, L = nfft 64, hop 32 (4 999 segments per signal)
(a) the fused call (detrended segments, and the centred STFT) against the two-step route of the same process: welch_frames or
    stft_frames, then torch.fft.rfft;
(b) against a plain copy of its bytes (read B * T * 4, write B * F * K * 8: one copy_ of half that many bytes each way);
(c) welch and cross_spectra end to end, fft="fused" against fft="torch";
(d) --ab ROOT: welch_psd on T1 and T2 from the package under ROOT (the parent's tree or this one), for the no-regression lines.
Accuracy: per leg, the largest relative l2 row error of the fused spectrum and of torch.fft.rfft over the same float32 rows, against
numpy.fft.rfft in float64 (the figures of tests/test_gpu_stft_fft.py on the benchmarked shapes; a sample of the rows).
Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events, the variants of a leg alternated step
by step, after a clock ramp; times are per call (median, min, max over --steps).

    python tools/bench_stft_fft.py [--steps 10] [--reps 20] [--out FILE] [--quick]
    python tools/bench_stft_fft.py --ab ROOT     one JSON line: welch_psd and the two-step route from the package under ROOT
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB = sys.argv[sys.argv.index("--ab") + 1] if "--ab" in sys.argv else None
sys.path.insert(0, os.path.abspath(AB) if AB else ROOT)
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
    return {"T1": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 400, 512, 160),
            "T2": (B.make_params(B.WIN_BH7, 12, 32), 1, 1 << 24, 4096, 4096, 1024),
            "N64": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 64, 64, 32)}


def ramp():
    """A second of work in front of the timed region: the clock has ramped when the first leg starts."""
    a = torch.randn((4096, 4096), device="cuda")
    for _ in range(40):
        a = (a @ a).clamp_(-1, 1)
    torch.cuda.synchronize()


def ab_main(steps, reps):
    """Calls both trees have: welch_psd on the rfft of each leg's segments, and the two-step route."""
    assert os.path.abspath(bhw.__file__).startswith(os.path.abspath(AB)), bhw.__file__
    ramp()
    out = {"root": os.path.abspath(AB)}
    g = torch.Generator(device="cuda").manual_seed(1)
    for name, (p, nb, T, L, nfft, hop) in legs().items():
        x = torch.randn((nb, T), device="cuda", generator=g) + 3.0
        with bhw.ResidentTable(p) as t:
            seg = t.welch_frames(p, x, L, hop, nfft=nfft)
            Y = torch.fft.rfft(seg, dim=-1)
            P = torch.empty((nb, Y.shape[-1]), device="cuda")
            F = Y.shape[1]
            ws = torch.empty(nb * (-(-F // 256)) * Y.shape[-1], dtype=torch.float64, device="cuda")
            mean = torch.empty(nb * F, device="cuda")
            r = timed({"welch_psd": lambda: bhw.welch_psd(Y, 1.0 / F, nfft=nfft, out=P, workspace=ws if F > 256 else None),
                       "welch_frames": lambda: t.welch_frames(p, x, L, hop, nfft=nfft, out=seg, workspace=mean),
                       "welch_torch_route": lambda: t.welch(p, x, length=L, noverlap=L - hop, nfft=nfft)}, steps, reps)
        out[name] = {k: v["median_ms"] * 1000 for k, v in r.items()}
        del x, seg, Y, P, ws
        torch.cuda.empty_cache()
    print(json.dumps(out))


def row_errors(Y, rows):
    Y, rows = Y.reshape(-1, Y.shape[-1]), rows.reshape(-1, rows.shape[-1])
    ref = np.fft.rfft(rows.astype(np.float64), axis=-1)
    nr = np.sqrt((np.abs(ref) ** 2).sum(-1))
    ne = np.sqrt((np.abs(Y.astype(np.complex128) - ref) ** 2).sum(-1))
    return float((ne[nr > 0] / nr[nr > 0]).max())


def accuracy_signal(nb, T, seed=3):
    """Noise + tones of 1e3 and 1e-3 + an offset: the structure of section 15's signal, at the amplitudes of the issue's rehearsal."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = torch.arange(T, device="cuda", dtype=torch.float64)
    x = torch.randn((nb, T), device="cuda", generator=g, dtype=torch.float64) + 1e3 * torch.cos(2 * np.pi * 0.1234 * n) \
        + 1e-3 * torch.cos(2 * np.pi * 0.31 * n + 1.0) + 0.5
    return x.float()


def fused_leg(name, p, nb, T, L, nfft, hop, steps, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((nb, T), device="cuda", generator=g) + 3.0
    F = 1 + (T - L) // hop
    K = nfft // 2 + 1
    rec = {"leg": name, "B": nb, "T": T, "L": L, "nfft": nfft, "hop": hop, "frames": F}
    with bhw.ResidentTable(p) as t:
        seg = torch.empty((nb, F, nfft), device="cuda")
        mean = torch.empty(nb * F, device="cuda")
        Y = torch.empty((nb, F, K), dtype=torch.complex64, device="cuda")
        segc = t.stft_frames(p, x, nfft, hop, win_length=L)
        Yc = torch.empty((nb, segc.shape[1], K), dtype=torch.complex64, device="cuda")
        bytes_in, bytes_out = nb * T * 4, nb * F * K * 8
        half = (bytes_in + bytes_out) // 2 // 4
        src, dst = torch.empty(half, device="cuda"), torch.empty(half, device="cuda")
        kw = dict(win_length=L, center=False, detrend=True)
        r = timed({"fused_table": lambda: t.stft(p, x, nfft, hop, out=Y, **kw),
                   "fused_library": lambda: bhw.stft(p, x, nfft, hop, out=Y, **kw),
                   "two_step": lambda: torch.fft.rfft(t.welch_frames(p, x, L, hop, nfft=nfft, out=seg, workspace=mean), dim=-1),
                   "welch_frames": lambda: t.welch_frames(p, x, L, hop, nfft=nfft, out=seg, workspace=mean),
                   "rfft_alone": lambda: torch.fft.rfft(seg, dim=-1),
                   "fused_centred": lambda: t.stft(p, x, nfft, hop, win_length=L, out=Yc),
                   "two_step_centred": lambda: torch.fft.rfft(t.stft_frames(p, x, nfft, hop, win_length=L, out=segc), dim=-1),
                   "copy_of_its_bytes": lambda: dst.copy_(src)}, steps, reps)
        rec["plan"] = B.describe_stft_fft(p, L, B.make_stft(nb, T, F, hop, nfft, shift=p.dat_width - 1), detrend=True, table=t.handle)
        m = {k: v["median_ms"] for k, v in r.items()}
        rec.update({"times": r, "bytes_in": bytes_in, "bytes_out": bytes_out,
                    "a_fused_over_two_step": m["fused_table"] / m["two_step"], "a_met": m["fused_table"] < m["two_step"],
                    "a_centred_fused_over_two_step": m["fused_centred"] / m["two_step_centred"],
                    "b_fused_over_copy": m["fused_table"] / m["copy_of_its_bytes"], "b_target": 1.15,
                    "b_met": m["fused_table"] <= 1.15 * m["copy_of_its_bytes"],
                    "fused_GBps": (bytes_in + bytes_out) / m["fused_table"] / 1e6,
                    "fused_GFLOPs": 2.5 * nfft * np.log2(nfft) * nb * F / m["fused_table"] / 1e6})
        # accuracy on the leg's shape: a sample of the rows (the first signal, at most 2000 rows)
        xa = accuracy_signal(min(nb, 2), min(T, L + 1999 * hop))
        rows = t.welch_frames(p, xa, L, hop, nfft=nfft)
        e_fused = row_errors(t.stft(p, xa, nfft, hop, **kw).cpu().numpy(), rows.cpu().numpy())
        e_rocfft = row_errors(torch.fft.rfft(rows, dim=-1).cpu().numpy(), rows.cpu().numpy())
        rec["accuracy"] = {"rows": int(rows.shape[0] * rows.shape[1]), "fused_rel_l2": e_fused, "rocfft_rel_l2": e_rocfft, "ratio": e_fused / e_rocfft,
                           "bound": 2.0, "cap": 2.0 ** -24 * float(np.log2(nfft)), "met": e_fused <= 2.0 * e_rocfft}
        # (c) end to end
        y = torch.randn((nb, T), device="cuda", generator=g)
        for fft in ("torch", "fused"):
            t.welch(p, x, length=L, noverlap=L - hop, nfft=nfft, fft=fft)
        e = timed({"welch_torch": lambda: t.welch(p, x, length=L, noverlap=L - hop, nfft=nfft),
                   "welch_fused": lambda: t.welch(p, x, length=L, noverlap=L - hop, nfft=nfft, fft="fused"),
                   "cross_spectra_torch": lambda: t.cross_spectra(p, x, y, length=L, noverlap=L - hop, nfft=nfft),
                   "cross_spectra_fused": lambda: t.cross_spectra(p, x, y, length=L, noverlap=L - hop, nfft=nfft, fft="fused")}, steps, reps)
        me = {k: v["median_ms"] for k, v in e.items()}
        rec["end_to_end"] = {"times": e, "c_welch_fused_over_torch": me["welch_fused"] / me["welch_torch"],
                             "c_cross_spectra_fused_over_torch": me["cross_spectra_fused"] / me["cross_spectra_torch"]}
    return rec


def resources():
    path = os.path.join(ROOT, "blackman_harris_win_amd", "kernel_resources.json")
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        res = json.load(f)
    out = {}
    for k, v in res.items():
        if k.startswith("k_stft_fft"):
            key = json.dumps({n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "SGPRs Spill", "ScratchSize", "Occupancy", "LDS Size")}, sort_keys=True)
            out.setdefault(key, []).append(k)
    return [{"figures": json.loads(k), "instances": len(v), "example": v[0],
             "note": "LDS Size is the static part (the direct form's ROM); the row buffers and twiddles are dynamic: the plan line's bytes"}
            for k, v in out.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_stft_fft.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written (a profiler run)")
    ap.add_argument("--ab", default=None)
    a = ap.parse_args()
    steps, reps = (2, 3) if a.quick else (a.steps, a.reps)
    if a.ab:
        return ab_main(steps, reps)
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
