#!/usr/bin/env python3
"""The fused inverse mixed-radix complex FFT + overlap-add kernel for I/Q output (bhw_istft_cmfft_f32_* / bhw.istft_iq_mixed) on one
GPU, one process.  Prints one JSON record and writes it to --out (profiles/r27_istft_iq_mixed.json by default).  The protocol of
tools/bench_istft_mixed.py.

Legs: the inverses of section 30's legs, centred as torch.istft frames them, complex signals
  W1 speech  BH-4, P 24, 32 b; B 64, T 160 000, L = nfft 400, hop 160
  W2 long    BH-7, P 12, 32 b; B 1, T 2^24, L = nfft 2000, hop 500
  W3 LTE     BH-4, P 24, 32 b; B 64, T 160 000, L = nfft 1536, hop 384
  W4 short   BH-4, P 24, 32 b; B 64, T 160 000, L = nfft 96, hop 48
Per leg, from the spectra Y = stft_iq_mixed(x) of a complex noise signal:
(a) the fused call, table and library form, against the two-call route of the same process: torch.fft.ifft(Y), then
    istft_overlap_add from the table; each part of the two-call route alone;
(b) against a plain copy of its bytes (read B * F * nfft * 8, write B * T * 8: one copy_ of half that many bytes each way);
(c) the round trip stft_iq_mixed -> istft_iq_mixed against stft_frames + fft -> ifft + istft_overlap_add.
Accuracy: the relative l2 error of the fused output and of the two-call route against numpy in float64 (the reference of
tests/test_gpu_istft_iq_mixed.py) on two signals of at most 2000 frames.
Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events, the variants of a leg alternated step
by step, after a clock ramp; times are per call (median, min, max over --steps).

    python tools/bench_istft_iq_mixed.py [--steps 10] [--reps 20] [--out FILE] [--quick]
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
    return {"W1": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 400, 400, 160),
            "W2": (B.make_params(B.WIN_BH7, 12, 32), 1, 1 << 24, 2000, 2000, 500),
            "W3": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 1536, 1536, 384),
            "W4": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 96, 96, 48)}


def ramp():
    """A second of work in front of the timed region: the clock has ramped when the first leg starts."""
    a = torch.randn((4096, 4096), device="cuda")
    for _ in range(40):
        a = (a @ a).clamp_(-1, 1)
    torch.cuda.synchronize()


def ref64(Yh, v, hop, col0, pad, T):
    """numpy in float64: ifft of every row, the overlap-add with the float32 v per part, divided by the envelope."""
    nb, F, _ = Yh.shape
    L, t0 = len(v), pad - col0
    vd = v.astype(np.float64)
    W = max(t0 + T, (F - 1) * hop + L)
    S, E = np.zeros((nb, W), dtype=np.complex128), np.zeros(W)
    rows = np.fft.ifft(Yh.astype(np.complex128), axis=-1)
    for f in range(F):
        S[:, f * hop:f * hop + L] += rows[:, f, col0:col0 + L] * vd
        E[f * hop:f * hop + L] += vd * vd
    S, E = S[:, t0:t0 + T], E[t0:t0 + T]
    return np.where(E > 0, S / np.where(E > 0, E, 1.0), 0.0)


def rel_l2(got, ref):
    got = got.astype(np.complex128)
    return float((np.sqrt((np.abs(got - ref) ** 2).sum(-1)) / np.sqrt((np.abs(ref) ** 2).sum(-1))).max())


def inverse_leg(name, p, nb, T, L, nfft, hop, steps, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((nb, T, 2), device="cuda", generator=g) + 3.0)
    pad, col0 = nfft // 2, (nfft - L) // 2
    kw = dict(win_length=L, length=T)
    rec = {"leg": name, "B": nb, "T": T, "L": L, "nfft": nfft, "hop": hop}
    with bhw.ResidentTable(p) as t:
        Y = t.stft_iq_mixed(p, x, nfft, hop, win_length=L)
        F = Y.shape[1]
        rec["frames"] = F
        out = torch.empty((nb, T), dtype=torch.complex64, device="cuda")
        rows = torch.fft.ifft(Y, dim=-1)
        seg = torch.empty((nb, F, nfft), dtype=torch.complex64, device="cuda")
        bytes_in, bytes_out = nb * F * nfft * 8, nb * T * 8
        half = (bytes_in + bytes_out) // 2 // 4
        src, dst = torch.empty(half, device="cuda"), torch.empty(half, device="cuda")
        fns = {"fused_table": lambda: t.istft_iq_mixed(p, Y, nfft, hop, out=out, **kw),
               "fused_library": lambda: bhw.istft_iq_mixed(p, Y, nfft, hop, out=out, **kw),
               "two_call": lambda: t.istft_overlap_add(p, torch.fft.ifft(Y, dim=-1), nfft, hop, out=out, **kw),
               "ifft_alone": lambda: torch.fft.ifft(Y, dim=-1),
               "overlap_add_alone": lambda: t.istft_overlap_add(p, rows, nfft, hop, out=out, **kw),
               "copy_of_its_bytes": lambda: dst.copy_(src),
               "round_trip_fused": lambda: t.istft_iq_mixed(p, t.stft_iq_mixed(p, x, nfft, hop, win_length=L, out=Y), nfft, hop, out=out, **kw),
               "round_trip_two_call": lambda: t.istft_overlap_add(
                   p, torch.fft.ifft(torch.fft.fft(t.stft_frames(p, x, nfft, hop, win_length=L, out=seg), dim=-1), dim=-1), nfft, hop, out=out, **kw)}
        r = timed(fns, steps, reps)
        s = B.make_stft(nb, T, F, hop, nfft, col0=col0, pad=pad, channels=2, shift=p.dat_width - 1)
        rec["plan"] = B.describe_istft_cmfft(p, L, s, normalize=True, table=t.handle)
        m = {k: v["median_ms"] for k, v in r.items()}
        rec.update({"times": r, "bytes_in": bytes_in, "bytes_out": bytes_out,
                    "bytes_the_two_call_route_adds": 2 * nb * F * nfft * 8,
                    "fused_over_two_call": m["fused_table"] / m["two_call"],
                    "library_over_table": m["fused_library"] / m["fused_table"],
                    "fused_over_copy": m["fused_table"] / m["copy_of_its_bytes"],
                    "round_trip_fused_over_two_call": m["round_trip_fused"] / m["round_trip_two_call"],
                    "fused_GBps": (bytes_in + bytes_out) / m["fused_table"] / 1e6})
        del rows, seg, src, dst
        # accuracy: two signals of at most 2000 frames of the leg's shape
        Fa = min(F, 2000)
        Ta = nfft + hop * (Fa - 1) - 2 * pad
        Ya = Y[:min(nb, 2), :Fa].contiguous()
        v = np.ldexp(bhw.window(p, L).cpu().numpy().astype(np.float32), -(p.dat_width - 1)).astype(np.float32)
        ref = ref64(Ya.cpu().numpy(), v, hop, col0, pad, Ta)
        e_fused = rel_l2(t.istft_iq_mixed(p, Ya, nfft, hop, win_length=L, length=Ta).cpu().numpy(), ref)
        e_two = rel_l2(t.istft_overlap_add(p, torch.fft.ifft(Ya, dim=-1), nfft, hop, win_length=L, length=Ta).cpu().numpy(), ref)
        cap = 2.0 ** -24 * float(np.log2(nfft))
        rec["accuracy"] = {"rows": int(Ya.shape[0] * Fa), "fused_rel_l2": e_fused, "two_call_rel_l2": e_two, "ratio": e_fused / e_two,
                           "bound": 2.0, "cap": cap, "met": e_fused <= 2.0 * e_two and e_fused <= cap}
    return rec


def resources():
    path = os.path.join(ROOT, "blackman_harris_win_amd", "kernel_resources.json")
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        res = json.load(f)
    out = {}
    for k, v in res.items():
        if k.startswith("k_istft_cmfft"):
            key = json.dumps({n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy", "LDS Size")},
                             sort_keys=True)
            out.setdefault(key, []).append(k)
    return [{"figures": json.loads(k), "instances": len(v), "example": v[0],
             "note": "LDS Size is the static part (the direct form's ROM); the buffers, twiddles and window are dynamic: the plan line's bytes"}
            for k, v in out.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_istft_iq_mixed.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written (a profiler run)")
    a = ap.parse_args()
    steps, reps = (2, 3) if a.quick else (a.steps, a.reps)
    ramp()
    rec = {"device": torch.cuda.get_device_name(0), "steps": steps, "reps": reps, "legs": [], "kernel_resources": resources()}
    for name, (p, nb, T, L, nfft, hop) in legs().items():
        rec["legs"].append(inverse_leg(name, p, nb, T, L, nfft, hop, steps, reps))
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec))
    if not a.quick:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
