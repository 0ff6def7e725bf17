#!/usr/bin/env python3
"""The fused inverse mixed-radix FFT + overlap-add kernel (bhw_istft_mfft_f32_* / bhw.istft_mixed) on one GPU, one process.  Prints one
JSON record and writes it to --out (profiles/r20_istft_mixed.json by default).  The protocol of tools/bench_istft_fft.py.

Legs: the inverses of section 23's legs, centred as torch.istft frames them
  W1 speech  BH-4, P 24, 32 b; B 64, 998 frames of 201 bins, L = nfft 400, hop 160 (T 159 520)
  W2 long    BH-7, P 12, 32 b; B 1, T 2^24, L = nfft 4000, hop 1000
  W3 short   BH-4, P 24, 32 b; B 64, T 160 000, L = nfft 96, hop 48
Per leg, from the spectra Y = stft_mixed(x) of a noise signal:
(a) the fused call, table and library form, against the two-step route of the same process: torch.fft.irfft(Y, n=nfft), then
    istft_overlap_add from the table; each part of the two-step route alone;
(b) against a plain copy of its bytes (read B * F * K * 8, write B * T * 4: one copy_ of half that many bytes each way);
(c) the round trip stft_mixed -> istft_mixed against stft_frames + rfft -> irfft + istft_overlap_add;
(d) on W1, for scale, bhw.istft at 400 / 512 / 160 on a 257-bin spectrum of the same batch.
Accuracy: the relative l2 error of the fused output and of the two-step route against numpy in float64 (the reference of
tests/test_gpu_istft_mixed.py) on two signals of at most 2000 frames.
Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events, the variants of a leg alternated step
by step, after a clock ramp; times are per call (median, min, max over --steps).

    python tools/bench_istft_mixed.py [--steps 10] [--reps 20] [--out FILE] [--quick]
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
    return {"W1": (B.make_params(B.WIN_BH4, 24, 32), 64, 159520, 400, 400, 160),
            "W2": (B.make_params(B.WIN_BH7, 12, 32), 1, 1 << 24, 4000, 4000, 1000),
            "W3": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 96, 96, 48)}


def ramp():
    """A second of work in front of the timed region: the clock has ramped when the first leg starts."""
    a = torch.randn((4096, 4096), device="cuda")
    for _ in range(40):
        a = (a @ a).clamp_(-1, 1)
    torch.cuda.synchronize()


def ref64(Yh, v, nfft, hop, col0, pad, T):
    """numpy in float64: irfft of every row, the overlap-add with the float32 v, divided by the envelope."""
    nb, F, _ = Yh.shape
    L, t0 = len(v), pad - col0
    vd = v.astype(np.float64)
    S, E = np.zeros((nb, max(t0 + T, (F - 1) * hop + L))), np.zeros(max(t0 + T, (F - 1) * hop + L))
    rows = np.fft.irfft(Yh.astype(np.complex128), n=nfft, axis=-1)
    for f in range(F):
        S[:, f * hop:f * hop + L] += rows[:, f, col0:col0 + L] * vd
        E[f * hop:f * hop + L] += vd * vd
    S, E = S[:, t0:t0 + T], E[t0:t0 + T]
    return np.where(E > 0, S / np.where(E > 0, E, 1.0), 0.0)


def rel_l2(got, ref):
    got = got.astype(np.float64)
    return float((np.sqrt(((got - ref) ** 2).sum(-1)) / np.sqrt((ref ** 2).sum(-1))).max())


def inverse_leg(name, p, nb, T, L, nfft, hop, steps, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((nb, T), device="cuda", generator=g) + 3.0
    K, pad, col0 = nfft // 2 + 1, nfft // 2, (nfft - L) // 2
    kw = dict(win_length=L, length=T)
    rec = {"leg": name, "B": nb, "T": T, "L": L, "nfft": nfft, "hop": hop}
    with bhw.ResidentTable(p) as t:
        Y = t.stft_mixed(p, x, nfft, hop, win_length=L)
        F = Y.shape[1]
        rec["frames"] = F
        out = torch.empty((nb, T), device="cuda")
        rows = torch.fft.irfft(Y, n=nfft, dim=-1)
        seg = torch.empty((nb, F, nfft), device="cuda")
        bytes_in, bytes_out = nb * F * K * 8, nb * T * 4
        half = (bytes_in + bytes_out) // 2 // 4
        src, dst = torch.empty(half, device="cuda"), torch.empty(half, device="cuda")
        fns = {"fused_table": lambda: t.istft_mixed(p, Y, nfft, hop, out=out, **kw),
               "fused_library": lambda: bhw.istft_mixed(p, Y, nfft, hop, out=out, **kw),
               "two_step": lambda: t.istft_overlap_add(p, torch.fft.irfft(Y, n=nfft, dim=-1), nfft, hop, out=out, **kw),
               "irfft_alone": lambda: torch.fft.irfft(Y, n=nfft, dim=-1),
               "overlap_add_alone": lambda: t.istft_overlap_add(p, rows, nfft, hop, out=out, **kw),
               "copy_of_its_bytes": lambda: dst.copy_(src),
               "round_trip_fused": lambda: t.istft_mixed(p, t.stft_mixed(p, x, nfft, hop, win_length=L, out=Y), nfft, hop, out=out, **kw),
               "round_trip_two_step": lambda: t.istft_overlap_add(
                   p, torch.fft.irfft(torch.fft.rfft(t.stft_frames(p, x, nfft, hop, win_length=L, out=seg), dim=-1), n=nfft, dim=-1),
                   nfft, hop, out=out, **kw)}
        if name == "W1":                                     # for scale: the power-of-two kernel on rows of 512 of the same batch
            Y2 = t.stft(p, x, 512, hop, win_length=L)
            fns["power_of_two_istft_400_512_160"] = lambda: t.istft(p, Y2, 512, hop, out=out, **kw)
        r = timed(fns, steps, reps)
        s = B.make_stft(nb, T, F, hop, nfft, col0=col0, pad=pad, shift=p.dat_width - 1)
        rec["plan"] = B.describe_istft_mfft(p, L, s, normalize=True, table=t.handle)
        m = {k: v["median_ms"] for k, v in r.items()}
        rec.update({"times": r, "bytes_in": bytes_in, "bytes_out": bytes_out,
                    "bytes_the_two_step_route_adds": 2 * nb * F * nfft * 4,
                    "fused_over_two_step": m["fused_table"] / m["two_step"],
                    "library_over_table": m["fused_library"] / m["fused_table"],
                    "fused_over_copy": m["fused_table"] / m["copy_of_its_bytes"],
                    "round_trip_fused_over_two_step": m["round_trip_fused"] / m["round_trip_two_step"],
                    "fused_GBps": (bytes_in + bytes_out) / m["fused_table"] / 1e6})
        if name == "W1":
            rec["fused_over_power_of_two_istft"] = m["fused_table"] / m["power_of_two_istft_400_512_160"]
        del rows, seg, src, dst
        # accuracy: two signals of at most 2000 frames of the leg's shape
        Fa = min(F, 2000)
        Ta = nfft + hop * (Fa - 1) - 2 * pad
        Ya = Y[:min(nb, 2), :Fa].contiguous()
        v = np.ldexp(bhw.window(p, L).cpu().numpy().astype(np.float32), -(p.dat_width - 1)).astype(np.float32)
        ref = ref64(Ya.cpu().numpy(), v, nfft, hop, col0, pad, Ta)
        e_fused = rel_l2(t.istft_mixed(p, Ya, nfft, hop, win_length=L, length=Ta).cpu().numpy(), ref)
        e_two = rel_l2(t.istft_overlap_add(p, torch.fft.irfft(Ya, n=nfft, dim=-1), nfft, hop, win_length=L, length=Ta).cpu().numpy(), ref)
        cap = 2.0 ** -24 * float(np.log2(nfft))
        rec["accuracy"] = {"rows": int(Ya.shape[0] * Fa), "fused_rel_l2": e_fused, "two_step_rel_l2": e_two, "ratio": e_fused / e_two,
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
        if k.startswith("k_istft_mfft"):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_istft_mixed.json"))
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
