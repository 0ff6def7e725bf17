#!/usr/bin/env python3
"""The fused max-hold / min-hold traces for real input (bhw_hold_fft_f32_* / bhw_hold_mfft_f32_*; bhw.hold_fft, hold_fft_mixed) on one
GPU, one process.  Prints one JSON record and writes it to --out (profiles/r31_hold_real.json by default).  The protocol is
tools/bench_hold_iq.py's.

Legs, float32 input, the legs of the real Welch siblings (DESIGN.md sections 26 and 28):
  T1 batch   BH-4, P 24, 32 b; B 64, T 160 000, window 400 in rows of 512, hop 160 (998 segments per signal)
  T1M batch  the same at rows of 400, the mixed-radix family
  T2 long    BH-7, P 12, 32 b; B 1, T 2^24, 4096 / hop 1024 (16 381 segments)
  T3 long    BH-7, P 12, 32 b; B 1, T 2^24, 4000 / hop 1000 (16 774 segments), mixed
  N64 short  BH-4, P 24, 32 b; B 64, T 160 000, 64 / 64 / hop 32 (4 999 segments per signal)
  N96 short  BH-4, P 24, 32 b; B 64, T 160 000, 96 / hop 48 (3 332 segments per signal), mixed
  ONE block  BH-4, P 24, 32 b; B 64, 200 segments of 400 in rows of 512, hop 160
  ONEM block the same at rows of 400, mixed
Variants, detrended segments, every output and workspace given, one resident table:
  (a) hold_fft(_mixed) from the table, both traces         (b) hold_fft(_mixed), the library form
  (c) spectrogram(_mixed) + amax + amin over the frames, the route (a) replaces, from the same table
  (d) spectrogram(_mixed) alone                            (e) welch_fft(_mixed), the mean of the same frames
The aim: (a) below (c) on every leg.  A leg counts as met or missed only beyond (c)'s own spread in the record, (max - min) / median of
its step medians; it is no test gate.  Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events,
the variants of a leg alternated step by step, after a clock ramp; times are per call (median, min, max over --steps).  The record also
holds the equality of (a) with (c) on the benchmarked data (the contract is exact), and the compiler's figures for the kernels.

    python tools/bench_hold_real.py [--steps 10] [--reps 20] [--out FILE] [--quick] [--legs T1,T2]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
    bh4 = B.make_params(B.WIN_BH4, 24, 32)
    bh7 = B.make_params(B.WIN_BH7, 12, 32)
    # (params, B, T, L, nfft, hop)
    return {"T1": (bh4, 64, 160000, 400, 512, 160),
            "T1M": (bh4, 64, 160000, 400, 400, 160),
            "T2": (bh7, 1, 1 << 24, 4096, 4096, 1024),
            "T3": (bh7, 1, 1 << 24, 4000, 4000, 1000),
            "N64": (bh4, 64, 160000, 64, 64, 32),
            "N96": (bh4, 64, 160000, 96, 96, 48),
            "ONE": (bh4, 64, 199 * 160 + 400, 400, 512, 160),
            "ONEM": (bh4, 64, 199 * 160 + 400, 400, 400, 160)}


def ramp():
    """A second of work in front of the timed region: the clock has ramped when the first leg starts."""
    a = torch.randn((4096, 4096), device="cuda")
    for _ in range(40):
        a = (a @ a).clamp_(-1, 1)
    torch.cuda.synchronize()


def leg(name, p, nb, T, L, nfft, hop, steps, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((nb, T), device="cuda", generator=g) + 3.0
    F = 1 + (T - L) // hop
    K = nfft // 2 + 1
    scale = 0.5
    pow2 = nfft & (nfft - 1) == 0
    rec = {"leg": name, "family": "fft" if pow2 else "mfft", "B": nb, "T": T, "L": L, "nfft": nfft, "hop": hop, "frames": F}
    s = B.make_stft(nb, T, F, hop, nfft, shift=p.dat_width - 1)
    kw = dict(win_length=L, center=False, detrend=True)
    ws_bytes, describe = (B.hold_fft_workspace_bytes, B.describe_hold_fft) if pow2 else (B.hold_mfft_workspace_bytes, B.describe_hold_mfft)
    with bhw.ResidentTable(p) as t:
        hold_t, hold_l, spectro, welch = ((t.hold_fft, bhw.hold_fft, t.spectrogram, t.welch_fft) if pow2 else
                                          (t.hold_fft_mixed, bhw.hold_fft_mixed, t.spectrogram_mixed, t.welch_fft_mixed))
        S = torch.empty((nb, F, K), dtype=torch.float32, device="cuda")
        om, on, P = (torch.empty((nb, K), device="cuda") for _ in range(3))
        cm, cn = torch.empty((nb, K), device="cuda"), torch.empty((nb, K), device="cuda")
        ws = torch.empty(ws_bytes(s) // 8, dtype=torch.float64, device="cuda")

        def three_call():
            rows = spectro(p, x, nfft, hop, out=S, **kw)
            torch.amax(rows, dim=-2, out=cm)
            torch.amin(rows, dim=-2, out=cn)
            return cm, cn

        fns = {"a_hold_table": lambda: hold_t(p, x, nfft, hop, scale, out_max=om, out_min=on, workspace=ws, **kw),
               "b_hold_library": lambda: hold_l(p, x, nfft, hop, scale, out_max=om, out_min=on, workspace=ws, **kw),
               "c_spectrogram_amax_amin": three_call,
               "d_spectrogram_alone": lambda: spectro(p, x, nfft, hop, out=S, **kw),
               "e_welch_fft": lambda: welch(p, x, nfft, hop, scale, out=P, workspace=ws, **kw)}
        r = timed(fns, steps, reps)
        m = {k: v["median_ms"] for k, v in r.items()}
        c = r["c_spectrogram_amax_amin"]
        spread = (c["max_ms"] - c["min_ms"]) / c["median_ms"]
        ratio = m["a_hold_table"] / m["c_spectrogram_amax_amin"]
        rec["plan"] = describe(p, L, s, detrend=True, table=t.handle)
        rec.update({"times": r, "bytes_in": nb * T * 4, "bytes_powers": nb * F * K * 4, "bytes_workspace": int(ws.numel()) * 8,
                    "bytes_out": 2 * nb * K * 4, "a_over_c": ratio, "c_spread": spread,
                    "aim": "met" if ratio < 1.0 - spread else "missed" if ratio > 1.0 + spread else "within (c)'s spread",
                    "a_over_b": m["a_hold_table"] / m["b_hold_library"],
                    "a_over_d": m["a_hold_table"] / m["d_spectrogram_alone"],
                    "a_over_e": m["a_hold_table"] / m["e_welch_fft"]})
        # the same words: (a) against (c) on the benchmarked data, at the factor of the timed calls (every bin but 0 and M doubled)
        am, an = hold_t(p, x, nfft, hop, scale, **kw)
        rm, rn = three_call()
        lm, ln = hold_l(p, x, nfft, hop, scale, **kw)
        sk = torch.full((K,), scale, dtype=torch.float64, device="cuda")
        sk[1:K - 1] = scale * 2.0
        torch.cuda.synchronize()
        rec["agreement"] = {"max_equal": bool(torch.equal(am, (rm.double() * sk).float())),
                            "min_equal": bool(torch.equal(an, (rn.double() * sk).float())),
                            "library_equals_table": bool(torch.equal(am, lm) and torch.equal(an, ln))}
    return rec


def resources():
    path = os.path.join(ROOT, "blackman_harris_win_amd", "kernel_resources.json")
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        res = json.load(f)
    out = {}
    for k, v in res.items():
        if k.startswith(("k_hold_", "k_welch_fft", "k_welch_mfft", "k_spectrogram", "k_stft_mfft")):
            key = json.dumps({"family": k.split("<")[0] if "join" not in k else k,
                              **{n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy", "LDS Size")}},
                             sort_keys=True)
            out.setdefault(key, []).append(k)
    return [{"figures": json.loads(k), "instances": len(v), "example": v[0]} for k, v in out.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_hold_real.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written (a profiler run)")
    ap.add_argument("--legs", default="T1,T1M,T2,T3,N64,N96,ONE,ONEM")
    a = ap.parse_args()
    steps, reps = (2, 3) if a.quick else (a.steps, a.reps)
    ramp()
    rec = {"device": torch.cuda.get_device_name(0), "steps": steps, "reps": reps, "legs": [], "kernel_resources": resources()}
    for name, (p, nb, T, L, nfft, hop) in legs().items():
        if name not in a.legs.split(","):
            continue
        rec["legs"].append(leg(name, p, nb, T, L, nfft, hop, steps, reps))
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec))
    if not a.quick:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
