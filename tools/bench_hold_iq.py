#!/usr/bin/env python3
"""The fused max-hold / min-hold traces for I/Q input (bhw_hold_cfft_f32_* / bhw_hold_cmfft_f32_*; bhw.hold_fft_iq, hold_fft_iq_mixed)
on one GPU, one process.  Prints one JSON record and writes it to --out (profiles/r30_hold_iq.json by default).  The protocol is
tools/bench_welch_iq_mixed.py's.

Legs, complex64 input, L = nfft: DESIGN.md section 32's five at the mixed-radix sizes, and section 27's long leg at a power of two:
  T1 batch   BH-4, P 24, 32 b; B 64, T 160 000, 400 / hop 160 (998 segments per signal)
  T2 long    BH-7, P 12, 32 b; B 1, T 2^24, 2000 / hop 500 (33 551 segments)
  T3 long    BH-7, P 12, 32 b; B 1, T 2^24, 1536 / hop 384 (43 687 segments)
  N96 short  BH-4, P 24, 32 b; B 64, T 160 000, 96 / hop 48 (3 332 segments per signal)
  ONE block  BH-4, P 24, 32 b; B 64, 200 segments of 400 / hop 160
  P2 long    BH-7, P 12, 32 b; B 1, T 2^24, 2048 / hop 512 (32 765 segments), the power-of-two family
Variants, detrended segments, every output and workspace given, one resident table:
  (a) hold_fft_iq(_mixed) from the table, both traces      (b) hold_fft_iq(_mixed), the library form
  (c) spectrogram_iq(_mixed) + amax + amin over the frames, the route (a) replaces, from the same table
  (d) spectrogram_iq(_mixed) alone                         (e) welch_fft_iq(_mixed), the mean of the same frames
The aim: (a) below (c) on every leg.  A leg counts as met or missed only beyond (c)'s own spread in the record, (max - min) / median of
its step medians; it is no test gate.  Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events,
the variants of a leg alternated step by step, after a clock ramp; times are per call (median, min, max over --steps).  The record also
holds the equality of (a) with (c) on the benchmarked data (the contract is exact), and the compiler's figures for the kernels.

    python tools/bench_hold_iq.py [--steps 10] [--reps 20] [--out FILE] [--quick] [--legs T1,T2]
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
    return {"T1": (bh4, 64, 160000, 400, 160),
            "T2": (bh7, 1, 1 << 24, 2000, 500),
            "T3": (bh7, 1, 1 << 24, 1536, 384),
            "N96": (bh4, 64, 160000, 96, 48),
            "ONE": (bh4, 64, 199 * 160 + 400, 400, 160),
            "P2": (bh7, 1, 1 << 24, 2048, 512)}


def ramp():
    """A second of work in front of the timed region: the clock has ramped when the first leg starts."""
    a = torch.randn((4096, 4096), device="cuda")
    for _ in range(40):
        a = (a @ a).clamp_(-1, 1)
    torch.cuda.synchronize()


def leg(name, p, nb, T, nfft, hop, steps, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((nb, T, 2), device="cuda", generator=g) + 3.0)
    L = nfft
    F = 1 + (T - L) // hop
    scale = 0.5
    pow2 = nfft & (nfft - 1) == 0
    rec = {"leg": name, "family": "cfft" if pow2 else "cmfft", "B": nb, "T": T, "L": L, "nfft": nfft, "hop": hop, "frames": F}
    s = B.make_stft(nb, T, F, hop, nfft, channels=2, shift=p.dat_width - 1)
    kw = dict(win_length=L, center=False, detrend=True)
    ws_bytes, describe = (B.hold_cfft_workspace_bytes, B.describe_hold_cfft) if pow2 else (B.hold_cmfft_workspace_bytes, B.describe_hold_cmfft)
    with bhw.ResidentTable(p) as t:
        hold_t, hold_l, spectro, welch = ((t.hold_fft_iq, bhw.hold_fft_iq, t.spectrogram_iq, t.welch_fft_iq) if pow2 else
                                          (t.hold_fft_iq_mixed, bhw.hold_fft_iq_mixed, t.spectrogram_iq_mixed, t.welch_fft_iq_mixed))
        S = torch.empty((nb, F, nfft), dtype=torch.float32, device="cuda")
        om, on, P = (torch.empty((nb, nfft), device="cuda") for _ in range(3))
        cm, cn = torch.empty((nb, nfft), device="cuda"), torch.empty((nb, nfft), device="cuda")
        ws = torch.empty(ws_bytes(s) // 8, dtype=torch.float64, device="cuda")

        def two_call():
            rows = spectro(p, x, nfft, hop, out=S, **kw)
            torch.amax(rows, dim=-2, out=cm)
            torch.amin(rows, dim=-2, out=cn)
            return cm, cn

        fns = {"a_hold_table": lambda: hold_t(p, x, nfft, hop, scale, out_max=om, out_min=on, workspace=ws, **kw),
               "b_hold_library": lambda: hold_l(p, x, nfft, hop, scale, out_max=om, out_min=on, workspace=ws, **kw),
               "c_spectrogram_amax_amin": two_call,
               "d_spectrogram_alone": lambda: spectro(p, x, nfft, hop, out=S, **kw),
               "e_welch_fft_iq": lambda: welch(p, x, nfft, hop, scale, out=P, workspace=ws, **kw)}
        r = timed(fns, steps, reps)
        m = {k: v["median_ms"] for k, v in r.items()}
        c = r["c_spectrogram_amax_amin"]
        spread = (c["max_ms"] - c["min_ms"]) / c["median_ms"]
        ratio = m["a_hold_table"] / m["c_spectrogram_amax_amin"]
        rec["plan"] = describe(p, L, s, detrend=True, table=t.handle)
        rec.update({"times": r, "bytes_in": nb * T * 8, "bytes_powers": nb * F * nfft * 4, "bytes_workspace": int(ws.numel()) * 8,
                    "bytes_out": 2 * nb * nfft * 4, "a_over_c": ratio, "c_spread": spread,
                    "aim": "met" if ratio < 1.0 - spread else "missed" if ratio > 1.0 + spread else "within (c)'s spread",
                    "a_over_b": m["a_hold_table"] / m["b_hold_library"],
                    "a_over_d": m["a_hold_table"] / m["d_spectrogram_alone"],
                    "a_over_e": m["a_hold_table"] / m["e_welch_fft_iq"]})
        # the same words: (a) against (c) on the benchmarked data, at the scale of the timed calls
        am, an = hold_t(p, x, nfft, hop, scale, **kw)
        rm, rn = two_call()
        lm, ln = hold_l(p, x, nfft, hop, scale, **kw)
        torch.cuda.synchronize()
        rec["agreement"] = {"max_equal": bool(torch.equal(am, (rm.double() * scale).float())),
                            "min_equal": bool(torch.equal(an, (rn.double() * scale).float())),
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
        if k.startswith(("k_hold_", "k_welch_cfft", "k_welch_cmfft", "k_stft_cfft", "k_stft_cmfft")):
            key = json.dumps({"family": k.split("<")[0] if "join" not in k else k,
                              **{n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy", "LDS Size")}},
                             sort_keys=True)
            out.setdefault(key, []).append(k)
    return [{"figures": json.loads(k), "instances": len(v), "example": v[0]} for k, v in out.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_hold_iq.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written (a profiler run)")
    ap.add_argument("--legs", default="T1,T2,T3,N96,ONE,P2")
    a = ap.parse_args()
    steps, reps = (2, 3) if a.quick else (a.steps, a.reps)
    ramp()
    rec = {"device": torch.cuda.get_device_name(0), "steps": steps, "reps": reps, "legs": [], "kernel_resources": resources()}
    for name, (p, nb, T, nfft, hop) in legs().items():
        if name not in a.legs.split(","):
            continue
        rec["legs"].append(leg(name, p, nb, T, nfft, hop, steps, reps))
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec))
    if not a.quick:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
