#!/usr/bin/env python3
"""The fused Welch PSD for I/Q input at a mixed-radix n_fft (bhw_welch_cmfft_f32_* / bhw.welch_fft_iq_mixed) on one GPU, one process.
Prints one JSON record and writes it to --out (profiles/r29_welch_iq_mixed.json by default).  The protocol is tools/bench_welch_iq.py's.

Legs, complex64 input, L = nfft:
  T1 batch   BH-4, P 24, 32 b; B 64, T 160 000, 400 / hop 160 (998 segments per signal): section 21's batch
  T2 long    BH-7, P 12, 32 b; B 1, T 2^24, 2000 / hop 500 (33 551 segments)
  T3 long    BH-7, P 12, 32 b; B 1, T 2^24, 1536 / hop 384 (43 687 segments)
  N96 short  BH-4, P 24, 32 b; B 64, T 160 000, 96 / hop 48 (3 332 segments per signal)
  ONE block  BH-4, P 24, 32 b; B 64, 200 segments of 400 / hop 160
Variants, detrended segments, every output and workspace given, one resident table:
  (a) welch_fft_iq_mixed from the table     (b) welch_fft_iq_mixed, the library form
  (c) stft_iq_mixed + welch_psd(onesided=False), the route (a) replaces, from the same table
  (d) stft_iq_mixed alone                   (e) welch_frames + torch.fft.fft + welch_psd
The aim: (a) below (c) on every leg.  A leg counts as met or missed only beyond (c)'s own spread in the record, (max - min) / median of
its step medians; it is no test gate.  Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events,
the variants of a leg alternated step by step, after a clock ramp; times are per call (median, min, max over --steps).  The record also
holds the agreement of (a) with (c) in float32 ulps on the benchmarked data, and the compiler's figures for the kernels.

    python tools/bench_welch_iq_mixed.py [--steps 10] [--reps 20] [--out FILE] [--quick] [--legs T1,T2]
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
    return {"T1": (bh4, 64, 160000, 400, 400, 160),
            "T2": (bh7, 1, 1 << 24, 2000, 2000, 500),
            "T3": (bh7, 1, 1 << 24, 1536, 1536, 384),
            "N96": (bh4, 64, 160000, 96, 96, 48),
            "ONE": (bh4, 64, 199 * 160 + 400, 400, 400, 160)}


def ramp():
    """A second of work in front of the timed region: the clock has ramped when the first leg starts."""
    a = torch.randn((4096, 4096), device="cuda")
    for _ in range(40):
        a = (a @ a).clamp_(-1, 1)
    torch.cuda.synchronize()


def leg(name, p, nb, T, L, nfft, hop, steps, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((nb, T, 2), device="cuda", generator=g) + 3.0)
    F = 1 + (T - L) // hop
    scale = 1.0 / F
    rec = {"leg": name, "B": nb, "T": T, "L": L, "nfft": nfft, "hop": hop, "frames": F}
    s = B.make_stft(nb, T, F, hop, nfft, channels=2, shift=p.dat_width - 1)
    kw = dict(win_length=L, center=False, detrend=True)
    with bhw.ResidentTable(p) as t:
        Y = torch.empty((nb, F, nfft), dtype=torch.complex64, device="cuda")
        seg = torch.empty((nb, F, nfft), dtype=torch.complex64, device="cuda")
        mean = torch.empty(nb * F * 2, device="cuda")
        P, P2 = torch.empty((nb, nfft), device="cuda"), torch.empty((nb, nfft), device="cuda")
        ws = torch.empty(B.welch_cmfft_workspace_bytes(s) // 8, dtype=torch.float64, device="cuda")
        pws = torch.empty(max(1, nb * (-(-F // 256)) * nfft), dtype=torch.float64, device="cuda")
        psd_ws = pws if F > 256 else None

        def two_call():
            return bhw.welch_psd(t.stft_iq_mixed(p, x, nfft, hop, out=Y, **kw), scale, nfft=nfft, onesided=False, out=P2, workspace=psd_ws)

        def torch_route():
            yy = torch.fft.fft(t.welch_frames(p, x, L, hop, nfft=nfft, out=seg, workspace=mean), dim=-1)
            return bhw.welch_psd(yy, scale, nfft=nfft, onesided=False, out=P2, workspace=psd_ws)

        fns = {"a_welch_fft_iq_mixed_table": lambda: t.welch_fft_iq_mixed(p, x, nfft, hop, scale, out=P, workspace=ws, **kw),
               "b_welch_fft_iq_mixed_library": lambda: bhw.welch_fft_iq_mixed(p, x, nfft, hop, scale, out=P, workspace=ws, **kw),
               "c_stft_iq_mixed_plus_welch_psd": two_call,
               "d_stft_iq_mixed_alone": lambda: t.stft_iq_mixed(p, x, nfft, hop, out=Y, **kw),
               "e_frames_fft_welch_psd": torch_route}
        r = timed(fns, steps, reps)
        m = {k: v["median_ms"] for k, v in r.items()}
        c = r["c_stft_iq_mixed_plus_welch_psd"]
        spread = (c["max_ms"] - c["min_ms"]) / c["median_ms"]
        ratio = m["a_welch_fft_iq_mixed_table"] / m["c_stft_iq_mixed_plus_welch_psd"]
        rec["plan"] = B.describe_welch_cmfft(p, L, s, detrend=True, table=t.handle)
        rec.update({"times": r, "bytes_in": nb * T * 8, "bytes_spectrum": nb * F * nfft * 8, "bytes_workspace": int(ws.numel()) * 8,
                    "bytes_out": nb * nfft * 4, "a_over_c": ratio, "c_spread": spread,
                    "aim": "met" if ratio < 1.0 - spread else "missed" if ratio > 1.0 + spread else "within (c)'s spread",
                    "a_over_b": m["a_welch_fft_iq_mixed_table"] / m["b_welch_fft_iq_mixed_library"],
                    "a_over_d": m["a_welch_fft_iq_mixed_table"] / m["d_stft_iq_mixed_alone"],
                    "a_over_e": m["a_welch_fft_iq_mixed_table"] / m["e_frames_fft_welch_psd"]})
        # the same numbers: (a) against (c) on the benchmarked data
        Pa = t.welch_fft_iq_mixed(p, x, nfft, hop, scale, **kw)
        Pc = two_call()
        torch.cuda.synchronize()
        ulps = int((Pa.view(torch.int32).long() - Pc.view(torch.int32).long()).abs().max())
        rec["agreement"] = {"max_ulps_a_against_c": ulps, "bound": 1, "met": ulps <= 1,
                            "library_equals_table": bool(torch.equal(Pa, bhw.welch_fft_iq_mixed(p, x, nfft, hop, scale, **kw)))}
    return rec


def resources():
    path = os.path.join(ROOT, "blackman_harris_win_amd", "kernel_resources.json")
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        res = json.load(f)
    out = {}
    for k, v in res.items():
        if k.startswith("k_welch_cmfft") or k.startswith("k_stft_cmfft") or k.startswith("k_welch_fft_join"):
            key = json.dumps({"family": k.split("<")[0] if "join" not in k else k,
                              **{n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy", "LDS Size")}},
                             sort_keys=True)
            out.setdefault(key, []).append(k)
    return [{"figures": json.loads(k), "instances": len(v), "example": v[0]} for k, v in out.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_welch_iq_mixed.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written (a profiler run)")
    ap.add_argument("--legs", default="T1,T2,T3,N96,ONE")
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
