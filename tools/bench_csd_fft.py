#!/usr/bin/env python3
"""The fused Welch cross spectra (bhw_csd_fft_f32_* / bhw.csd_fft / bhw.cross_spectra_fused) on one GPU, one process.  Prints one JSON
record and writes it to --out (profiles/r25_csd_fft.json by default).

Legs, section 26's with the long record at the largest n_fft this call takes:
  T1 batch   BH-4, P 24, 32 b; B 64, T 160 000, L 400 in rows of 512, hop 160 (998 segments per signal)
  T2 long    BH-7, P 12, 32 b; B 1, T 2^24, L = nfft 2048, hop 512 (32 765 segments)
  N64 short  BH-4, P 24, 32 b; B 64, T 160 000, L = nfft 64, hop 32 (4 999 segments per signal)
  ONE block  BH-4, P 24, 32 b; B 64, 200 segments of L 400 in rows of 512, hop 160
  T1B        T1 with ONE x broadcast against the 64 signals of y
Variants, detrended segments, every output and workspace given:
  (a) csd_fft from a table, the full mask, and (a1) with pxy alone
  (b) csd_fft, the library form, the full mask
  (c) stft(x) + stft(y) + welch_csd from the same table, the full mask: the parent's route, the yardstick
  (d) the two stft calls alone
  (e) cross_spectra(fft="torch"), end to end (it allocates its segments and spectra)
The aim: (a) below (c) on every leg.  Each leg is reported as met, missed, or inside (c)'s own spread, (max - min) / median of its step
medians; it is no test gate.  Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events, the
variants of a leg alternated step by step, after a clock ramp; times are per call (median, min, max over --steps).  Under broadcast
the kernel transforms x once per response, (c) once: the record says what that costs.  The record also holds the agreement of (a) with
(c) on the benchmarked data and the compiler's figures for the new kernels.

    python tools/bench_csd_fft.py [--steps 10] [--reps 20] [--out FILE] [--quick] [--legs T1,T2]
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

ALL = ("pxy", "pxx", "pyy", "coherence", "h1")


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
    return {"T1": (bh4, 64, 160000, 400, 512, 160, False),
            "T2": (B.make_params(B.WIN_BH7, 12, 32), 1, 1 << 24, 2048, 2048, 512, False),
            "N64": (bh4, 64, 160000, 64, 64, 32, False),
            "ONE": (bh4, 64, 199 * 160 + 400, 400, 512, 160, False),
            "T1B": (bh4, 64, 160000, 400, 512, 160, True)}


def ramp():
    """A second of work in front of the timed region: the clock has ramped when the first leg starts."""
    a = torch.randn((4096, 4096), device="cuda")
    for _ in range(40):
        a = (a @ a).clamp_(-1, 1)
    torch.cuda.synchronize()


def leg(name, p, nb, T, L, nfft, hop, bcast, steps, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    y = torch.randn((nb, T), device="cuda", generator=g) + 3.0
    x = torch.randn((T,) if bcast else (nb, T), device="cuda", generator=g) + 0.25 * (y[0] if bcast else y)
    F = 1 + (T - L) // hop
    K = nfft // 2 + 1
    nx = 1 if bcast else nb
    scale = 1.0 / F
    rec = {"leg": name, "B": nb, "T": T, "L": L, "nfft": nfft, "hop": hop, "frames": F, "broadcast_x": bcast}
    s = B.make_stft(nb, T, F, hop, nfft, shift=p.dat_width - 1)
    kw = dict(win_length=L, center=False, detrend=True)
    with bhw.ResidentTable(p) as t:
        SX = torch.empty((F, K) if bcast else (nb, F, K), dtype=torch.complex64, device="cuda")
        SY = torch.empty((nb, F, K), dtype=torch.complex64, device="cuda")
        mk = lambda: {n: torch.empty((nb, K), dtype=torch.complex64 if B.CSD_OUTPUTS[n][1] else torch.float32, device="cuda") for n in ALL}
        o_a, o_c = mk(), mk()
        ws = torch.empty(B.csd_fft_workspace_bytes(s) // 8, dtype=torch.float64, device="cuda")
        cws = torch.empty(max(1, nb * (-(-F // 256)) * K * 4), dtype=torch.float64, device="cuda")
        csd_ws = cws if F > 256 else None

        def two_stft():
            t.stft(p, x, nfft, hop, out=SX, **kw)
            t.stft(p, y, nfft, hop, out=SY, **kw)

        def parent_route():
            two_stft()
            return bhw.welch_csd(SX, SY, scale, nfft=nfft, outputs=ALL, out=o_c, workspace=csd_ws)

        fns = {"a_csd_fft_table_full": lambda: t.csd_fft(p, x, y, nfft, hop, scale, outputs=ALL, out=o_a, workspace=ws, **kw),
               "a1_csd_fft_table_pxy": lambda: t.csd_fft(p, x, y, nfft, hop, scale, outputs=("pxy",), out={"pxy": o_a["pxy"]}, workspace=ws, **kw),
               "b_csd_fft_library_full": lambda: bhw.csd_fft(p, x, y, nfft, hop, scale, outputs=ALL, out=o_a, workspace=ws, **kw),
               "c_two_stft_plus_welch_csd": parent_route,
               "d_two_stft_alone": two_stft}
        r = timed(fns, steps, reps)
        t.cross_spectra(p, x, y, length=L, noverlap=L - hop, nfft=nfft)               # the warm call reads the window sums
        r.update(timed({"e_cross_spectra_torch": lambda: t.cross_spectra(p, x, y, length=L, noverlap=L - hop, nfft=nfft)}, steps, reps))
        m = {k: v["median_ms"] for k, v in r.items()}
        c = r["c_two_stft_plus_welch_csd"]
        spread = (c["max_ms"] - c["min_ms"]) / c["median_ms"]
        ratio = m["a_csd_fft_table_full"] / m["c_two_stft_plus_welch_csd"]
        verdict = "inside (c)'s spread" if abs(ratio - 1.0) <= spread else "met" if ratio < 1.0 else "missed"
        rec["plan"] = B.describe_csd_fft(p, L, s, detrend=True, outputs=ALL, broadcast_x=bcast, table=t.handle)
        rec.update({"times": r, "bytes_in": (nb + nx) * T * 4, "bytes_spectra": (nb + nx) * F * K * 8, "bytes_workspace": int(ws.numel()) * 8,
                    "bytes_out": nb * K * 4 * 7, "a_over_c": ratio, "c_spread": spread, "verdict": verdict,
                    "a1_over_c": m["a1_csd_fft_table_pxy"] / m["c_two_stft_plus_welch_csd"],
                    "b_over_a": m["b_csd_fft_library_full"] / m["a_csd_fft_table_full"],
                    "a_over_d": m["a_csd_fft_table_full"] / m["d_two_stft_alone"],
                    "a_over_e": m["a_csd_fft_table_full"] / m["e_cross_spectra_torch"]})
        if bcast:
            rec["broadcast_note"] = ("the fused kernel transforms x once per response (2 * B transforms), (c) transforms it once (B + 1): "
                                     "a_over_c of this leg against the T1 leg's is what that costs")
        # the same numbers: (a) against (c) on the benchmarked data
        ga = t.csd_fft(p, x, y, nfft, hop, scale, outputs=ALL, **kw)
        gc = parent_route()
        torch.cuda.synchronize()
        same = lambda u, v: bool(torch.equal(torch.view_as_real(u) if u.is_complex() else u, torch.view_as_real(v) if v.is_complex() else v))
        top = float(gc["pxy"].abs().max())
        lib = bhw.csd_fft(p, x, y, nfft, hop, scale, outputs=ALL, **kw)
        rec["agreement"] = {"pxy_max_abs_diff_over_max": float((ga["pxy"] - gc["pxy"]).abs().max()) / top,
                            "coherence_max_abs_diff": float((ga["coherence"] - gc["coherence"]).abs().max()),
                            "pxx_max_ulps": int((ga["pxx"].view(torch.int32).long() - gc["pxx"].view(torch.int32).long()).abs().max()),
                            "library_equals_table": all(same(ga[n], lib[n]) for n in ALL)}
    return rec


def resources():
    path = os.path.join(ROOT, "blackman_harris_win_amd", "kernel_resources.json")
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        res = json.load(f)
    out = {}
    for k, v in res.items():
        if k.startswith("k_csd_fft") or k.startswith("k_welch_fft_direct") or k.startswith("k_welch_fft_table"):
            key = json.dumps({"family": k.split("<")[0],
                              **{n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy", "LDS Size")}},
                             sort_keys=True)
            out.setdefault(key, []).append(k)
    return [{"figures": json.loads(k), "instances": len(v), "example": v[0]} for k, v in out.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_csd_fft.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written (a profiler run)")
    ap.add_argument("--legs", default="T1,T2,N64,ONE,T1B")
    a = ap.parse_args()
    steps, reps = (2, 3) if a.quick else (a.steps, a.reps)
    ramp()
    rec = {"device": torch.cuda.get_device_name(0), "steps": steps, "reps": reps, "legs": [], "kernel_resources": resources()}
    for name, (p, nb, T, L, nfft, hop, bcast) in legs().items():
        if name not in a.legs.split(","):
            continue
        rec["legs"].append(leg(name, p, nb, T, L, nfft, hop, bcast, steps, reps))
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec))
    if not a.quick:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
