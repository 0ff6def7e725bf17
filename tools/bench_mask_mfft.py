#!/usr/bin/env python3
"""The mixed-radix fused STFT + mask + inverse STFT kernel (bhw_mask_mfft_f32_* / bhw.stft_mask_istft_mixed) on one GPU.  Prints one JSON
record and writes it to --out (profiles/r42_mask_mfft.json by default).  The protocol, the variants and the record are those of
tools/bench_mask_fft.py, whose timing loop and float64 reference it imports.

Legs, centred, reflect padding, length = T, L = nfft:
  S400 speech   BH-4, P 24, 32 b; B 64, T 160 000, 400 / 400 / 160 (1 001 frames per signal, 201 bins)
  A960 audio    BH-4, P 24, 32 b; B 64, T 160 000, 960 / 960 / 480 (334 frames per signal, 481 bins)
  L2000 long    BH-7, P 12, 32 b; B 1, T 2^24, 2000 / 2000 / 500 (33 555 frames)
  N96 short     BH-4, P 24, 32 b; B 64, T 160 000, 96 / 96 / 48 (3 334 frames per signal)
Variants, all from one resident table, outputs preallocated:
  (a) the fused call with full (B, F, K) gains          (b) the fused call with one (K,) gain row
  (c) stft_mixed + a torch multiply + istft_mixed (the route it replaces)   (d) stft_mixed + istft_mixed alone
  (e) a plain copy of (a)'s bytes: read B * T * 4 + B * F * K * 4, write B * T * 4 (one copy_ of half that many bytes each way)
The protocol of tools/bench_istft_fft.py: a clock ramp, every variant warmed, --steps steps of --reps back-to-back calls between
device events, the variants of a leg alternated step by step, medians.  The aim -- (a) and (b) below (c), judged outside (c)'s own
spread (max - min) / median of its step medians -- is reported, met or missed, not asserted.  What IS asserted, on the timed data of
every leg: the fused output equals (c) word for word (a leg that misses fails).  The end-to-end errors of the fused call and of
torch.istft(torch.stft(x) * g) against numpy in float64 are recorded on a short signal of each leg's shape.

Each leg runs in a child process of its own under a time limit (--leg-timeout seconds); a leg that fails or runs out of time is
recorded as such and the legs after it are not started.

    python tools/bench_mask_mfft.py [--steps 10] [--reps 20] [--out FILE] [--quick]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mask_fft import ref64, timed  # noqa: E402

LEGS = {"S400": ("bh4", 24, 64, 160000, 400, 400, 160), "A960": ("bh4", 24, 64, 160000, 960, 960, 480),
        "L2000": ("bh7", 12, 1, 1 << 24, 2000, 2000, 500), "N96": ("bh4", 24, 64, 160000, 96, 96, 48)}


def run_leg(name, steps, reps):
    import numpy as np
    import torch
    import blackman_harris_win_amd as bhw
    from blackman_harris_win_amd import binding as B
    win, pw, nb, T, L, nfft, hop = LEGS[name]
    p = B.make_params(B.WIN_BH4 if win == "bh4" else B.WIN_BH7, pw, 32)
    a = torch.randn((4096, 4096), device="cuda")                        # the clock ramp: a second of work in front of the timed region
    for _ in range(40):
        a = (a @ a).clamp_(-1, 1)
    torch.cuda.synchronize()
    del a
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((nb, T), device="cuda", generator=g) + 3.0
    K, pad, col0 = nfft // 2 + 1, nfft // 2, (nfft - L) // 2
    F = 1 + T // hop
    gains = torch.rand((nb, F, K), device="cuda", generator=g) * 2.0
    row = gains[0, 0].contiguous()
    kw = dict(win_length=L, length=T)
    rec = {"leg": name, "B": nb, "T": T, "L": L, "nfft": nfft, "hop": hop, "frames": F, "bins": K}
    with bhw.ResidentTable(p) as t:
        Y = t.stft_mixed(p, x, nfft, hop, win_length=L)
        assert tuple(Y.shape) == (nb, F, K)
        Yr = torch.view_as_real(Y)
        out = torch.empty((nb, T), device="cuda")
        g4 = gains[..., None]
        bytes_in, bytes_out = nb * T * 4 + nb * F * K * 4, nb * T * 4
        half = (bytes_in + bytes_out) // 2 // 4
        src, dst = torch.empty(half, device="cuda"), torch.empty(half, device="cuda")

        def three_calls():
            t.stft_mixed(p, x, nfft, hop, win_length=L, out=Y)
            Yr.mul_(g4)
            t.istft_mixed(p, Y, nfft, hop, out=out, **kw)

        def two_calls():
            t.stft_mixed(p, x, nfft, hop, win_length=L, out=Y)
            t.istft_mixed(p, Y, nfft, hop, out=out, **kw)

        r = timed(torch, {"a_fused_full_gains": lambda: bhw.stft_mask_istft_mixed(p, x, gains, nfft, hop, out=out, table=t, **kw),
                          "b_fused_one_gain_row": lambda: bhw.stft_mask_istft_mixed(p, x, row, nfft, hop, out=out, table=t, **kw),
                          "c_stft_multiply_istft": three_calls,
                          "d_stft_istft": two_calls,
                          "e_copy_of_its_bytes": lambda: dst.copy_(src)}, steps, reps)
        sa = B.make_stft(nb, T, F, hop, nfft, col0=col0, pad=pad, pad_mode=B.PAD_REFLECT, shift=p.dat_width - 1)
        ss = B.make_stft(nb, T, F, hop, nfft, col0=col0, pad=pad, shift=p.dat_width - 1)
        rec["plan"] = B.describe_mask_mfft(p, L, sa, ss, normalize=True, g_stride=K, g_batch_stride=F * K, table=t.handle)
        m = {k: v["median_ms"] for k, v in r.items()}
        c = r["c_stft_multiply_istft"]
        spread = (c["max_ms"] - c["min_ms"]) / c["median_ms"]
        rec.update({"times": r, "bytes_in": bytes_in, "bytes_out": bytes_out, "bytes_of_the_spectrum_the_three_calls_move": 4 * nb * F * K * 8,
                    "a_over_c": m["a_fused_full_gains"] / m["c_stft_multiply_istft"], "b_over_c": m["b_fused_one_gain_row"] / m["c_stft_multiply_istft"],
                    "a_over_d": m["a_fused_full_gains"] / m["d_stft_istft"], "a_over_copy": m["a_fused_full_gains"] / m["e_copy_of_its_bytes"],
                    "spread_of_c": spread,
                    "aim_a_below_c": m["a_fused_full_gains"] < m["c_stft_multiply_istft"] * (1.0 - spread),
                    "aim_b_below_c": m["b_fused_one_gain_row"] < m["c_stft_multiply_istft"] * (1.0 - spread),
                    "a_GBps": (bytes_in + bytes_out) / m["a_fused_full_gains"] / 1e6})
        del src, dst
        # the fused call is the three calls word for word, on the timed data
        three_calls()
        want = out.clone()
        got = bhw.stft_mask_istft_mixed(p, x, gains, nfft, hop, table=t, **kw)
        rec["word_for_word_the_three_calls"] = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
        assert rec["word_for_word_the_three_calls"], f"leg {name}: the fused output is not the three calls' word for word"
        # accuracy on two signals of at most 400 frames of the leg's shape
        Fa = min(F, 400)
        Ta = hop * (Fa - 1)
        xa, ga = x[:min(nb, 2), :Ta].contiguous(), gains[:min(nb, 2), :Fa].contiguous()
        v = bhw.window(p, L, dtype=torch.float32)
        fused = bhw.stft_mask_istft_mixed(p, xa, ga, nfft, hop, win_length=L, length=Ta, table=t)
        St = torch.stft(xa, nfft, hop, L, window=v, center=True, pad_mode="reflect", return_complex=True)
        yard = torch.istft(St * ga.transpose(-1, -2), nfft, hop, L, window=v, center=True, length=Ta)
        ref = ref64(np, xa.cpu().numpy(), ga.cpu().numpy().astype(np.float64), v.cpu().numpy(), nfft, hop, L, Ta)
        e_f = float(np.abs(fused.cpu().numpy().astype(np.float64) - ref).max())
        e_t = float(np.abs(yard.cpu().numpy().astype(np.float64) - ref).max())
        rec["accuracy"] = {"frames": Fa, "fused_max_abs": e_f, "torch_max_abs": e_t, "ratio": e_f / e_t, "bound": 2.0, "met": e_f <= 2.0 * e_t}
        rec["device"] = torch.cuda.get_device_name(0)
    return rec


def resources():
    path = os.path.join(ROOT, "blackman_harris_win_amd", "kernel_resources.json")
    if not os.path.exists(path):
        return []
    with open(path) as f:
        res = json.load(f)
    out = {}
    for k, v in res.items():
        if k.startswith(("k_mask_mfft", "k_istft_mfft")):
            key = json.dumps({"family": k.split("_direct")[0].split("_table")[0],
                              **{n: v.get(n) for n in ("VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy")}}, sort_keys=True)
            out.setdefault(key, []).append(k)
    return [{"figures": json.loads(k), "instances": len(v), "example": v[0]} for k, v in out.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r42_mask_mfft.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written")
    ap.add_argument("--leg", default=None, help="(internal) run one leg in this process and print its record")
    ap.add_argument("--leg-timeout", type=int, default=240)
    a = ap.parse_args()
    steps, reps = (2, 3) if a.quick else (a.steps, a.reps)
    if a.leg:
        print(json.dumps(run_leg(a.leg, steps, reps)))
        return 0
    rec = {"steps": steps, "reps": reps, "legs": [], "kernel_resources": resources()}
    for name in LEGS:
        cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", name, "--steps", str(steps),
               "--reps", str(reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            rec["legs"].append({"leg": name, "failed": r.returncode, "stderr": r.stderr[-1000:]})
            break                                                        # nothing more is started on the GPU after a failed step
        rec["legs"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(rec))
    if not a.quick:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0 if all("failed" not in leg for leg in rec["legs"]) else 1


if __name__ == "__main__":
    sys.exit(main())
