#!/usr/bin/env python3
"""The fused STFT + complex gain + inverse STFT kernels of both families (bhw_cmask_fft_f32_* / bhw_cmask_mfft_f32_*, through
bhw.stft_cmask_istft / bhw.stft_cmask_istft_mixed) on one GPU.  Prints one JSON record and writes it to --out
(profiles/r43_cmask.json by default).  The protocol is that of tools/bench_mask_fft.py and tools/bench_mask_mfft.py, whose timing loop
and float64 reference it imports, on their seven legs.

Legs (DESIGN.md sections 41 to 43), centred, reflect padding, length = T:
  T1    BH-4, P 24, 32 b; B 64, T 160 000, 400 / 512 / 160          T2    BH-7, P 12, 32 b; B 1, T 2^24, 2048 / 2048 / 512
  N64   BH-4, P 24, 32 b; B 64, T 160 000, 64 / 64 / 32             S400  BH-4, P 24, 32 b; B 64, T 160 000, 400 / 400 / 160
  A960  BH-4, P 24, 32 b; B 64, T 160 000, 960 / 960 / 480          L2000 BH-7, P 12, 32 b; B 1, T 2^24, 2000 / 2000 / 500
  N96   BH-4, P 24, 32 b; B 64, T 160 000, 96 / 96 / 48
Variants, all from one resident table, outputs preallocated:
  (a) the fused call with full (B, F, K) complex gains     (b) the fused call with one (K,) row of complex gains
  (c) stft* + a torch complex multiply (in place) + istft*: the route the call replaces      (d) the two transforms alone
  (e) a plain copy of (a)'s bytes: read B * T * 4 + B * F * K * 8, write B * T * 4 (one copy_ of half that many bytes each way)
A clock ramp, every variant warmed, --steps steps of --reps back-to-back calls between device events, the variants of a leg alternated
step by step, medians.  The aim -- (a) and (b) below (c), judged outside (c)'s own spread (max - min) / median of its step medians -- is
reported, met or missed, not asserted.  What IS asserted, on the timed data of every leg: (a) equals the exact reference word for
word -- istft*(Z) with Z the four separately rounded float32 products of the contract on the planes of stft*(x).  Whether (c), torch's
complex multiply, gives the same words is recorded, not asserted: the contract does not promise it.  The end-to-end errors of the
fused call and of torch.istft(torch.stft(x) * G) against numpy in float64 are recorded on a short signal of each leg's shape.

Each leg runs in a child process of its own under a time limit (--leg-timeout seconds); a leg that fails or runs out of time is
recorded as such and the legs after it are not started.

    python tools/bench_cmask.py [--steps 10] [--reps 20] [--out FILE] [--quick] [--legs T1,S400]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mask_fft import LEGS as POW2_LEGS, ref64, timed  # noqa: E402
from bench_mask_mfft import LEGS as MIXED_LEGS  # noqa: E402

LEGS = {**{k: ("fft",) + v for k, v in POW2_LEGS.items()}, **{k: ("mfft",) + v for k, v in MIXED_LEGS.items()}}


def gains(torch, shape, generator):
    """Complex64 gains on the device: magnitudes uniform in [0, 2) times unit phases uniform on the circle."""
    mag = torch.rand(shape, device="cuda", generator=generator) * 2.0
    ph = torch.rand(shape, device="cuda", generator=generator) * 6.283185307179586
    return torch.complex(mag * torch.cos(ph), mag * torch.sin(ph))


def exact_rows(torch, Y, G):
    """The contract's masked rows: four separately rounded float32 products on the planes, one subtraction, one addition."""
    yr, yi, gr, gi = Y.real, Y.imag, G.real, G.imag
    return torch.complex(yr * gr - yi * gi, yr * gi + yi * gr)


def run_leg(name, steps, reps):
    import numpy as np
    import torch
    import blackman_harris_win_amd as bhw
    from blackman_harris_win_amd import binding as B
    fam, win, pw, nb, T, L, nfft, hop = LEGS[name]
    mixed = fam == "mfft"
    fused = bhw.stft_cmask_istft_mixed if mixed else bhw.stft_cmask_istft
    describe = B.describe_cmask_mfft if mixed else B.describe_cmask_fft
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
    G = gains(torch, (nb, F, K), g)
    row = G[0, 0].contiguous()
    kw = dict(win_length=L, length=T)
    rec = {"leg": name, "family": fam, "B": nb, "T": T, "L": L, "nfft": nfft, "hop": hop, "frames": F, "bins": K}
    with bhw.ResidentTable(p) as t:
        stft, istft = (t.stft_mixed, t.istft_mixed) if mixed else (t.stft, t.istft)
        Y = stft(p, x, nfft, hop, win_length=L)
        assert tuple(Y.shape) == (nb, F, K)
        out = torch.empty((nb, T), device="cuda")
        bytes_in, bytes_out = nb * T * 4 + nb * F * K * 8, nb * T * 4
        half = (bytes_in + bytes_out) // 2 // 4
        src, dst = torch.empty(half, device="cuda"), torch.empty(half, device="cuda")

        def three_calls():
            stft(p, x, nfft, hop, win_length=L, out=Y)
            Y.mul_(G)
            istft(p, Y, nfft, hop, out=out, **kw)

        def two_calls():
            stft(p, x, nfft, hop, win_length=L, out=Y)
            istft(p, Y, nfft, hop, out=out, **kw)

        r = timed(torch, {"a_fused_full_gains": lambda: fused(p, x, G, nfft, hop, out=out, table=t, **kw),
                          "b_fused_one_gain_row": lambda: fused(p, x, row, nfft, hop, out=out, table=t, **kw),
                          "c_stft_complex_multiply_istft": three_calls,
                          "d_stft_istft": two_calls,
                          "e_copy_of_its_bytes": lambda: dst.copy_(src)}, steps, reps)
        sa = B.make_stft(nb, T, F, hop, nfft, col0=col0, pad=pad, pad_mode=B.PAD_REFLECT, shift=p.dat_width - 1)
        ss = B.make_stft(nb, T, F, hop, nfft, col0=col0, pad=pad, shift=p.dat_width - 1)
        rec["plan"] = describe(p, L, sa, ss, normalize=True, g_stride=K, g_batch_stride=F * K, table=t.handle)
        m = {k: v["median_ms"] for k, v in r.items()}
        c = r["c_stft_complex_multiply_istft"]
        spread = (c["max_ms"] - c["min_ms"]) / c["median_ms"]
        mc = m["c_stft_complex_multiply_istft"]
        rec.update({"times": r, "bytes_in": bytes_in, "bytes_out": bytes_out, "bytes_of_the_spectrum_the_three_calls_move": 4 * nb * F * K * 8,
                    "a_over_c": m["a_fused_full_gains"] / mc, "b_over_c": m["b_fused_one_gain_row"] / mc,
                    "a_over_d": m["a_fused_full_gains"] / m["d_stft_istft"], "a_over_copy": m["a_fused_full_gains"] / m["e_copy_of_its_bytes"],
                    "multiply_ms_c_minus_d": mc - m["d_stft_istft"], "spread_of_c": spread,
                    "aim_a_below_c": m["a_fused_full_gains"] < mc * (1.0 - spread),
                    "aim_b_below_c": m["b_fused_one_gain_row"] < mc * (1.0 - spread),
                    "a_GBps": (bytes_in + bytes_out) / m["a_fused_full_gains"] / 1e6})
        del src, dst
        # (a) is the exact reference word for word, on the timed data
        three_calls()
        by_torch = out.clone()
        stft(p, x, nfft, hop, win_length=L, out=Y)
        want = istft(p, exact_rows(torch, Y, G), nfft, hop, **kw)
        got = fused(p, x, G, nfft, hop, table=t, **kw)
        rec["word_for_word_the_exact_reference"] = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
        rec["word_for_word_torchs_complex_multiply"] = bool(torch.equal(got.view(torch.int32), by_torch.view(torch.int32)))
        rec["max_abs_difference_from_torchs_complex_multiply"] = float((got - by_torch).abs().max())
        assert rec["word_for_word_the_exact_reference"], f"leg {name}: the fused output is not the exact reference's word for word"
        wrow = istft(p, exact_rows(torch, Y, row), nfft, hop, **kw)
        grow = fused(p, x, row, nfft, hop, table=t, **kw)
        assert torch.equal(grow.view(torch.int32), wrow.view(torch.int32)), f"leg {name}: one gain row is not the exact reference's word for word"
        del want, got, wrow, grow, by_torch
        # accuracy on two signals of at most 400 frames of the leg's shape
        Fa = min(F, 400)
        Ta = hop * (Fa - 1)
        xa, ga = x[:min(nb, 2), :Ta].contiguous(), G[:min(nb, 2), :Fa].contiguous()
        v = bhw.window(p, L, dtype=torch.float32)
        fz = fused(p, xa, ga, nfft, hop, win_length=L, length=Ta, table=t)
        St = torch.stft(xa, nfft, hop, L, window=v, center=True, pad_mode="reflect", return_complex=True)
        yard = torch.istft(St * ga.transpose(-1, -2), nfft, hop, L, window=v, center=True, length=Ta)
        ref = ref64(np, xa.cpu().numpy(), ga.cpu().numpy().astype(np.complex128), v.cpu().numpy(), nfft, hop, L, Ta)
        e_f = float(np.abs(fz.cpu().numpy().astype(np.float64) - ref).max())
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
        if k.startswith(("k_cmask_", "k_mask_")):
            key = json.dumps({"family": k.split("_direct")[0].split("_table")[0],
                              **{n: v.get(n) for n in ("VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy")}}, sort_keys=True)
            out.setdefault(key, []).append(k)
    return [{"figures": json.loads(k), "instances": len(v), "example": v[0]} for k, v in out.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r43_cmask.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written")
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated leg names (default: all seven)")
    ap.add_argument("--leg", default=None, help="(internal) run one leg in this process and print its record")
    ap.add_argument("--leg-timeout", type=int, default=240)
    a = ap.parse_args()
    steps, reps = (2, 3) if a.quick else (a.steps, a.reps)
    if a.leg:
        print(json.dumps(run_leg(a.leg, steps, reps)))
        return 0
    rec = {"steps": steps, "reps": reps, "legs": [], "kernel_resources": resources()}
    for name in a.legs.split(","):
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
