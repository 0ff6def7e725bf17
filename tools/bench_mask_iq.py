#!/usr/bin/env python3
"""The fused STFT + gain + inverse STFT kernels for I/Q input (bhw_[c]mask_cfft_f32_* / bhw_[c]mask_cmfft_f32_*, through
bhw.stft_mask_istft_iq, bhw.stft_cmask_istft_iq and their _mixed siblings) on one GPU.  Prints one JSON record and writes it to --out
(profiles/r44_mask_iq.json by default).  The protocol is that of tools/bench_cmask.py, whose timing loop it shares
(tools/bench_mask_fft.py: timed).

Legs, complex64 input, centred, reflect padding, length = T; each with pair gains and with real gains:
  I1    BH-4, P 24, 32 b; B 64, T 160 000, 400 / 512 / 160          I2    BH-7, P 12, 32 b; B 1, T 2^23, 2048 / 2048 / 512
  IN64  BH-4, P 24, 32 b; B 64, T 160 000, 64 / 64 / 32             IS400 BH-4, P 24, 32 b; B 64, T 160 000, 400 / 400 / 160
  IA960 BH-4, P 24, 32 b; B 64, T 160 000, 960 / 960 / 480          IL2000 BH-7, P 12, 32 b; B 1, T 2^23, 2000 / 2000 / 500
  IO75  BH-4, P 24, 32 b; B 64, T 160 000, 75 / 75 / 25
Variants, all from one resident table, outputs preallocated:
  (a) the fused call with full (B, F, K) gains, K = n_fft      (b) the fused call with one (K,) row of gains
  (c) stft_iq* + a torch multiply (in place; complex for pair gains, real for real gains) + istft_iq*: the route the call replaces
  (d) the two transforms alone
  (e) a plain copy of (a)'s bytes: read B * T * 8 + the gains, write B * T * 8 (one copy_ of half that many bytes each way)
A clock ramp, every variant warmed, --steps steps of --reps back-to-back calls between device events, the variants of a leg alternated
step by step, medians.  The aim -- (a) and (b) below (c), judged outside (c)'s own spread (max - min) / median of its step medians -- is
reported, met or missed, not asserted.  What IS asserted, on the timed data of every leg: (a) and (b) equal the exact reference word
for word -- istft_iq*(Z) with Z the separately rounded float32 products of the contract on the planes of stft_iq*(x).  The end-to-end
errors of the fused call and of torch.istft(torch.stft(x) * G) in complex64 against the same expression in complex128 are recorded on
a short signal of each leg's shape.

Each leg runs in a child process of its own under a time limit (--leg-timeout seconds); a leg that fails or runs out of time is
recorded as such and the legs after it are not started.

    python tools/bench_mask_iq.py [--steps 10] [--reps 20] [--out FILE] [--quick] [--legs I1,IS400] [--gains pair,real]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mask_fft import timed  # noqa: E402

# leg -> (family, window, phase width, B, T, L, n_fft, hop)
LEGS = {
    "I1": ("cfft", "bh4", 24, 64, 160000, 400, 512, 160),
    "I2": ("cfft", "bh7", 12, 1, 1 << 23, 2048, 2048, 512),
    "IN64": ("cfft", "bh4", 24, 64, 160000, 64, 64, 32),
    "IS400": ("cmfft", "bh4", 24, 64, 160000, 400, 400, 160),
    "IA960": ("cmfft", "bh4", 24, 64, 160000, 960, 960, 480),
    "IL2000": ("cmfft", "bh7", 12, 1, 1 << 23, 2000, 2000, 500),
    "IO75": ("cmfft", "bh4", 24, 64, 160000, 75, 75, 25),
}


def gains(torch, shape, generator, pair):
    """Gains on the device: magnitudes uniform in [0, 2), for pairs times unit phases uniform on the circle."""
    mag = torch.rand(shape, device="cuda", generator=generator) * 2.0
    if not pair:
        return mag
    ph = torch.rand(shape, device="cuda", generator=generator) * 6.283185307179586
    return torch.complex(mag * torch.cos(ph), mag * torch.sin(ph))


def exact_rows(torch, Y, G):
    """The contract's masked rows: separately rounded float32 products on the planes (and one subtraction, one addition for pairs)."""
    yr, yi = Y.real, Y.imag
    if not G.is_complex():
        return torch.complex(yr * G, yi * G)
    gr, gi = G.real, G.imag
    return torch.complex(yr * gr - yi * gi, yr * gi + yi * gr)


def _same(torch, a, b):
    return bool(torch.equal(torch.view_as_real(a).view(torch.int32), torch.view_as_real(b).view(torch.int32)))


def run_leg(name, gtype, steps, reps):
    import torch
    import blackman_harris_win_amd as bhw
    from blackman_harris_win_amd import binding as B
    fam, win, pw, nb, T, L, nfft, hop = LEGS[name]
    mixed, pair = fam == "cmfft", gtype == "pair"
    fused = getattr(bhw, f"stft_{'c' if pair else ''}mask_istft_iq{'_mixed' if mixed else ''}")
    describe = getattr(B, f"describe_{'c' if pair else ''}mask_{fam}")
    p = B.make_params(B.WIN_BH4 if win == "bh4" else B.WIN_BH7, pw, 32)
    a = torch.randn((4096, 4096), device="cuda")                        # the clock ramp: a second of work in front of the timed region
    for _ in range(40):
        a = (a @ a).clamp_(-1, 1)
    torch.cuda.synchronize()
    del a
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((nb, T, 2), device="cuda", generator=g) + 3.0)
    K, pad, col0 = nfft, nfft // 2, (nfft - L) // 2
    F = 1 + (T + 2 * pad - nfft) // hop
    G = gains(torch, (nb, F, K), g, pair)
    row = G[0, 0].contiguous()
    ge = 8 if pair else 4
    kw = dict(win_length=L, length=T)
    rec = {"leg": name, "gains": gtype, "family": fam, "B": nb, "T": T, "L": L, "nfft": nfft, "hop": hop, "frames": F, "bins": K}
    with bhw.ResidentTable(p) as t:
        stft, istft = (t.stft_iq_mixed, t.istft_iq_mixed) if mixed else (t.stft_iq, t.istft_iq)
        Y = stft(p, x, nfft, hop, win_length=L)
        assert tuple(Y.shape) == (nb, F, K)
        out = torch.empty((nb, T), dtype=torch.complex64, device="cuda")
        bytes_in, bytes_out = nb * T * 8 + nb * F * K * ge, nb * T * 8
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
                          "c_stft_multiply_istft": three_calls,
                          "d_stft_istft": two_calls,
                          "e_copy_of_its_bytes": lambda: dst.copy_(src)}, steps, reps)
        sa = B.make_stft(nb, T, F, hop, nfft, col0=col0, pad=pad, pad_mode=B.PAD_REFLECT, channels=2, shift=p.dat_width - 1)
        ss = B.make_stft(nb, T, F, hop, nfft, col0=col0, pad=pad, channels=2, shift=p.dat_width - 1)
        rec["plan"] = describe(p, L, sa, ss, normalize=True, g_stride=K, g_batch_stride=F * K, table=t.handle)
        m = {k: v["median_ms"] for k, v in r.items()}
        c = r["c_stft_multiply_istft"]
        spread = (c["max_ms"] - c["min_ms"]) / c["median_ms"]
        mc = m["c_stft_multiply_istft"]
        rec.update({"times": r, "bytes_in": bytes_in, "bytes_out": bytes_out, "bytes_of_the_spectrum_the_three_calls_move": 4 * nb * F * K * 8,
                    "a_over_c": m["a_fused_full_gains"] / mc, "b_over_c": m["b_fused_one_gain_row"] / mc,
                    "a_over_d": m["a_fused_full_gains"] / m["d_stft_istft"], "a_over_copy": m["a_fused_full_gains"] / m["e_copy_of_its_bytes"],
                    "multiply_ms_c_minus_d": mc - m["d_stft_istft"], "spread_of_c": spread,
                    "aim_a_below_c": m["a_fused_full_gains"] < mc * (1.0 - spread),
                    "aim_b_below_c": m["b_fused_one_gain_row"] < mc * (1.0 - spread),
                    "a_GBps": (bytes_in + bytes_out) / m["a_fused_full_gains"] / 1e6})
        del src, dst
        # (a) and (b) are the exact reference word for word, on the timed data
        three_calls()
        by_torch = out.clone()
        stft(p, x, nfft, hop, win_length=L, out=Y)
        want = istft(p, exact_rows(torch, Y, G), nfft, hop, **kw)
        got = fused(p, x, G, nfft, hop, table=t, **kw)
        rec["word_for_word_the_exact_reference"] = _same(torch, got, want)
        rec["word_for_word_torchs_multiply"] = _same(torch, got, by_torch)
        rec["max_abs_difference_from_torchs_multiply"] = float((got - by_torch).abs().max())
        assert rec["word_for_word_the_exact_reference"], f"leg {name}: the fused output is not the exact reference's word for word"
        wrow = istft(p, exact_rows(torch, Y, row), nfft, hop, **kw)
        grow = fused(p, x, row, nfft, hop, table=t, **kw)
        assert _same(torch, grow, wrow), f"leg {name}: one gain row is not the exact reference's word for word"
        del want, got, wrow, grow, by_torch
        # accuracy on two signals of at most 400 frames of the leg's shape
        Fa = min(F, 400)
        Ta = hop * (Fa - 1) + nfft - 2 * pad
        xa, ga = x[:min(nb, 2), :Ta].contiguous(), G[:min(nb, 2), :Fa].contiguous()
        v = bhw.window(p, L, dtype=torch.float32)
        fz = fused(p, xa, ga, nfft, hop, win_length=L, length=Ta, table=t)

        def chain(xx, vv, gg):
            S = torch.stft(xx, nfft, hop, L, window=vv, center=True, pad_mode="reflect", onesided=False, return_complex=True)
            return torch.istft(S * gg.transpose(-1, -2), nfft, hop, L, window=vv, center=True, length=Ta, onesided=False, return_complex=True)

        yard = chain(xa, v, ga)
        ref = chain(xa.to(torch.complex128), v.double(), ga.to(torch.complex128) if pair else ga.double())
        e_f = float((fz.to(torch.complex128) - ref).abs().max())
        e_t = float((yard.to(torch.complex128) - ref).abs().max())
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
        if k.startswith(("k_cmask_c", "k_mask_c", "k_istft_c")):
            key = json.dumps({"family": k.split("_direct")[0].split("_table")[0],
                              **{n: v.get(n) for n in ("VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy")}}, sort_keys=True)
            out.setdefault(key, []).append(k)
    return [{"figures": json.loads(k), "instances": len(v), "example": v[0]} for k, v in out.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r44_mask_iq.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written")
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated leg names (default: all seven)")
    ap.add_argument("--gains", default="pair,real", help="comma-separated gain types (default: both)")
    ap.add_argument("--leg", default=None, help="(internal) run one leg in this process and print its record: NAME:GAINS")
    ap.add_argument("--leg-timeout", type=int, default=240)
    a = ap.parse_args()
    steps, reps = (2, 3) if a.quick else (a.steps, a.reps)
    if a.leg:
        name, gtype = a.leg.split(":")
        print(json.dumps(run_leg(name, gtype, steps, reps)))
        return 0
    rec = {"steps": steps, "reps": reps, "legs": [], "kernel_resources": resources()}
    failed = False
    for name in a.legs.split(","):
        for gtype in a.gains.split(","):
            cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", f"{name}:{gtype}", "--steps",
                   str(steps), "--reps", str(reps)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            if r.returncode != 0:
                rec["legs"].append({"leg": name, "gains": gtype, "failed": r.returncode, "stderr": r.stderr[-1000:]})
                failed = True
                break                                                    # nothing more is started on the GPU after a failed step
            rec["legs"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        if failed:
            break
    print(json.dumps(rec))
    if not a.quick:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0 if not failed else 1


if __name__ == "__main__":
    sys.exit(main())
