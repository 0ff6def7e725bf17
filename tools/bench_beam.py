#!/usr/bin/env python3
"""The fused multichannel filter-and-sum kernels of both families (bhw_beam_fft_f32_* / bhw_beam_mfft_f32_*, through
bhw.stft_beamform_istft / bhw.stft_beamform_istft_mixed) on one GPU.  Prints one JSON record and writes it to --out
(profiles/r45_beam.json by default).  The protocol is that of tools/bench_cmask.py, whose legs and timing loop it imports.

Legs: the seven shapes of section 43, centred, reflect padding, length = T, with the 64 signals of the five batch
legs arranged as 8 signals x 8 channels ("-8x8") and as 32 x 2 ("-32x2"), and the two 2^24-sample legs as 1 signal x 4 channels of
2^22 ("-1x4").
Variants, all from one resident table, outputs preallocated:
  (a) the fused call with full (B, C, F, K) weights
  (y1) stft* on the (B * C, T) batch, a torch complex multiply by the weights and a sum over the channels, istft*
  (y2) C calls of stft_cmask_istft* on the channels (strided views, read in place) and a time-domain sum
  (e) a plain copy of (a)'s bytes
The yardstick of a leg is the FASTER of (y1) and (y2), measured in the same process; it is never the code under test.  A clock ramp,
every variant warmed, --steps steps of --reps back-to-back calls between device events, the variants of a leg alternated step by step,
medians.  The aim -- (a) below the yardstick by more than the yardstick's own spread (max - min) / median of its step medians -- is
reported, met or missed, with the ratio; it is not asserted.  What IS asserted, on the timed data of every leg: (a) equals the exact
reference word for word -- istft*(Z) with Z the contract's separately rounded float32 products of stft*(x) per channel, summed per part
in float32 in ascending channel order.

Each leg runs in a child process of its own under a time limit (--leg-timeout seconds); a leg that fails or runs out of time is
recorded as such and the legs after it are not started.

    python tools/bench_beam.py [--steps 10] [--reps 20] [--out FILE] [--quick] [--legs T1-8x8,S400-32x2]
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
from bench_cmask import LEGS as CMASK_LEGS, exact_rows, gains  # noqa: E402

LEGS = {}
for _name, (_fam, _win, _pw, _nb, _T, _L, _nfft, _hop) in CMASK_LEGS.items():
    if _nb == 64:
        LEGS[_name + "-8x8"] = (_fam, _win, _pw, 8, 8, _T, _L, _nfft, _hop)
        LEGS[_name + "-32x2"] = (_fam, _win, _pw, 32, 2, _T, _L, _nfft, _hop)
    else:
        LEGS[_name + "-1x4"] = (_fam, _win, _pw, _nb, 4, _T // 4, _L, _nfft, _hop)


def exact_sum(torch, Y, G):
    """The contract's summed rows: exact_rows() per channel (axis 1), Z = P_0, then Z = Z + P_c per part in float32, ascending."""
    Z = exact_rows(torch, Y[:, 0], G[:, 0])
    for c in range(1, Y.shape[1]):
        P = exact_rows(torch, Y[:, c], G[:, c])
        Z = torch.complex(Z.real + P.real, Z.imag + P.imag)
    return Z


def run_leg(name, steps, reps):
    import torch
    import blackman_harris_win_amd as bhw
    from blackman_harris_win_amd import binding as B
    fam, win, pw, nb, C, T, L, nfft, hop = LEGS[name]
    mixed = fam == "mfft"
    fused = bhw.stft_beamform_istft_mixed if mixed else bhw.stft_beamform_istft
    cmask = bhw.stft_cmask_istft_mixed if mixed else bhw.stft_cmask_istft
    describe = B.describe_beam_mfft if mixed else B.describe_beam_fft
    p = B.make_params(B.WIN_BH4 if win == "bh4" else B.WIN_BH7, pw, 32)
    a = torch.randn((4096, 4096), device="cuda")                        # the clock ramp: a second of work in front of the timed region
    for _ in range(40):
        a = (a @ a).clamp_(-1, 1)
    torch.cuda.synchronize()
    del a
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((nb, C, T), device="cuda", generator=g) + 3.0
    K, pad, col0 = nfft // 2 + 1, nfft // 2, (nfft - L) // 2
    F = 1 + T // hop
    G = gains(torch, (nb, C, F, K), g)
    kw = dict(win_length=L, length=T)
    rec = {"leg": name, "family": fam, "B": nb, "C": C, "T": T, "L": L, "nfft": nfft, "hop": hop, "frames": F, "bins": K}
    with bhw.ResidentTable(p) as t:
        stft, istft = (t.stft_mixed, t.istft_mixed) if mixed else (t.stft, t.istft)
        xf = x.view(nb * C, T)
        Y = stft(p, xf, nfft, hop, win_length=L)
        assert tuple(Y.shape) == (nb * C, F, K)
        Y4 = Y.view(nb, C, F, K)
        Z = torch.empty((nb, F, K), dtype=torch.complex64, device="cuda")
        out = torch.empty((nb, T), device="cuda")
        per_channel = torch.empty((C, nb, T), device="cuda")
        bytes_in, bytes_out = nb * C * T * 4 + nb * C * F * K * 8, nb * T * 4
        half = (bytes_in + bytes_out) // 2 // 4
        src, dst = torch.empty(half, device="cuda"), torch.empty(half, device="cuda")

        def spectra_route():
            stft(p, xf, nfft, hop, win_length=L, out=Y)
            Y4.mul_(G)
            torch.sum(Y4, dim=1, out=Z)
            istft(p, Z, nfft, hop, out=out, **kw)

        def channel_route():
            for c in range(C):
                cmask(p, x[:, c], G[:, c], nfft, hop, out=per_channel[c], table=t, **kw)
            torch.sum(per_channel, dim=0, out=out)

        r = timed(torch, {"a_fused": lambda: fused(p, x, G, nfft, hop, out=out, table=t, **kw),
                          "y1_stft_multiply_sum_istft": spectra_route,
                          "y2_cmask_per_channel_and_sum": channel_route,
                          "e_copy_of_its_bytes": lambda: dst.copy_(src)}, steps, reps)
        sa = B.make_stft(nb, T, F, hop, nfft, col0=col0, pad=pad, pad_mode=B.PAD_REFLECT, shift=p.dat_width - 1)
        ss = B.make_stft(nb, T, F, hop, nfft, col0=col0, pad=pad, shift=p.dat_width - 1)
        rec["plan"] = describe(p, L, sa, ss, C, normalize=True, g_stride=K, g_ch_stride=F * K, g_batch_stride=C * F * K, table=t.handle)
        m = {k: v["median_ms"] for k, v in r.items()}
        which = min(("y1_stft_multiply_sum_istft", "y2_cmask_per_channel_and_sum"), key=lambda k: m[k])
        y = r[which]
        spread = (y["max_ms"] - y["min_ms"]) / y["median_ms"]
        rec.update({"times": r, "bytes_in": bytes_in, "bytes_out": bytes_out, "yardstick": which, "spread_of_the_yardstick": spread,
                    "a_over_yardstick": m["a_fused"] / y["median_ms"], "a_over_y1": m["a_fused"] / m["y1_stft_multiply_sum_istft"],
                    "a_over_y2": m["a_fused"] / m["y2_cmask_per_channel_and_sum"], "a_over_copy": m["a_fused"] / m["e_copy_of_its_bytes"],
                    "aim_a_below_the_yardstick": m["a_fused"] < y["median_ms"] * (1.0 - spread),
                    "a_GBps": (bytes_in + bytes_out) / m["a_fused"] / 1e6})
        del src, dst, per_channel
        # (a) is the exact reference word for word, on the timed data
        stft(p, xf, nfft, hop, win_length=L, out=Y)
        want = istft(p, exact_sum(torch, Y4, G), nfft, hop, **kw)
        got = fused(p, x, G, nfft, hop, table=t, **kw)
        rec["word_for_word_the_exact_reference"] = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
        assert rec["word_for_word_the_exact_reference"], f"leg {name}: the fused output is not the exact reference's word for word"
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
        if k.startswith(("k_beam_", "k_cmask_fft", "k_cmask_mfft")):
            key = json.dumps({"family": k.split("_direct")[0].split("_table")[0],
                              **{n: v.get(n) for n in ("VGPRs", "VGPRs Spill", "ScratchSize", "Occupancy")}}, sort_keys=True)
            out.setdefault(key, []).append(k)
    return [{"figures": json.loads(k), "instances": len(v), "example": v[0]} for k, v in out.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r45_beam.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written")
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated leg names (default: all twelve)")
    ap.add_argument("--leg", default=None, help="(internal) run one leg in this process and print its record")
    ap.add_argument("--leg-timeout", type=int, default=120)
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
