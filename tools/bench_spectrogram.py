#!/usr/bin/env python3
"""The fused spectrogram (bhw_spectrogram_f32_* / bhw.spectrogram) on one GPU, one process.  Prints one JSON record and writes it to
--out (profiles/r16_spectrogram.json by default).

Legs, all centred with reflect padding:
  T1 batch   BH-4, P 24, 32 b; B 64, T 160 000, 400 / 512 / 160, 80 mels
  T2 long    BH-7, P 12, 32 b; B 1, T 2^24, 4096 / 4096 / 1024, 128 mels
  N64 short  BH-4, P 24, 32 b; B 64, T 160 000, 64 / 64 / 32, 10 mels
Variants, each from a resident table and in library form where the library has one:
  (a) the power spectrogram                    (b) the bank spectrogram                (c) bhw.stft alone
  (d) bhw.stft + the torch expressions for power (abs() ** 2), and for power . bank (matmul)
  (e) torch.stft + the same expressions        (f) a plain copy of the call's bytes (of (a)'s and of (b)'s)
Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events, the variants of a leg alternated step
by step, after a clock ramp; times are per call (median, min, max over --steps).  (a) and (b) are compared with (c) of the same
process; the margin is the spread of (c)'s own step medians.

    python tools/bench_spectrogram.py [--steps 10] [--reps 20] [--out FILE] [--quick]
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
    return {"T1": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 400, 512, 160, 80),
            "T2": (B.make_params(B.WIN_BH7, 12, 32), 1, 1 << 24, 4096, 4096, 1024, 128),
            "N64": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 64, 64, 32, 10)}


def ramp():
    """A second of work in front of the timed region: the clock has ramped when the first leg starts."""
    a = torch.randn((4096, 4096), device="cuda")
    for _ in range(40):
        a = (a @ a).clamp_(-1, 1)
    torch.cuda.synchronize()


def leg(name, p, nb, T, L, nfft, hop, mels, steps, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((nb, T), device="cuda", generator=g) + 3.0
    F, K = 1 + T // hop, nfft // 2 + 1
    rec = {"leg": name, "B": nb, "T": T, "L": L, "nfft": nfft, "hop": hop, "frames": F, "mels": mels}
    mel = bhw.mel_weights(nfft, mels, 16000)
    fb = bhw.FilterBank(mel, device="cuda")
    bank = torch.from_numpy(mel).cuda()
    v = bhw.window(p, L, dtype=torch.float32)
    kw = dict(win_length=L)
    with bhw.ResidentTable(p) as t:
        P = torch.empty((nb, F, K), device="cuda")
        Pm = torch.empty((nb, F, mels), device="cuda")
        Y = torch.empty((nb, F, K), dtype=torch.complex64, device="cuda")
        bytes_in, out_a, out_b, out_c = nb * T * 4, nb * F * K * 4, nb * F * mels * 4, nb * F * K * 8
        ha, hb = (bytes_in + out_a) // 8, (bytes_in + out_b) // 8
        src, dst = torch.empty(ha, device="cuda"), torch.empty(ha, device="cuda")

        def torch_stft():
            return torch.stft(x, nfft, hop, L, window=v, center=True, pad_mode="reflect", return_complex=True)

        r = timed({"a_power_table": lambda: t.spectrogram(p, x, nfft, hop, out=P, **kw),
                   "a_power_library": lambda: bhw.spectrogram(p, x, nfft, hop, out=P, **kw),
                   "b_bank_table": lambda: t.spectrogram(p, x, nfft, hop, fbank=fb, out=Pm, **kw),
                   "b_bank_library": lambda: bhw.spectrogram(p, x, nfft, hop, fbank=fb, out=Pm, **kw),
                   "c_stft_table": lambda: t.stft(p, x, nfft, hop, out=Y, **kw),
                   "c_stft_library": lambda: bhw.stft(p, x, nfft, hop, out=Y, **kw),
                   "d_stft_power_table": lambda: t.stft(p, x, nfft, hop, out=Y, **kw).abs() ** 2,
                   "d_stft_bank_table": lambda: torch.matmul(t.stft(p, x, nfft, hop, out=Y, **kw).abs() ** 2, bank),
                   "d_stft_bank_library": lambda: torch.matmul(bhw.stft(p, x, nfft, hop, out=Y, **kw).abs() ** 2, bank),
                   "e_torch_power": lambda: torch_stft().abs() ** 2,
                   "e_torch_bank": lambda: torch.matmul((torch_stft().abs() ** 2).transpose(-1, -2), bank),
                   "f_copy_of_a_bytes": lambda: dst.copy_(src),
                   "f_copy_of_b_bytes": lambda: dst[:hb].copy_(src[:hb])}, steps, reps)
        s = B.make_stft(nb, T, F, hop, nfft, col0=(nfft - L) // 2, pad=nfft // 2, pad_mode=B.PAD_REFLECT, shift=p.dat_width - 1)
        rec["plan_power"] = B.describe_spectrogram(p, L, s, table=t.handle)
        rec["plan_bank"] = B.describe_spectrogram(p, L, s, fbank=fb.descriptor, table=t.handle)
        m = {k: q["median_ms"] for k, q in r.items()}
        c = r["c_stft_table"]
        rec.update({"times": r, "bytes_in": bytes_in, "bytes_out_power": out_a, "bytes_out_bank": out_b, "bytes_out_stft": out_c,
                    "c_spread": (c["max_ms"] - c["min_ms"]) / c["median_ms"],
                    "a_over_c": m["a_power_table"] / m["c_stft_table"], "b_over_c": m["b_bank_table"] / m["c_stft_table"],
                    "a_over_c_library": m["a_power_library"] / m["c_stft_library"], "b_over_c_library": m["b_bank_library"] / m["c_stft_library"],
                    "a_over_d": m["a_power_table"] / m["d_stft_power_table"], "b_over_d": m["b_bank_table"] / m["d_stft_bank_table"],
                    "a_over_e": m["a_power_table"] / m["e_torch_power"], "b_over_e": m["b_bank_table"] / m["e_torch_bank"],
                    "a_over_copy": m["a_power_table"] / m["f_copy_of_a_bytes"], "b_over_copy": m["b_bank_table"] / m["f_copy_of_b_bytes"]})
    return rec


def resources():
    path = os.path.join(ROOT, "blackman_harris_win_amd", "kernel_resources.json")
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        res = json.load(f)
    out = {}
    for k, q in res.items():
        if k.startswith("k_spectrogram"):
            key = json.dumps({n: q.get(n) for n in ("VGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy")}, sort_keys=True)
            out.setdefault(key, []).append(k)
    return [{"figures": json.loads(k), "instances": len(q), "example": q[0]} for k, q in out.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_spectrogram.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written")
    a = ap.parse_args()
    steps, reps = (2, 3) if a.quick else (a.steps, a.reps)
    ramp()
    rec = {"device": torch.cuda.get_device_name(0), "steps": steps, "reps": reps, "legs": [], "kernel_resources": resources()}
    for name, (p, nb, T, L, nfft, hop, mels) in legs().items():
        rec["legs"].append(leg(name, p, nb, T, L, nfft, hop, mels, steps, reps))
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec))
    if not a.quick:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
