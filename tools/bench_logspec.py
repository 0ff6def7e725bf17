#!/usr/bin/env python3
"""The fused log-mel spectrogram and MFCC (bhw_logspec_f32_*, bhw_logspec_mfft_f32_* / bhw.log_spectrogram(_mixed), bhw.mfcc(_mixed)) on
one GPU, one process.  Prints one JSON record and writes it to --out (profiles/r40_logspec.json by default); --tests FILE folds in
the record tests/test_gpu_logspec.py writes under BHW_LOGSPEC_RECORD (the share of log words that are not bit-equal, the end-to-end
errors).

Legs, all centred with reflect padding, log = 10 log10(max(q, 1e-10)) (torchaudio amplitude_to_DB of a power), 13 coefficients:
  M400 speech  BH-4, P 24, 32 b; B 64, T 160 000, 400 / 400 / 160, mixed radix, 80 mel
  T1 batch     BH-4, P 24, 32 b; B 64, T 160 000, 400 / 512 / 160, 80 mel
  T2 long      BH-7, P 12, 32 b; B 1, T 2^24, 4096 / 4096 / 1024, 128 mel
  N64 short    BH-4, P 24, 32 b; B 64, T 160 000, 64 / 64 / 32, 10 mel
Variants, each from a resident table and in library form:
  (a) the log-mel spectrogram in one launch    (b) 13 MFCCs in one launch       (c) spectrogram(_mixed)(fbank) alone
  (d) (c) + torch clamp, log10 and mul        (e) (d) + matmul with the DCT    (f) a plain copy of the call's bytes (of (a)'s and (b)'s)
The protocol is tools/bench_spectrogram.py's: every variant warmed, then timed in steps of `reps` back-to-back calls between device
events, the variants of a leg alternated step by step, after a clock ramp; times are per call (median, min, max over --steps).  The
spread of a route is (max - min) / median of its own step medians.

    python tools/bench_logspec.py [--steps 10] [--reps 20] [--out FILE] [--tests FILE] [--quick]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import blackman_harris_win_amd as bhw  # noqa: E402
from blackman_harris_win_amd import binding as B  # noqa: E402
from bench_spectrogram import ramp, timed  # noqa: E402

COEFFS, FLOOR, DB = 13, 1e-10, 10.0 / math.log(10.0)


def legs():
    return {"M400": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 400, 400, 160, 80),
            "T1": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 400, 512, 160, 80),
            "T2": (B.make_params(B.WIN_BH7, 12, 32), 1, 1 << 24, 4096, 4096, 1024, 128),
            "N64": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 64, 64, 32, 10)}


def leg(name, p, nb, T, L, nfft, hop, mels, steps, reps):
    mixed = B.mfft_supported(nfft)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((nb, T), device="cuda", generator=g) + 3.0
    F = 1 + T // hop
    coeffs = min(COEFFS, mels)
    rec = {"leg": name, "B": nb, "T": T, "L": L, "nfft": nfft, "hop": hop, "frames": F, "mels": mels, "coeffs": coeffs, "mixed": mixed}
    fb = bhw.FilterBank(bhw.mel_weights(nfft, mels, 16000), device="cuda")
    dense = bhw.dct_weights(coeffs, mels)
    dm, dct = bhw.DctMatrix(dense, device="cuda"), torch.from_numpy(dense).cuda()
    kw = dict(win_length=L, fbank=fb)
    lkw = dict(log="db", floor=FLOOR, **kw)
    with bhw.ResidentTable(p) as t:
        G, C, Pm = (torch.empty((nb, F, w), device="cuda") for w in (mels, coeffs, mels))
        bytes_in, out_a, out_b = nb * T * 4, nb * F * mels * 4, nb * F * coeffs * 4
        ha, hb = (bytes_in + out_a) // 8, (bytes_in + out_b) // 8
        src, dst = torch.empty(ha, device="cuda"), torch.empty(ha, device="cuda")
        fns = {}
        logs = bhw.log_spectrogram_mixed if mixed else bhw.log_spectrogram
        mfcc = bhw.mfcc_mixed if mixed else bhw.mfcc
        for form, obj, tab in (("table", t, t), ("library", bhw, None)):
            spec = obj.spectrogram_mixed if mixed else obj.spectrogram
            fns["a_logmel_" + form] = lambda tab=tab: logs(p, x, nfft, hop, out=G, table=tab, **lkw)
            fns["b_mfcc_" + form] = lambda tab=tab: mfcc(p, x, nfft, hop, dct=dm, out=C, table=tab, **lkw)
            fns["c_bank_" + form] = lambda spec=spec: spec(p, x, nfft, hop, out=Pm, **kw)
            fns["d_bank_torch_log_" + form] = lambda spec=spec: 10.0 * torch.log10(torch.clamp(spec(p, x, nfft, hop, out=Pm, **kw), min=FLOOR))
            fns["e_bank_torch_log_dct_" + form] = lambda spec=spec: torch.matmul(10.0 * torch.log10(torch.clamp(spec(p, x, nfft, hop, out=Pm, **kw), min=FLOOR)), dct)
        fns["f_copy_of_a_bytes"] = lambda: dst.copy_(src)
        fns["f_copy_of_b_bytes"] = lambda: dst[:hb].copy_(src[:hb])
        r = timed(fns, steps, reps)
        s = B.make_stft(nb, T, F, hop, nfft, col0=(nfft - L) // 2, pad=nfft // 2, pad_mode=B.PAD_REFLECT, shift=p.dat_width - 1)
        describe = B.describe_logspec_mfft if mixed else B.describe_logspec
        rec["plan_logmel"] = describe(p, L, s, B.make_logspec(FLOOR, DB), fbank=fb.descriptor, table=t.handle)
        rec["plan_mfcc"] = describe(p, L, s, B.make_logspec(FLOOR, DB, coeffs=coeffs, dct_rows=mels), fbank=fb.descriptor, table=t.handle)
    m = {k: q["median_ms"] for k, q in r.items()}
    spread = {k: (q["max_ms"] - q["min_ms"]) / q["median_ms"] for k, q in r.items()}
    rec.update({"times": r, "spread": spread, "bytes_in": bytes_in, "bytes_out_logmel": out_a, "bytes_out_mfcc": out_b})
    for form in ("table", "library"):
        a, b, c, d, e = (m[k + form] for k in ("a_logmel_", "b_mfcc_", "c_bank_", "d_bank_torch_log_", "e_bank_torch_log_dct_"))
        rec["ratios_" + form] = {"a_over_d": a / d, "b_over_e": b / e, "a_over_c": a / c, "b_over_c": b / c,
                                 "a_over_copy": a / m["f_copy_of_a_bytes"], "b_over_copy": b / m["f_copy_of_b_bytes"]}
        # an aim is met when the fused route's slowest step is below the other route's fastest one
        rec["verdict_" + form] = {
            "a_below_d": r["a_logmel_" + form]["max_ms"] < r["d_bank_torch_log_" + form]["min_ms"],
            "b_below_e": r["b_mfcc_" + form]["max_ms"] < r["e_bank_torch_log_dct_" + form]["min_ms"],
            "a_within_c_spread": a <= c * (1.0 + spread["c_bank_" + form]),
            "b_within_c_spread": b <= c * (1.0 + spread["c_bank_" + form])}
    return rec


def resources():
    path = os.path.join(ROOT, "blackman_harris_win_amd", "kernel_resources.json")
    if not os.path.exists(path):
        return []
    with open(path) as f:
        res = json.load(f)
    out = {}
    for k, q in res.items():
        fam = k.split("<")[0]
        if fam.startswith(("k_logspec", "k_spectrogram", "k_stft_mfft")):
            key = json.dumps({"family": fam, **{n: q.get(n) for n in ("VGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy")}},
                             sort_keys=True)
            out[key] = out.get(key, 0) + 1
    return [dict(json.loads(k), instances=n) for k, n in sorted(out.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r40_logspec.json"))
    ap.add_argument("--tests", default=None, help="the JSON record of tests/test_gpu_logspec.py (BHW_LOGSPEC_RECORD)")
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written")
    a = ap.parse_args()
    steps, reps = (2, 3) if a.quick else (a.steps, a.reps)
    ramp()
    rec = {"device": torch.cuda.get_device_name(0), "steps": steps, "reps": reps, "legs": [], "kernel_resources": resources()}
    for name, (p, nb, T, L, nfft, hop, mels) in legs().items():
        rec["legs"].append(leg(name, p, nb, T, L, nfft, hop, mels, steps, reps))
        torch.cuda.empty_cache()
    if a.tests and os.path.exists(a.tests):
        with open(a.tests) as f:
            rec["tests"] = json.load(f)
    print(json.dumps(rec))
    if not a.quick:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
