#!/usr/bin/env python3
"""Welch's method around the FFT (bhw_welch_frames_f32_* / bhw_welch_psd_f32 / bhw.welch) on one GPU, one process.  Prints one JSON
record and writes it to --out (profiles/r12_welch.json by default).

Legs, on section 14's shapes:
  T1 batch   BH-4, P 24, 32 b; B 64, T 160 000, L 400 in rows of 512, hop 160, no padding (998 segments per signal)
  T2 long    BH-7, P 12, 32 b; B 1, T 2^24, L = nfft 4096, hop 1024 (16 381 segments)
Segments: welch_table / welch_library (constant detrend), welch_flags0 (no detrending: the stft frames kernel), stft_frames (this
tree's stft_frames(center=False) on the same signal), torch (unfold, - mean, * w; zero-padded to nfft where nfft > L).  The budget of
the detrended call is the ratio of bytes moved to the stft frames call -- one more read of each segment for the mean, plus the means --
times 1.15; the ratio to the PARENT commit's stft_frames comes from --ab runs of both trees in alternating processes.
Periodogram, on the rfft of T1's and T2's segments and on a one-block case (B 64, F 200, K 257): welch_psd; torch_sum
(torch.view_as_real(Y).sum(1), a read-once reduction over the same bytes: the yardstick, target <= 1.15 x); copy (Y.clone(): reads and
writes the bytes, listed at half its time); torch (abs() ** 2, mean(1)).
End to end: ResidentTable.welch against the torch-only route (unfold, - mean, * w, rfft, abs() ** 2, mean), with the rfft alone.
Accuracy: the two figures of tests/test_gpu_welch.py::test_welch_end_to_end_within_twice_the_torch_route.
Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events, the variants of a leg alternated
step by step; times are per call (median, min, max over --steps).

    python tools/bench_welch.py [--steps 10] [--reps 20] [--out FILE] [--quick]
    python tools/bench_welch.py --ab ROOT     one JSON line: stft_frames(center=False) and section 14's calls from the package under ROOT
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB = sys.argv[sys.argv.index("--ab") + 1] if "--ab" in sys.argv else None
sys.path.insert(0, os.path.abspath(AB) if AB else ROOT)
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
    return {"T1": (B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 400, 512, 160),
            "T2": (B.make_params(B.WIN_BH7, 12, 32), 1, 1 << 24, 4096, 4096, 1024)}


def ramp():
    """A second of work in front of the timed region: the clock has ramped when the first leg starts."""
    a = torch.randn((4096, 4096), device="cuda")
    for _ in range(40):
        a = (a @ a).clamp_(-1, 1)
    torch.cuda.synchronize()


def ab_main(steps, reps):
    """stft_frames(center=False) on the Welch legs' signals and section 14's centred frames and overlap-add: calls both trees have."""
    assert os.path.abspath(bhw.__file__).startswith(os.path.abspath(AB)), bhw.__file__
    ramp()
    out = {"root": os.path.abspath(AB)}
    g = torch.Generator(device="cuda").manual_seed(1)
    for name, (p, nb, T, L, nfft, hop) in legs().items():
        x = torch.randn((nb, T), device="cuda", generator=g)
        with bhw.ResidentTable(p) as t:
            y0 = t.stft_frames(p, x, nfft, hop, win_length=L, center=False)
            y1 = t.stft_frames(p, x, nfft, hop, win_length=L)
            xo = torch.empty_like(x)
            r = timed({"stft_frames_center_off": lambda: t.stft_frames(p, x, nfft, hop, win_length=L, center=False, out=y0),
                       "stft_frames_centred": lambda: t.stft_frames(p, x, nfft, hop, win_length=L, out=y1),
                       "istft_overlap_add": lambda: t.istft_overlap_add(p, y1, nfft, hop, win_length=L, length=T, out=xo)}, steps, reps)
        out[name] = {k: v["median_ms"] * 1000 for k, v in r.items()}
        out[name]["frames_center_off"] = y0.shape[1]
        del x, y0, y1, xo
    print(json.dumps(out))


def torch_segments(x, w, L, nfft, hop):
    seg = x.unfold(-1, L, hop)
    seg = (seg - seg.mean(-1, keepdim=True)) * w
    return torch.nn.functional.pad(seg, (0, nfft - L)) if nfft > L else seg


def torch_welch(x, w, L, nfft, hop, scale):
    seg = x.unfold(-1, L, hop)
    seg = (seg - seg.mean(-1, keepdim=True)) * w
    P = (torch.fft.rfft(seg, n=nfft).abs() ** 2).mean(-2) * scale
    P[..., 1:] *= 2.0
    if nfft % 2 == 0:
        P[..., -1] /= 2.0
    return P


def segments_leg(name, p, nb, T, L, nfft, hop, steps, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((nb, T), device="cuda", generator=g) + 3.0
    F = 1 + (T - L) // hop
    y = torch.empty((nb, F, nfft), device="cuda")
    ws = torch.empty(nb * F, device="cuda")
    w = bhw.window(p, L, dtype=torch.float32)
    with bhw.ResidentTable(p) as t:
        ys = t.stft_frames(p, x, nfft, hop, win_length=L, center=False)
        assert torch.equal(t.welch_frames(p, x, L, hop, nfft=nfft), bhw.welch_frames(p, x, L, hop, nfft=nfft))
        r = timed({"welch_table": lambda: t.welch_frames(p, x, L, hop, nfft=nfft, out=y, workspace=ws),
                   "welch_library": lambda: bhw.welch_frames(p, x, L, hop, nfft=nfft, out=y, workspace=ws),
                   "welch_flags0": lambda: t.welch_frames(p, x, L, hop, nfft=nfft, detrend=False, out=y),
                   "stft_frames": lambda: t.stft_frames(p, x, nfft, hop, win_length=L, center=False, out=ys),
                   "torch": lambda: torch_segments(x, w, L, nfft, hop)}, steps, reps)
        desc = B.describe_welch(p, L, stft=B.make_stft(nb, T, F, hop, nfft, shift=p.dat_width - 1), detrend=True, table=t.handle)
    rows = nb * F
    b_stft, b_welch = rows * (L + nfft) * 4, rows * (2 * L + nfft) * 4 + rows * 2 * 4
    rec = {"leg": name, "B": nb, "T": T, "L": L, "nfft": nfft, "hop": hop, "frames": F, "frames_stft_center_off": ys.shape[1], "plan": desc,
           "bytes_stft_frames": b_stft, "bytes_welch_detrend": b_welch, "bytes_ratio": b_welch / b_stft, "budget_ratio": 1.15 * b_welch / b_stft,
           "times": r}
    m = {k: v["median_ms"] for k, v in r.items()}
    per_row_stft = m["stft_frames"] / (nb * ys.shape[1])
    rec["ratio_to_stft_frames_this_tree_per_row"] = (m["welch_table"] / rows) / per_row_stft
    rec["flags0_to_stft_frames_per_row"] = (m["welch_flags0"] / rows) / per_row_stft
    rec["torch_over_welch"] = m["torch"] / m["welch_table"]
    rec["welch_GBps"] = b_welch / m["welch_table"] / 1e6
    return rec


def psd_leg(name, Y, nfft, steps, reps):
    nb, F, K = Y.shape
    P = torch.empty((nb, K), device="cuda")
    d = B.make_psd(nb, F, K, nfft, 1.0 / F, onesided=True)
    need = int(B.lib().bhw_welch_psd_workspace_bytes(ctypes.byref(d))) // 8
    ws = torch.empty(max(need, 1), dtype=torch.float64, device="cuda")
    Yc = torch.empty_like(Y)
    r = timed({"welch_psd": lambda: bhw.welch_psd(Y, 1.0 / F, nfft=nfft, out=P, workspace=ws if need else None),
               "torch_sum": lambda: torch.view_as_real(Y).sum(1),
               "copy": lambda: Yc.copy_(Y),
               "torch": lambda: (Y.abs() ** 2).mean(1)}, steps, reps)
    m = {k: v["median_ms"] for k, v in r.items()}
    nbytes = Y.numel() * 8
    return {"leg": name, "B": nb, "F": F, "K": K, "bytes": nbytes, "plan": B.describe_welch(psd=d), "times": r,
            "ratio_to_torch_sum": m["welch_psd"] / m["torch_sum"], "target": 1.15, "met": m["welch_psd"] <= 1.15 * m["torch_sum"],
            "half_copy_ms": m["copy"] / 2, "torch_over_welch_psd": m["torch"] / m["welch_psd"], "welch_psd_GBps": nbytes / m["welch_psd"] / 1e6}


def end_to_end_leg(name, p, nb, T, L, nfft, hop, steps, reps):
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn((nb, T), device="cuda", generator=g) + 3.0
    w = bhw.window(p, L, dtype=torch.float32)
    scale = float(1.0 / (w.double() ** 2).sum())
    with bhw.ResidentTable(p) as t:
        t.welch(p, x, length=L, noverlap=L - hop, nfft=nfft)
        seg = t.welch_frames(p, x, L, hop, nfft=nfft)
        r = timed({"welch_table": lambda: t.welch(p, x, length=L, noverlap=L - hop, nfft=nfft),
                   "torch": lambda: torch_welch(x, w, L, nfft, hop, scale),
                   "rfft_alone": lambda: torch.fft.rfft(seg, dim=-1)}, steps, reps)
    m = {k: v["median_ms"] for k, v in r.items()}
    return {"leg": name, "times": r, "torch_over_welch": m["torch"] / m["welch_table"],
            "welch_without_fft_ms": m["welch_table"] - m["rfft_alone"], "torch_without_fft_ms": m["torch"] - m["rfft_alone"]}


def accuracy():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_welch as TW
    p = B.make_params(B.WIN_BH7, 16, 32)
    xh = TW._test_signal(200000, 5)
    x = torch.from_numpy(xh).cuda()
    out = []
    for L, nov, nfft in ((4096, 2048, 4096), (400, 240, 512)):
        vh = TW._v(p, L)
        _, ref = TW._welch_ref64(xh, vh, 1.0, L, nov, nfft, True)
        _, P = bhw.welch(p, x, 1.0, length=L, noverlap=nov, nfft=nfft)
        yard = TW._rel_err(TW._torch_route(torch, x, torch.from_numpy(vh).cuda(), 1.0, L, nov, nfft).cpu().numpy(), ref)
        err = TW._rel_err(P.cpu().numpy(), ref)
        out.append({"L": L, "noverlap": nov, "nfft": nfft, "T": 200000, "bhw_welch_rel_err": err, "torch_route_rel_err": yard,
                    "ratio": err / yard, "bound": 2.0, "met": err <= 2.0 * yard})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_welch.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no file written (a profiler run)")
    ap.add_argument("--ab", default=None)
    a = ap.parse_args()
    steps, reps = (2, 3) if a.quick else (a.steps, a.reps)
    if a.ab:
        return ab_main(steps, reps)
    ramp()
    rec = {"device": torch.cuda.get_device_name(0), "steps": steps, "reps": reps, "segments": [], "psd": [], "end_to_end": []}
    for name, (p, nb, T, L, nfft, hop) in legs().items():
        rec["segments"].append(segments_leg(name, p, nb, T, L, nfft, hop, steps, reps))
        seg = bhw.welch_frames(p, torch.randn((nb, T), device="cuda"), L, hop, nfft=nfft)
        Y = torch.fft.rfft(seg, dim=-1)
        del seg
        rec["psd"].append(psd_leg(name + " rfft", Y, nfft, steps, reps))
        if name == "T1":
            rec["psd"].append(psd_leg("one block", Y[:, :200].contiguous(), nfft, steps, reps))
        del Y
        rec["end_to_end"].append(end_to_end_leg(name, p, nb, T, L, nfft, hop, steps, reps))
        torch.cuda.empty_cache()
    for s in rec["segments"]:
        s["met_against_this_tree"] = s["ratio_to_stft_frames_this_tree_per_row"] <= s["budget_ratio"]
    rec["accuracy"] = accuracy()
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec))
    if not a.quick:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
