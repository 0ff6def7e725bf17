#!/usr/bin/env python3
"""Welch cross spectra (bhw_welch_csd_f32 / bhw.cross_spectra) on one GPU, one process.  Prints one JSON record and writes it to --out
(profiles/r13_csd.json by default).

Legs, on section 15's periodogram shapes with X and Y of that shape each:
  T1          (64, 998, 257)     the rfft of 64 signals of 160 000 samples, 400 in 512 / hop 160
  T2          (1, 16 381, 2049)  the rfft of one signal of 2^24 samples, 4096 / hop 1024
  one block   (64, 200, 257)
  T1 bcast    T1 with X one signal (998, 257) paired with each of Y's 64
Per leg: csd_full (all five outputs), csd_pxy (P_xy alone: the two-chain kernel); two_psd (bhw.welch_psd of X, then of Y: the same bytes
read by the parent's code -- the yardstick, target <= 1.15 x); torch_sum (torch.view_as_real sums over both tensors: the read floor);
torch_full and torch_pxy (the torch route for the same outputs: (X.conj() * Y).mean(1), two abs() ** 2 ... mean, the coherence and
H1 expressions).
End to end: ResidentTable.cross_spectra on section 15's T1 / T2 signals (y = x delayed and scaled + noise) against the torch-only
route, with the one FFT call over both signals' segments alone.
Accuracy: the figures of tests/test_gpu_csd.py's two end-to-end tests, three seeds each.
Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events, the variants of a leg alternated
step by step; times are per call (median, min, max over --steps).

    python tools/bench_csd.py [--steps 10] [--reps 20] [--out FILE] [--quick] [--no-accuracy]
    python tools/bench_csd.py --ab ROOT     one JSON line: welch_psd on section 15's legs from the package under ROOT
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

ALL = ("pxy", "pxx", "pyy", "coherence", "h1")
SHAPES = {"T1": (64, 998, 257, 512), "T2": (1, 16381, 2049, 4096), "one block": (64, 200, 257, 512)}


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


def ramp():
    """A second of work in front of the timed region: the clock has ramped when the first leg starts."""
    a = torch.randn((4096, 4096), device="cuda")
    for _ in range(40):
        a = (a @ a).clamp_(-1, 1)
    torch.cuda.synchronize()


def spectra(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.view_as_complex(torch.randn(tuple(shape) + (2,), device="cuda", generator=g))


def ab_main(steps, reps):
    """welch_psd on section 15's three periodogram shapes: a call both trees have."""
    assert os.path.abspath(bhw.__file__).startswith(os.path.abspath(AB)), bhw.__file__
    ramp()
    out = {"root": os.path.abspath(AB)}
    for name, (nb, F, K, nfft) in SHAPES.items():
        Y = spectra((nb, F, K), 1)
        P = torch.empty((nb, K), device="cuda")
        ws = torch.empty(max(nb * -(-F // 256) * K, 1), dtype=torch.float64, device="cuda")
        r = timed({"welch_psd": lambda: bhw.welch_psd(Y, 1.0 / F, nfft=nfft, out=P, workspace=ws if F > 256 else None)}, steps, reps)
        out[name] = r["welch_psd"]["median_ms"] * 1000
        del Y
    print(json.dumps(out))


def torch_outputs(X, Y, full):
    """The torch route for the same outputs."""
    C = (X.conj() * Y).mean(1)
    if not full:
        return C
    Pxx, Pyy = (X.abs() ** 2).mean(1), (Y.abs() ** 2).mean(1)
    return C, Pxx, Pyy, C.abs() ** 2 / (Pxx * Pyy), C / Pxx


def csd_leg(name, X, Y, nfft, steps, reps):
    nb, F, K = Y.shape
    bc = X.dim() == 2
    scale = 1.0 / F
    outs = {n: torch.empty((nb, K), device="cuda", dtype=torch.complex64 if B.CSD_OUTPUTS[n][1] else torch.float32) for n in ALL}
    d = B.make_csd(nb, F, K, nfft, scale, outputs=ALL, onesided=True, broadcast_x=bc)
    d2 = B.make_csd(nb, F, K, nfft, scale, outputs=("pxy",), onesided=True, broadcast_x=bc)
    need = int(B.lib().bhw_welch_csd_workspace_bytes(ctypes.byref(d))) // 8
    ws = torch.empty(max(need, 1), dtype=torch.float64, device="cuda")
    Xp = X if not bc else X.unsqueeze(0)
    Px, Py = torch.empty((Xp.shape[0], K), device="cuda"), torch.empty((nb, K), device="cuda")
    wsn = ws if need else None
    Xe = X if not bc else X.expand(nb, F, K)                         # the torch routes broadcast a view

    def two_psd():
        bhw.welch_psd(Xp, scale, nfft=nfft, out=Px, workspace=wsn)
        bhw.welch_psd(Y, scale, nfft=nfft, out=Py, workspace=wsn)

    r = timed({"csd_full": lambda: bhw.welch_csd(X, Y, scale, nfft=nfft, outputs=ALL, out=outs, workspace=wsn),
               "csd_pxy": lambda: bhw.welch_csd(X, Y, scale, nfft=nfft, outputs=("pxy",), out={"pxy": outs["pxy"]}, workspace=wsn),
               "two_psd": two_psd,
               "torch_sum": lambda: (torch.view_as_real(Xp).sum(1), torch.view_as_real(Y).sum(1)),
               "torch_full": lambda: torch_outputs(Xe, Y, True),
               "torch_pxy": lambda: torch_outputs(Xe, Y, False)}, steps, reps)
    m = {k: v["median_ms"] for k, v in r.items()}
    nbytes = (Xp.numel() + Y.numel()) * 8
    return {"leg": name, "B": nb, "F": F, "K": K, "x_broadcast": bc, "bytes": nbytes, "plan_full": B.describe_csd(d), "plan_pxy": B.describe_csd(d2),
            "times": r, "target": 1.15,
            "full_over_two_psd": m["csd_full"] / m["two_psd"], "full_met": m["csd_full"] <= 1.15 * m["two_psd"],
            "pxy_over_two_psd": m["csd_pxy"] / m["two_psd"], "pxy_met": m["csd_pxy"] <= 1.15 * m["two_psd"],
            "full_over_torch_sum": m["csd_full"] / m["torch_sum"], "pxy_over_torch_sum": m["csd_pxy"] / m["torch_sum"],
            "torch_full_over_csd_full": m["torch_full"] / m["csd_full"], "torch_pxy_over_csd_pxy": m["torch_pxy"] / m["csd_pxy"],
            "csd_full_GBps": nbytes / m["csd_full"] / 1e6, "csd_pxy_GBps": nbytes / m["csd_pxy"] / 1e6}


def torch_cross(x, y, w, L, nfft, hop, scale):
    def spec(t):
        seg = t.unfold(-1, L, hop)
        return torch.fft.rfft((seg - seg.mean(-1, keepdim=True)) * w, n=nfft)
    X, Y = spec(x), spec(y)
    d = torch.full((nfft // 2 + 1,), 2.0 * scale, device=x.device)
    d[0] = scale
    if nfft % 2 == 0:
        d[-1] = scale
    C = (X.conj() * Y).mean(-2)
    Pxx, Pyy = (X.abs() ** 2).mean(-2), (Y.abs() ** 2).mean(-2)
    return C * d, Pxx * d, Pyy * d, C.abs() ** 2 / (Pxx * Pyy), C / Pxx


def end_to_end_leg(name, p, nb, T, L, nfft, hop, steps, reps):
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn((nb, T), device="cuda", generator=g) + 3.0
    y = 0.5 * torch.roll(x, 3, -1) + 0.1 * torch.randn((nb, T), device="cuda", generator=g) - 1.0
    w = bhw.window(p, L, dtype=torch.float32)
    scale = float(1.0 / (w.double() ** 2).sum())
    F = 1 + (T - L) // hop
    with bhw.ResidentTable(p) as t:
        t.cross_spectra(p, x, y, length=L, noverlap=L - hop, nfft=nfft)
        seg = torch.empty((2 * nb, F, nfft), device="cuda")
        t.welch_frames(p, x, L, hop, nfft=nfft, out=seg[:nb])
        t.welch_frames(p, y, L, hop, nfft=nfft, out=seg[nb:])
        r = timed({"cross_spectra_table": lambda: t.cross_spectra(p, x, y, length=L, noverlap=L - hop, nfft=nfft),
                   "csd_table": lambda: t.csd(p, x, y, length=L, noverlap=L - hop, nfft=nfft),
                   "torch": lambda: torch_cross(x, y, w, L, nfft, hop, scale),
                   "rfft_alone": lambda: torch.fft.rfft(seg, dim=-1)}, steps, reps)
    m = {k: v["median_ms"] for k, v in r.items()}
    return {"leg": name, "B": nb, "T": T, "L": L, "nfft": nfft, "hop": hop, "frames": F, "times": r,
            "torch_over_cross_spectra": m["torch"] / m["cross_spectra_table"], "fft_share": m["rfft_alone"] / m["cross_spectra_table"],
            "cross_spectra_without_fft_ms": m["cross_spectra_table"] - m["rfft_alone"], "torch_without_fft_ms": m["torch"] - m["rfft_alone"]}


def accuracy():
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_csd as TC
    p = B.make_params(B.WIN_BH7, 16, 32)
    out = []
    for L, nov, nfft in ((4096, 2048, 4096), (400, 240, 512)):
        vh = TC._v(p, L)
        v = torch.from_numpy(vh).cuda()
        for seed in (5, 6, 7):
            for what, strong in (("csd", 1e3), ("coherence", 4.0)):
                xh, yh = TC._pair(200000, seed, strong)
                x, y = torch.from_numpy(xh).cuda(), torch.from_numpy(yh).cuda()
                _, Pref, Cref = TC._cross_ref64(xh, yh, vh, 1.0, L, nov, nfft)
                Py, Cy = TC._torch_route(torch, x, y, v, 1.0, L, nov, nfft)
                if what == "csd":
                    _, P = bhw.csd(p, x, y, 1.0, length=L, noverlap=nov, nfft=nfft)
                    top = np.abs(Pref).max()
                    err = float(np.abs(P.cpu().numpy().astype(np.complex128) - Pref).max() / top)
                    yard = float(np.abs(Py.cpu().numpy().astype(np.complex128) - Pref).max() / top)
                else:
                    _, C = bhw.coherence(p, x, y, 1.0, length=L, noverlap=nov, nfft=nfft)
                    err = float(np.abs(C.cpu().numpy().astype(np.float64) - Cref).max())
                    yard = float(np.abs(Cy.cpu().numpy().astype(np.float64) - Cref).max())
                out.append({"what": what, "L": L, "noverlap": nov, "nfft": nfft, "T": 200000, "seed": seed, "strong_tone": strong,
                            "bhw_err": err, "torch_route_err": yard, "ratio": err / yard, "bound": 2.0, "met": err <= 2.0 * yard})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_csd.json"))
    ap.add_argument("--quick", action="store_true", help="2 steps of 3 calls, no accuracy leg, no file written (a profiler run)")
    ap.add_argument("--no-accuracy", action="store_true")
    ap.add_argument("--ab", default=None)
    a = ap.parse_args()
    steps, reps = (2, 3) if a.quick else (a.steps, a.reps)
    if a.ab:
        return ab_main(steps, reps)
    ramp()
    rec = {"device": torch.cuda.get_device_name(0), "steps": steps, "reps": reps, "csd": [], "end_to_end": []}
    for name, (nb, F, K, nfft) in SHAPES.items():
        X, Y = spectra((nb, F, K), 1), spectra((nb, F, K), 2)
        rec["csd"].append(csd_leg(name, X, Y, nfft, steps, reps))
        if name == "T1":
            rec["csd"].append(csd_leg("T1 bcast", X[0].contiguous(), Y, nfft, steps, reps))
        del X, Y
        torch.cuda.empty_cache()
    rec["end_to_end"].append(end_to_end_leg("T1", B.make_params(B.WIN_BH4, 24, 32), 64, 160000, 400, 512, 160, steps, reps))
    torch.cuda.empty_cache()
    rec["end_to_end"].append(end_to_end_leg("T2", B.make_params(B.WIN_BH7, 12, 32), 1, 1 << 24, 4096, 4096, 1024, steps, reps))
    if not a.quick and not a.no_accuracy:
        rec["accuracy"] = accuracy()
    print(json.dumps(rec))
    if not a.quick:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
