#!/usr/bin/env python3
"""Weighted overlap-add (bhw_overlap_add_device / bhw_overlap_add_from_table) on one GPU, one process.  Prints one JSON record.

Legs: S1 STFT synthesis (BH-7, 2^12, 32 bits, hop N/4, 2^14 frames), S2 (Hann, 2^16, 24 bits, hop N/2, 2^10
frames), S3 I/Q (BH-4, 2^14, 16 bits, hop N/2, 2^11 frames, two channels), S4 long window (BH-7, 2^22, 32 bits, hop N/2, 16 frames).
Each leg times the library call and the from-table call against, in the same process:
  (a) torch: w = bhw.generate(p, 0, N) once, then the int64 products, index_add_ into the signal, the shift and the int32 cast
  (c) the copy floor: a kernel that reads the same y bytes and writes the same x bytes (the frames' first hop columns copied out
      contiguously, plus a max over 1024-element rows of y that reads all of it), standing for the traffic with no arithmetic.
Every variant is warmed, then timed in steps of `reps` (>= 20) back-to-back calls between device events, the variants alternated
step by step; times are per call (median and spread over --steps).  Counted bytes = y read (frames N C 4) + x written (count C 4);
the rate on them and its fraction of 8 TB/s are reported per variant.

    python tools/bench_overlap_add.py [--steps 10] [--reps 20] [--out FILE] [--quick]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import blackman_harris_win_amd as bhw  # noqa: E402
from blackman_harris_win_amd import binding as B  # noqa: E402

PEAK = 8e12


def timed(fns, steps, reps, warm=3):
    """{name: per-call stats} of call functions, `reps` calls per step, the variants alternated step by step."""
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
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "steps": steps, "reps": reps} for k, v in ts.items()}


def run_leg(name, p, hop, frames, C, steps, reps, baselines=True):
    N = 1 << p.phi_width
    shift = p.dat_width - 1
    dev = torch.cuda.current_device()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(1)
    y = torch.randint(-2 ** 31, 2 ** 31, (frames, N * C), dtype=torch.int64, device="cuda", generator=g).int()
    ext = (frames - 1) * hop + N
    x = torch.empty((ext, C), dtype=torch.int32, device="cuda")
    o = B.make_ola(frames, hop, ext, channels=C, shift=shift)
    L = B.lib()
    py, px, po, pp = ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(x.data_ptr()), ctypes.byref(o), ctypes.byref(p)
    table = bhw.ResidentTable(p)
    fns = {"library": lambda: L.bhw_overlap_add_device(pp, dev, st, po, py, px),
           "from_table": lambda: L.bhw_overlap_add_from_table(table.handle, pp, st, po, py, px)}
    plans = {"library": B.describe_ola(p, frames, hop, channels=C), "from_table": table.describe_overlap_add(p, frames, hop, channels=C)}
    for k, fn in fns.items():
        x.fill_(0)
        B.check(fn())
        if k == "library":
            ref = x.clone()
        else:
            assert torch.equal(x, ref), (name, k)
    if baselines:
        w = bhw.generate(p, 0, N).long()
        idx = (torch.arange(frames, device="cuda")[:, None] * hop + torch.arange(N, device="cuda")[None, :]).reshape(-1)
        acc = torch.empty((ext, C), dtype=torch.int64, device="cuda")

        def torch_route():
            acc.zero_()
            acc.index_add_(0, idx, (y.view(frames, N, C).long() * w[None, :, None]).view(-1, C))
            return (acc >> shift).int()

        assert torch.equal(torch_route(), ref), name
        fns["torch_route"] = torch_route
        # copy floor: x (ext C int32) written once from y's first columns, and every y element read once
        cols = min(hop, N)
        head = y.view(frames, N * C)[:, :cols * C]
        xs = x.view(-1)
        n_head = min(frames * cols * C, xs.numel())
        yrows = y.view(-1, 1024)                                 # the reduction over short rows: enough workgroups for any leg
        sink = torch.empty((yrows.shape[0],), dtype=torch.int32, device="cuda")

        def copy_floor():
            xs[:n_head].view(-1, cols * C)[: n_head // (cols * C)].copy_(head[: n_head // (cols * C)])
            if n_head < xs.numel():
                xs[n_head:].fill_(0)
            torch.amax(yrows, dim=1, out=sink)

        fns["copy_floor"] = copy_floor
    res = timed(fns, steps, reps)
    counted = frames * N * C * 4 + ext * C * 4
    for r in res.values():
        r["rate_TBps"] = counted / (r["median_ms"] * 1e-3) / 1e12
        r["frac_of_8TBps"] = r["rate_TBps"] * 1e12 / PEAK
    table.close()
    rec = {"window": p.win_type, "N": N, "dat_width": p.dat_width, "hop": hop, "frames": frames, "channels": C, "count": ext,
           "counted_bytes": counted, "plans": plans, "times": res}
    if baselines:
        rec["notes"] = {"copy_floor": "x written from the frames' first hop columns (zero fill past them) plus a max over "
                                      "1024-element rows of y: y read once (its first hop columns twice), x written once, two launches"}
    print(name, {k: round(v["median_ms"] * 1e3, 1) for k, v in res.items()}, "us", file=sys.stderr)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="no baselines (the profiler pass)")
    a = ap.parse_args()
    reps = max(20, a.reps)
    res = {"device": torch.cuda.get_device_name(0), "reps_per_step": reps, "peak_TBps": PEAK / 1e12, "legs": {}}
    legs = [("S1_stft", B.make_params(B.WIN_BH7, 12, 32), 1 << 10, 1 << 14, 1),
            ("S2_hann", B.make_params(B.WIN_HANN, 16, 24), 1 << 15, 1 << 10, 1),
            ("S3_iq", B.make_params(B.WIN_BH4, 14, 16), 1 << 13, 1 << 11, 2),
            ("S4_long", B.make_params(B.WIN_BH7, 22, 32), 1 << 21, 16, 1)]
    for name, p, hop, frames, C in legs:
        res["legs"][name] = run_leg(name, p, hop, frames, C, a.steps, reps, baselines=not a.quick)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
