#!/usr/bin/env python3
"""Overlapped-frame apply (bhw_apply_frames_device / bhw_apply_frames_from_table) on one GPU, one process.  Prints one JSON record.

Legs: L1 STFT (BH-7, 2^12, 32 bits, hop N/4, 2^14 frames), L2 Welch (Nuttall, 2^16, 24 bits, hop N/2, 2^10
frames), L3 I/Q (BH-4, 2^14, 16 bits, hop N/2, 2^11 frames, two channels), L4 long window (BH-7, 2^22, 32 bits, hop N/2, 1/2/4/16
frames, both routes forced: it sets the planner's crossover), plus the same crossover sweep at 2^18 and 2^20.  Each leg times the
library call and the from-table call against, in the same process:
  (a) torch: w = bhw.generate(p, 0, N) once, then ((x framed).long() * w >> shift).int()
  (b) one bhw_apply_device per frame, all of them captured in one graph (L1: the first 1 024 frames, scaled to the leg's count;
      none for L3: the existing apply has no I/Q form)
  (c) the copy floor: the framed x made contiguous -- the same reads and writes with no arithmetic.
Every variant is warmed, then timed in steps of `reps` (>= 20) back-to-back calls between device events, the variants alternated
step by step; times are per call (median and spread over --steps).  Counted bytes = y written (frames N C 4) + distinct x read
(((frames - 1) hop + N) C 4); the rate on them and its fraction of 8 TB/s are reported per variant.

    python tools/bench_apply_frames.py [--steps 10] [--reps 20] [--out FILE] [--quick]
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
DIRECT, PER_FRAME = 0, 2            # forced routes of bhw_dbg_apply_frames_route (bhw_plan.h)


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


def run_leg(name, p, hop, frames, C, steps, reps, per_frame_limit=None, routes=False, baselines=True):
    N = 1 << p.phi_width
    shift = p.dat_width - 1
    dev = torch.cuda.current_device()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randint(-2 ** 31, 2 ** 31, (((frames - 1) * hop + N) * C,), dtype=torch.int64, device="cuda", generator=g).int()
    y = torch.empty((frames, N * C), dtype=torch.int32, device="cuda")
    f = B.make_frames(frames, hop, channels=C, shift=shift)
    L = B.lib()
    px, py, pf, pp = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.byref(f), ctypes.byref(p)
    table = bhw.ResidentTable(p)
    fns, plans = {}, {}
    if routes:
        fns["frames_kernel"] = lambda: L.bhw_dbg_apply_frames_route(pp, dev, st, pf, px, py, DIRECT)
        if C == 1:
            fns["per_frame"] = lambda: L.bhw_dbg_apply_frames_route(pp, dev, st, pf, px, py, PER_FRAME)
    else:
        fns["library"] = lambda: L.bhw_apply_frames_device(pp, dev, st, pf, px, py)
    fns["from_table"] = lambda: L.bhw_apply_frames_from_table(table.handle, pp, st, pf, px, py)
    plans["library"] = B.describe_frames(p, frames, hop, channels=C)
    plans["from_table"] = table.describe_frames(p, frames, hop, channels=C)
    # correctness of the timed calls against each other before timing
    for k, fn in fns.items():
        y.fill_(0)
        B.check(fn())
        if k == next(iter(fns)):
            ref = y.clone()
        else:
            assert torch.equal(y, ref), (name, k)
    notes = {}
    if baselines:
        w = bhw.generate(p, 0, N).long()
        xs = x.as_strided((frames, N, C), (hop * C, C, 1))
        yt = torch.empty((frames, N, C), dtype=torch.int32, device="cuda")

        def torch_route():
            return ((xs.long() * w[None, :, None]) >> shift).int()

        assert torch.equal(((xs.long() * w[None, :, None]) >> shift).int().view(frames, N * C), ref), name
        fns["torch_route"] = torch_route
        fns["copy_floor"] = lambda: yt.copy_(xs)
        if C == 1:
            nf = min(frames, per_frame_limit or frames)
            s = torch.cuda.Stream()
            B.check(L.bhw_prepare_device(pp, dev, ctypes.c_void_p(s.cuda_stream)))   # the capturing stream's own scratch
            s.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=s):
                for i in range(nf):
                    bhw.apply(p, x[i * hop:i * hop + N], shift=shift, out=y[i])
            fns["per_frame_graph"] = graph.replay
            if nf < frames:
                notes["per_frame_graph"] = f"{nf} of {frames} frames per replay; scaled_ms = median x {frames / nf:g}"
        else:
            notes["per_frame_graph"] = "none: bhw_apply_device has no I/Q form"
    res = timed(fns, steps, reps)
    counted = frames * N * C * 4 + ((frames - 1) * hop + N) * C * 4
    for k, r in res.items():
        ms = r["median_ms"]
        if k == "per_frame_graph" and k in notes and "scaled" in notes[k]:
            ms = ms * frames / min(frames, per_frame_limit)
            r["scaled_ms"] = ms
        r["rate_TBps"] = counted / (ms * 1e-3) / 1e12
        r["frac_of_8TBps"] = r["rate_TBps"] * 1e12 / PEAK
    table.close()
    rec = {"window": p.win_type, "N": N, "dat_width": p.dat_width, "hop": hop, "frames": frames, "channels": C,
           "counted_bytes": counted, "plans": plans, "times": res}
    if notes:
        rec["notes"] = notes
    print(name, {k: round(v.get("scaled_ms", v["median_ms"]) * 1e3, 1) for k, v in res.items()}, "us", file=sys.stderr)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="L1-L3 and L4 at 4 frames only, no baselines (the profiler pass)")
    a = ap.parse_args()
    reps = max(20, a.reps)
    res = {"device": torch.cuda.get_device_name(0), "reps_per_step": reps, "peak_TBps": PEAK / 1e12, "legs": {}}
    bh7 = lambda pw, W: B.make_params(B.WIN_BH7, pw, W)  # noqa: E731
    wt, _, aa = B.coeffs_preset("nuttall", 24)
    legs = [("L1_stft", bh7(12, 32), 1 << 10, 1 << 14, 1, 1024),
            ("L2_welch", B.make_params(wt, 16, 24, aa=aa), 1 << 15, 1 << 10, 1, None),
            ("L3_iq", B.make_params(B.WIN_BH4, 14, 16), 1 << 13, 1 << 11, 2, None)]
    for name, p, hop, frames, C, lim in legs:
        res["legs"][name] = run_leg(name, p, hop, frames, C, a.steps, reps, per_frame_limit=lim, baselines=not a.quick)
    for pw in ((22,) if a.quick else (18, 20, 22)):
        for frames in ((4,) if a.quick else (1, 2, 4, 8, 16)):
            if pw == 22 and frames == 8:
                continue
            name = f"L4_long_pw{pw}_f{frames}" if pw == 22 else f"crossover_pw{pw}_f{frames}"
            res["legs"][name] = run_leg(name, bh7(pw, 32), 1 << (pw - 1), frames, 1, a.steps, reps, routes=True,
                                        baselines=not a.quick and pw == 22)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
