#!/usr/bin/env python3
"""Windows of any length (bhw_*_len_*) on one GPU, one process.  Prints one JSON record and writes it to --out
(profiles/r09_len.json by default).

Legs, each next to a reference leg run in the same process:
  G1  generate_len, library, BH-7 / 32 bits, L = 2^20 - 1            vs  generate(ALGO_DIRECT) at N = 2^20 (the same K - 1 chains per
                                                                          coefficient): per-coefficient ratio
  G2  generate_len_from_table, BH-7 / 32 bits, L = 3 * 2^24, P = 26  vs  generate_from_table over a ragged range of the same count
                                                                          (no whole period: k_range_combine, the existing gather)
  F1  apply_frames_len_from_table, BH-7 / 32 bits, L = 400, P = 24,  vs  a plain framed copy of the same bytes (torch as_strided copy:
      hop 160, 2^16 frames                                                x read frame by frame, y written)
  O1  overlap_add_len_from_table, the same shape                      vs  the copy floor: y read once (amax over its rows) and the
                                                                          outputs written (a copy of the frames' first hop columns)
  F1 / O1 library: the library calls of the same shape, reported as measured.
Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events, the variants of a leg alternated step
by step; times are per call (median, min, max over --steps).  Counted bytes per leg are listed with the rates.

    python tools/bench_len.py [--steps 10] [--reps 20] [--out FILE] [--quick]
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


def rates(res, nbytes):
    for k, v in res.items():
        if k in nbytes:
            v["bytes"] = nbytes[k]
            v["TBps"] = nbytes[k] / (v["median_ms"] * 1e-3) / 1e12
            v["of_peak"] = v["TBps"] * 1e12 / PEAK
    return res


def leg_g1(steps, reps, quick):
    P = 16 if quick else 20
    p = B.make_params(B.WIN_BH7, P, 32)
    N, L = 1 << P, (1 << P) - 1
    out = torch.empty(N, dtype=torch.int32, device="cuda")
    dev, st, lib = torch.cuda.current_device(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), B.lib()
    ex = B.BhwExec()
    ex.struct_size, ex.algo = ctypes.sizeof(B.BhwExec), B.ALGO_DIRECT
    po, pp = ctypes.c_void_p(out.data_ptr()), ctypes.byref(p)
    fns = {"generate_len": lambda: lib.bhw_generate_len_device(pp, L, dev, st, 0, L, po),
           "direct_pow2": lambda: lib.bhw_generate_device_ex(pp, dev, st, 0, N, po, ctypes.byref(ex))}
    for f in fns.values():
        B.check(f())
    r = rates(timed(fns, steps, reps), {"generate_len": 4 * L, "direct_pow2": 4 * N})
    ratio = (r["generate_len"]["median_ms"] / L) / (r["direct_pow2"]["median_ms"] / N)
    return {"leg": "G1", "config": f"BH-7 / 32 bits, L = 2^{P} - 1 vs N = 2^{P}", "plan": B.describe_len(p, L), "results": r,
            "per_coefficient_ratio": ratio, "target": 1.15}


def leg_g2(steps, reps, quick):
    P = 20 if quick else 26
    p = B.make_params(B.WIN_BH7, P, 32)
    L = 3 << (P - 2)
    out = torch.empty(L, dtype=torch.int32, device="cuda")
    st, lib = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), B.lib()
    po, pp = ctypes.c_void_p(out.data_ptr()), ctypes.byref(p)
    with bhw.ResidentTable(p) as t:
        h = t.handle
        fns = {"generate_len_from_table": lambda: lib.bhw_generate_len_from_table(h, pp, L, st, 0, L, po),
               "range_combine_ragged": lambda: lib.bhw_generate_from_table(h, pp, st, 1, L, po)}
        for f in fns.values():
            B.check(f())
        r = rates(timed(fns, steps, reps), {k: 4 * L for k in fns})
        plans = {"generate_len_from_table": B.describe_len(p, L, table=h), "range_combine_ragged": t.describe(p, 1, L)}
    return {"leg": "G2", "config": f"BH-7 / 32 bits, L = 3 * 2^{P - 2}, P = {P}", "plans": plans, "results": r,
            "ratio": r["generate_len_from_table"]["median_ms"] / r["range_combine_ragged"]["median_ms"], "target": 1.15}


def _signal(frames, hop, L):
    g = torch.Generator(device="cuda").manual_seed(1)
    return torch.randint(-2 ** 31, 2 ** 31, ((frames - 1) * hop + L,), dtype=torch.int64, device="cuda", generator=g).int()


def leg_f1_o1(steps, reps, quick):
    P, L, hop = 24, 400, 160
    frames = 1 << (12 if quick else 16)
    p = B.make_params(B.WIN_BH7, P, 32)
    x = _signal(frames, hop, L)
    ext = (frames - 1) * hop + L
    y = torch.empty((frames, L), dtype=torch.int32, device="cuda")
    dev, st, lib = torch.cuda.current_device(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), B.lib()
    f = B.make_frames(frames, hop, shift=31)
    o = B.make_ola(frames, hop, ext, shift=31)
    xo = torch.empty(ext, dtype=torch.int32, device="cuda")
    pp, pf, poo = ctypes.byref(p), ctypes.byref(f), ctypes.byref(o)
    px, py, pxo = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(xo.data_ptr())
    framed = x.as_strided((frames, L), (hop, 1))
    ycopy = torch.empty_like(y)
    ymax = torch.empty(frames, dtype=torch.int32, device="cuda")
    with bhw.ResidentTable(p) as t:
        h = t.handle
        ffns = {"frames_len_from_table": lambda: lib.bhw_apply_frames_len_from_table(h, pp, L, st, pf, px, py),
                "frames_len_library": lambda: lib.bhw_apply_frames_len_device(pp, L, dev, st, pf, px, py),
                "framed_copy": lambda: ycopy.copy_(framed)}
        B.check(ffns["frames_len_from_table"]())
        ref = y.clone()
        B.check(ffns["frames_len_library"]())
        assert torch.equal(y, ref)
        fb = 4 * frames * L * 2                                         # x read frame by frame, y written
        rf = rates(timed(ffns, steps, reps), {k: fb for k in ffns})
        ofns = {"ola_len_from_table": lambda: lib.bhw_overlap_add_len_from_table(h, pp, L, st, poo, py, pxo),
                "ola_len_library": lambda: lib.bhw_overlap_add_len_device(pp, L, dev, st, poo, py, pxo),
                "copy_floor": lambda: (torch.amax(y, dim=1, out=ymax), xo[:frames * hop].view(frames, hop).copy_(y[:, :hop]))}
        B.check(ofns["ola_len_from_table"]())
        ref = xo.clone()
        B.check(ofns["ola_len_library"]())
        assert torch.equal(xo, ref)
        ob = 4 * frames * L + 4 * ext                                   # y read once, x written once
        ro = rates(timed(ofns, steps, reps), {k: ob for k in ofns})
        plans = {"frames_from_table": B.describe_len(p, L, frames=f, table=h), "frames_library": B.describe_len(p, L, frames=f),
                 "ola_from_table": B.describe_len(p, L, ola=o, table=h), "ola_library": B.describe_len(p, L, ola=o)}
    cfg = f"BH-7 / 32 bits, L = {L}, P = {P}, hop {hop}, {frames} frames"
    return [{"leg": "F1", "config": cfg, "plans": plans, "results": rf, "target": 1.2,
             "ratio": rf["frames_len_from_table"]["median_ms"] / rf["framed_copy"]["median_ms"],
             "library_ratio": rf["frames_len_library"]["median_ms"] / rf["framed_copy"]["median_ms"]},
            {"leg": "O1", "config": cfg, "results": ro, "target": 1.2,
             "ratio": ro["ola_len_from_table"]["median_ms"] / ro["copy_floor"]["median_ms"],
             "library_ratio": ro["ola_len_library"]["median_ms"] / ro["copy_floor"]["median_ms"]}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="small shapes (a profiler pass)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_len.json"))
    a = ap.parse_args()
    torch.cuda.init()
    legs = [leg_g1(a.steps, a.reps, a.quick), leg_g2(a.steps, a.reps, a.quick)] + leg_f1_o1(a.steps, a.reps, a.quick)
    rec = {"tool": "tools/bench_len.py", "device": torch.cuda.get_device_name(0), "steps": a.steps, "reps": a.reps, "quick": a.quick,
           "legs": legs}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
