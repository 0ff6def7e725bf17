#!/usr/bin/env python3
"""Float32 frame apply and overlap-add (bhw_apply_frames_f32_* / bhw_overlap_add_f32_*) on one GPU, one process.  Prints one JSON
record and writes it to --out (profiles/r10_f32.json by default).

Legs, the shapes of r07 / r08 / r09:
  L1 STFT (BH-7, 2^12, 32 bits, hop N/4, 2^14 frames), L2 Welch (Nuttall, 2^16, 24 bits, hop N/2, 2^10 frames), L3 I/Q (BH-4, 2^14,
  16 bits, hop N/2, 2^11 frames, two channels), F1 (BH-7, 32 bits, L = 400, P = 24, hop 160, 2^16 frames): the frame apply;
  S1 / S2 (Hann, 2^16, 24 bits, hop N/2, 2^10 frames) / S3 / O1: the overlap-add of the same shapes.
Each leg times, in the same process:
  f32_table / f32_library       the float32 call from a resident table / by the direct CORDIC chains (overlap-add: also normalised)
  i32_table                     the int32 from-table call of the same shape (the same bytes)
  workaround                    what a float caller runs today: x (or y) quantised to int32, the int32 from-table call, the result
                                converted back to float32 (overlap-add: and divided by a precomputed window envelope)
  torch                         torch fp32 with v = bhw.window(..., dtype=float32): x.unfold * v (frames); (y * v) index_add_ into
                                the signal, then the division by the envelope (overlap-add)
Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events, the variants of a leg alternated step
by step; times are per call (median, min, max over --steps).  Targets (from byte counts): f32 frames from a table <= 1.05 x the int32
one, f32 overlap-add from a table <= 1.10 x, normalised <= 1.15 x the plain f32 call, every f32 from-table leg below the workaround.

    python tools/bench_f32.py [--steps 10] [--reps 20] [--out FILE] [--quick]
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
    for v in res.values():
        v["bytes"] = nbytes
        v["TBps"] = nbytes / (v["median_ms"] * 1e-3) / 1e12
        v["of_peak"] = v["TBps"] * 1e12 / PEAK
    return res


def _ok(rc):
    B.check(rc)


def frames_leg(name, p, N, hop, frames, C, steps, reps, length=None):
    L = N
    shift = p.dat_width - 1
    g = torch.Generator(device="cuda").manual_seed(1)
    n = ((frames - 1) * hop + L) * C
    xf = torch.randn(n, device="cuda", generator=g) * 1000
    xi = torch.empty(n, dtype=torch.int32, device="cuda")
    yf = torch.empty((frames, L * C), device="cuda")
    yi = torch.empty((frames, L * C), dtype=torch.int32, device="cuda")
    dev, st, lib = torch.cuda.current_device(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), B.lib()
    f = B.make_frames(frames, hop, channels=C, shift=shift)
    pp, pf = ctypes.byref(p), ctypes.byref(f)
    pxf, pyf, pxi, pyi = (ctypes.c_void_p(t.data_ptr()) for t in (xf, yf, xi, yi))
    lw = L if length is None else length
    v = bhw.window(p, L, dtype=torch.float32)
    framed = xf.as_strided((frames, L, C), (hop * C, C, 1))
    yv = yf.view(frames, L, C)
    vv = v[:, None]
    with bhw.ResidentTable(p) as t:
        h = t.handle
        i32 = (lambda: lib.bhw_apply_frames_from_table(h, pp, st, pf, pxi, pyi)) if length is None else \
              (lambda: lib.bhw_apply_frames_len_from_table(h, pp, length, st, pf, pxi, pyi))
        fns = {"f32_table": lambda: _ok(lib.bhw_apply_frames_f32_from_table(h, pp, lw, st, pf, pxf, pyf)),
               "f32_library": lambda: _ok(lib.bhw_apply_frames_f32_device(pp, lw, dev, st, pf, pxf, pyf)),
               "i32_table": lambda: _ok(i32()),
               "workaround": lambda: (xi.copy_(xf), _ok(i32()), yf.copy_(yi)),
               "torch": lambda: torch.mul(framed, vv, out=yv)}
        fns["f32_table"]()
        ref = yf.clone()
        fns["f32_library"]()
        assert torch.equal(yf, ref)
        fns["torch"]()
        torch_equal = bool(torch.equal(yf, ref))
        res = rates(timed(fns, steps, reps), frames * L * C * 4 + ((frames - 1) * hop + L) * C * 4)
        plans = {"f32_table": B.describe_f32(p, lw, frames=f, table=h), "f32_library": B.describe_f32(p, lw, frames=f)}
    m = {k: v["median_ms"] for k, v in res.items()}
    return {"leg": name, "kind": "frames", "N": L, "hop": hop, "frames": frames, "channels": C, "plans": plans, "results": res,
            "torch_fp32_bit_equal": torch_equal,
            "f32_over_i32_table": m["f32_table"] / m["i32_table"], "target_f32_over_i32": 1.05,
            "f32_table_over_workaround": m["f32_table"] / m["workaround"]}


def ola_leg(name, p, N, hop, frames, C, steps, reps, length=None):
    L = N
    shift = p.dat_width - 1
    ext = (frames - 1) * hop + L
    g = torch.Generator(device="cuda").manual_seed(2)
    yf = torch.randn((frames, L * C), device="cuda", generator=g) * 1000
    yi = torch.empty((frames, L * C), dtype=torch.int32, device="cuda")
    xf = torch.empty((ext, C), device="cuda")
    xi = torch.empty((ext, C), dtype=torch.int32, device="cuda")
    dev, st, lib = torch.cuda.current_device(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), B.lib()
    o = B.make_ola(frames, hop, ext, channels=C, shift=shift)
    pp, po = ctypes.byref(p), ctypes.byref(o)
    pxf, pyf, pxi, pyi = (ctypes.c_void_p(t.data_ptr()) for t in (xf, yf, xi, yi))
    lw = L if length is None else length
    v = bhw.window(p, L, dtype=torch.float32)
    idx = (torch.arange(frames, device="cuda")[:, None] * hop + torch.arange(L, device="cuda")[None, :]).reshape(-1)
    env = torch.zeros(ext, device="cuda").index_add_(0, idx, (v * v).repeat(frames))
    envc = env.clamp_min(1e-30)[:, None]
    prod = torch.empty((frames, L, C), device="cuda")
    yv = yf.view(frames, L, C)
    vv = v[:, None]
    with bhw.ResidentTable(p) as t:
        h = t.handle
        i32 = (lambda: lib.bhw_overlap_add_from_table(h, pp, st, po, pyi, pxi)) if length is None else \
              (lambda: lib.bhw_overlap_add_len_from_table(h, pp, length, st, po, pyi, pxi))
        fns = {"f32_table": lambda: _ok(lib.bhw_overlap_add_f32_from_table(h, pp, lw, st, po, 0, pyf, pxf)),
               "f32_table_norm": lambda: _ok(lib.bhw_overlap_add_f32_from_table(h, pp, lw, st, po, 1, pyf, pxf)),
               "f32_library": lambda: _ok(lib.bhw_overlap_add_f32_device(pp, lw, dev, st, po, 0, pyf, pxf)),
               "f32_library_norm": lambda: _ok(lib.bhw_overlap_add_f32_device(pp, lw, dev, st, po, 1, pyf, pxf)),
               "i32_table": lambda: _ok(i32()),
               "workaround": lambda: (yi.copy_(yf), _ok(i32()), torch.div(xi, envc, out=xf)),
               "torch": lambda: (torch.mul(yv, vv, out=prod), xf.zero_(), xf.index_add_(0, idx, prod.view(-1, C)), xf.div_(envc))}
        for k in ("f32_table", "f32_library"):
            fns[k]()
        res = rates(timed(fns, steps, reps), frames * L * C * 4 + ext * C * 4)
        plans = {"f32_table": B.describe_f32(p, lw, ola=o, table=h), "f32_table_norm": B.describe_f32(p, lw, ola=o, normalize=True, table=h),
                 "f32_library": B.describe_f32(p, lw, ola=o)}
    m = {k: v["median_ms"] for k, v in res.items()}
    return {"leg": name, "kind": "overlap-add", "N": L, "hop": hop, "frames": frames, "channels": C, "plans": plans, "results": res,
            "f32_over_i32_table": m["f32_table"] / m["i32_table"], "target_f32_over_i32": 1.10,
            "norm_over_plain_table": m["f32_table_norm"] / m["f32_table"], "target_norm": 1.15,
            "f32_table_over_workaround": m["f32_table"] / m["workaround"],
            "f32_table_norm_over_workaround": m["f32_table_norm"] / m["workaround"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="fewer frames per leg (a profiler pass)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_f32.json"))
    a = ap.parse_args()
    torch.cuda.init()
    q = 4 if a.quick else 0                                              # frames divided by 2^q
    bh7 = lambda pw, W: B.make_params(B.WIN_BH7, pw, W)  # noqa: E731
    wt, _, aa = B.coeffs_preset("nuttall", 24)
    legs = [frames_leg("L1_stft", bh7(12, 32), 1 << 12, 1 << 10, 1 << (14 - q), 1, a.steps, a.reps),
            frames_leg("L2_welch", B.make_params(wt, 16, 24, aa=aa), 1 << 16, 1 << 15, 1 << (10 - q), 1, a.steps, a.reps),
            frames_leg("L3_iq", B.make_params(B.WIN_BH4, 14, 16), 1 << 14, 1 << 13, 1 << (11 - q), 2, a.steps, a.reps),
            frames_leg("F1_len400", bh7(24, 32), 400, 160, 1 << (16 - q), 1, a.steps, a.reps, length=400),
            ola_leg("S1_stft", bh7(12, 32), 1 << 12, 1 << 10, 1 << (14 - q), 1, a.steps, a.reps),
            ola_leg("S2_hann", B.make_params(B.WIN_HANN, 16, 24), 1 << 16, 1 << 15, 1 << (10 - q), 1, a.steps, a.reps),
            ola_leg("S3_iq", B.make_params(B.WIN_BH4, 14, 16), 1 << 14, 1 << 13, 1 << (11 - q), 2, a.steps, a.reps),
            ola_leg("O1_len400", bh7(24, 32), 400, 160, 1 << (16 - q), 1, a.steps, a.reps, length=400)]
    rec = {"tool": "tools/bench_f32.py", "device": torch.cuda.get_device_name(0), "steps": a.steps, "reps": a.reps, "quick": a.quick,
           "peak_TBps": PEAK / 1e12, "legs": legs}
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
