#!/usr/bin/env python3
"""A/B of the unbatched float32 overlap-add and frame apply between two builds of the package, one process per build.

    python tools/ab_ola_f32.py ROOT_A >> ab.jsonl; python tools/ab_ola_f32.py ROOT_B >> ab.jsonl; ... (alternate A and B)

ROOT is a directory holding a built blackman_harris_win_amd package (a checkout after `python __graft_entry__.py`, e.g. of the parent
commit, or this tree).  Times, per call from a resident table (median of 10 steps of 20 calls, µs), section 13's overlap-add legs
S1 - S3, O1 (plain and normalised) and frames legs L1, F1.  Prints one JSON line.  profiles/r11_ola_parent_ab.jsonl holds two
alternations, parent / this change.
"""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.abspath(sys.argv[1])
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import blackman_harris_win_amd as bhw  # noqa: E402
from blackman_harris_win_amd import binding as B  # noqa: E402

assert os.path.abspath(bhw.__file__).startswith(ROOT), bhw.__file__


def timed(fns, steps=10, reps=20):
    for f in fns.values():
        f()
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
            ts[k].append(e0.elapsed_time(e1) / reps * 1000)
    return {k: statistics.median(v) for k, v in ts.items()}


def main():
    st, lib = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), B.lib()
    bh7 = lambda pw, W: B.make_params(B.WIN_BH7, pw, W)  # noqa: E731
    out = {}
    for name, p, N, hop, frames, C in [("S1", bh7(12, 32), 1 << 12, 1 << 10, 1 << 14, 1),
                                       ("S2", B.make_params(B.WIN_HANN, 16, 24), 1 << 16, 1 << 15, 1 << 10, 1),
                                       ("S3", B.make_params(B.WIN_BH4, 14, 16), 1 << 14, 1 << 13, 1 << 11, 2),
                                       ("O1", bh7(24, 32), 400, 160, 1 << 16, 1)]:
        ext = (frames - 1) * hop + N
        yf = torch.randn((frames, N * C), device="cuda") * 1000
        xf = torch.empty((ext, C), device="cuda")
        o = B.make_ola(frames, hop, ext, channels=C, shift=p.dat_width - 1)
        pp, po, py, px = ctypes.byref(p), ctypes.byref(o), ctypes.c_void_p(yf.data_ptr()), ctypes.c_void_p(xf.data_ptr())
        with bhw.ResidentTable(p) as t:
            h = t.handle
            r = timed({"plain": lambda: B.check(lib.bhw_overlap_add_f32_from_table(h, pp, N, st, po, 0, py, px)),
                       "norm": lambda: B.check(lib.bhw_overlap_add_f32_from_table(h, pp, N, st, po, 1, py, px))})
        out[name + "_plain_us"], out[name + "_norm_us"] = r["plain"], r["norm"]
    for name, p, N, hop, frames, C in [("L1", bh7(12, 32), 1 << 12, 1 << 10, 1 << 14, 1), ("F1", bh7(24, 32), 400, 160, 1 << 16, 1)]:
        x = torch.randn(((frames - 1) * hop + N) * C, device="cuda")
        y = torch.empty(frames * N * C, device="cuda")
        f = B.make_frames(frames, hop, channels=C, shift=p.dat_width - 1)
        pp, pf, px, py = ctypes.byref(p), ctypes.byref(f), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr())
        with bhw.ResidentTable(p) as t:
            h = t.handle
            out[name + "_frames_us"] = timed({"f": lambda: B.check(lib.bhw_apply_frames_f32_from_table(h, pp, N, st, pf, px, py))})["f"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
