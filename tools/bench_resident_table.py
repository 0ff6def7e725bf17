#!/usr/bin/env python3
"""Resident CORDIC tables (bhw_table_create) against the rebuilt table strategy, one GPU, one process.  Prints one JSON record.

Every leg times whole steps between device events (torch.cuda.Event on the current stream), after warming up every shape it
times.  A step holds `reps` back-to-back calls, so that the host's launch latency (a few microseconds of Python and ctypes per
call) is hidden behind the device work as it is for a caller that streams; times are per call (step / reps).  Each side of a leg
reports the median and the spread (min, max) over --steps steps, the bytes its kernels must move at the least per call
(coefficients written, samples read, the table read once), and the plan line of bhw_table_describe / bhw_describe_plan.
Both sides of a leg run in the same process, alternated step by step.  bench.py stays the contract line (its headline rebuilds
the table in every step, as a caller without a resident table must).

    python tools/bench_resident_table.py [--steps 50] [--out FILE]
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

N26 = 1 << 26


def _stats(ts, reps):
    return {"median_ms": statistics.median(ts) / reps, "min_ms": min(ts) / reps, "max_ms": max(ts) / reps, "steps": len(ts), "reps": reps}


def ab(fa, fb, steps, reps, warm=5):
    """Median / spread per call of two call functions, `reps` calls per step, the two sides alternated step by step."""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(steps):
        for f, ts in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
    return _stats(ta, reps), _stats(tb, reps)


def leg(name, new, old, bytes_new, bytes_old, plan_new, plan_old, steps, note="", reps=1):
    a, b = ab(new, old, steps, reps)
    rec = {"from_table": dict(a, bytes=bytes_new, plan=plan_new), "baseline": dict(b, bytes=bytes_old, plan=plan_old),
           "speedup": b["median_ms"] / a["median_ms"]}
    if note:
        rec["note"] = note
    print(f"{name}: {a['median_ms']:.4f} ms vs {b['median_ms']:.4f} ms", file=sys.stderr)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    steps = max(50, args.steps)
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    L = B.lib()
    res = {"device": torch.cuda.get_device_name(0), "steps": steps, "legs": {}}
    p = bhw.make_params(B.WIN_BH7, 26, 32)
    out = torch.empty(N26, dtype=torch.int32, device="cuda")
    for _ in range(200):                                     # clock ramp
        bhw.generate(p, 0, N26, out=out)
    torch.cuda.synchronize()

    rt = bhw.ResidentTable(p)
    tb = rt.nbytes
    res["table"] = {"bytes": tb, "describe": rt.describe(p, 0, N26)}

    # C3: the whole BH-7 2^26 / 32-bit window
    res["legs"]["C3_from_table"] = leg(
        "C3_from_table", lambda: rt.generate(p, 0, N26, out=out), lambda: bhw.generate(p, 0, N26, out=out),
        4 * N26 + tb, 4 * N26 + 2 * tb, rt.describe(p, 0, N26), B.describe_plan(p, 0, N26), steps, reps=20)

    # weights sweep at one length: BH-7, Nuttall, flat-top (2), Hann, each with both cosine-sum rules, from ONE table
    sweep = []
    for win, preset in ((B.WIN_BH7, None), (None, "nuttall"), (None, "flat-top-2"), (B.WIN_HANN, None)):
        aa = None
        if preset:
            win, _, aa = B.coeffs_preset(preset, 32)
        for combine in (B.COMBINE_HLS, B.COMBINE_VHDL):
            sweep.append(bhw.make_params(win, 26, 32, combine=combine, aa=aa))

    def sweep_new():
        for q in sweep:
            rt.generate(q, 0, N26, out=out)

    def sweep_old():
        for q in sweep:
            bhw.generate(q, 0, N26, out=out)
    res["legs"]["weights_sweep_from_table"] = leg(
        "weights_sweep_from_table", sweep_new, sweep_old, len(sweep) * (4 * N26 + tb), len(sweep) * (4 * N26 + 2 * tb),
        " | ".join(rt.describe(q, 0, N26) for q in sweep), " | ".join(B.describe_plan(q, 0, N26) for q in sweep), steps,
        note=f"one call = {len(sweep)} windows: BH-7, Nuttall, flat-top (2), Hann x (HLS rule, VHDL rule)", reps=3)

    # fused apply over one frame
    x = torch.randint(-(1 << 30), 1 << 30, (N26,), dtype=torch.int32, device="cuda")
    y = torch.empty_like(x)
    res["legs"]["apply_C3_from_table"] = leg(
        "apply_C3_from_table", lambda: rt.apply(p, x, out=y, shift=31), lambda: bhw.apply(p, x, out=y, shift=31),
        8 * N26 + tb, 8 * N26 + 2 * tb, rt.describe(p, 0, N26) + " (apply)", B.describe_plan(p, 0, N26) + " (apply)", steps, reps=20)

    # streaming: the 2^26 window as enable() chunks
    for chunk in (1 << 20, 1 << 16):
        k = N26 // chunk

        def chunks_new(chunk=chunk, k=k):
            for i in range(k):
                rt.generate(p, i * chunk, chunk, out=out[i * chunk:])

        def chunks_old(chunk=chunk, k=k):
            for i in range(k):
                bhw.generate(p, i * chunk, chunk, out=out[i * chunk:])
        res["legs"][f"enable_chunks_{k}x2^{chunk.bit_length() - 1}"] = leg(
            f"enable_chunks {k} x {chunk}", chunks_new, chunks_old, 4 * N26 + tb, 4 * N26,
            rt.describe(p, chunk, chunk), B.describe_plan(p, chunk, chunk), steps, note=f"one call = the window as {k} enable() chunks (AUTO on the baseline side)")

    # the ragged kernel itself: k_range_combine against k_table_combine (format read at run time) over the same table
    n0, cnt = 12345, 1 << 24
    o24 = torch.empty(cnt, dtype=torch.int32, device="cuda")
    for name, q in (("nibble", p), ("nibble_esc", bhw.make_params(B.WIN_BH7, 26, 32, model=B.MODEL_CPP))):
        with bhw.ResidentTable(q) as t2:
            st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

            def generic(t2=t2, q=q):
                B.check(L.bhw_dbg_generate_from_table_generic(t2.handle, ctypes.byref(q), st(), n0, cnt, ctypes.c_void_p(o24.data_ptr())))
            ref = torch.empty_like(o24)
            generic()
            t2.generate(q, n0, cnt, out=ref)
            assert torch.equal(ref, o24), name
            res["legs"][f"range_kernel_ab_{name}"] = leg(
                f"range_kernel_ab {name}", lambda t2=t2, q=q: t2.generate(q, n0, cnt, out=o24), generic, 4 * cnt + t2.nbytes,
                4 * cnt + t2.nbytes, t2.describe(q, n0, cnt), t2.describe(q, n0, cnt).split("]: ")[0] + "]: k_table_combine (format read at run time)",
                steps, note="baseline: bhw_dbg_generate_from_table_generic, the same table through k_table_combine", reps=10)

    # 20 whole windows from the table, captured once and replayed, against the same 20 calls eagerly
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(20):
                rt.generate(p, 0, N26, out=out)

        def eager():
            for _ in range(20):
                rt.generate(p, 0, N26, out=out)
        res["legs"]["graph_from_table"] = leg(
            "graph_from_table", g.replay, eager, 20 * (4 * N26 + tb), 20 * (4 * N26 + tb), "graph of 20 x " + rt.describe(p, 0, N26),
            "20 eager x " + rt.describe(p, 0, N26), steps, note="one call = 20 whole windows")
        torch.cuda.synchronize()
        del g
    rt.close()
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
