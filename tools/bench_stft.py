#!/usr/bin/env python3
"""Batched, centred STFT framing and overlap-add (bhw_stft_frames_f32_* / bhw_istft_ola_f32_*) on one GPU, one process.  Prints one JSON
record and writes it to --out (profiles/r11_stft.json by default).

Legs:
  T1 batch       BH-4, P 24, 32 b; B 64, T 160 000, n_fft 512, L 400, hop 160, reflect
  T2 long        BH-7, P 12, 32 b; B 1, T 2^24, n_fft = L 4096, hop 1024, reflect; also the f32 frames call on the same rows of the
                 padded signal (frames_f32_table: center=False, the rows k_frames_f32_* frames)
  T3 clips       as T1 with B 4096, T 16 000
  S1 / S3        the normalised overlap-add of T1 / T3 (length = T)
  D_L1..D_F1     the new frames kernel at B = 1, pad 0, col0 0, n_fft = L against k_frames_f32_* on section 13's L1-L3, F1 shapes
  R_S1..R_O1     section 13's overlap-add legs S1-S3, O1 (the unbatched calls), against profiles/r10_f32.json
Variants of the frames legs: stft_table / stft_library (the new calls); copy (torch copy of the framed view of the padded batch into y:
every byte of y written, x read through the frames); torch (F.pad + unfold * the window padded to n_fft); workaround (F.pad, then B
calls of apply_frames f32 from the table into a zeroed buffer).  Of the overlap-add legs: istft_table / istft_library; unbatched (one
f32 from-table overlap-add over B * frames frames: the cost of batching); torch (fold + envelope division); per_signal (B calls of the
f32 from-table overlap-add).  Every variant is warmed, then timed in steps of `reps` back-to-back calls between device events, the
variants of a leg alternated step by step; times are per call (median, min, max over --steps).

    python tools/bench_stft.py [--steps 10] [--reps 20] [--out FILE] [--quick]
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
import torch.nn.functional as F  # noqa: E402
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


def _ok(rc):
    B.check(rc)


def _ctx():
    return torch.cuda.current_device(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), B.lib()


def frames_leg(name, p, nb, T, n_fft, L, hop, steps, reps, workaround=True, frames_f32=False):
    pad, col0, shift = n_fft // 2, (n_fft - L) // 2, p.dat_width - 1
    frames = 1 + (T + 2 * pad - n_fft) // hop
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((nb, T), device="cuda", generator=g)
    y = torch.empty((nb, frames, n_fft), device="cuda")
    dev, st, lib = _ctx()
    s = B.make_stft(nb, T, frames, hop, n_fft, col0=col0, pad=pad, pad_mode=B.PAD_REFLECT, shift=shift)
    pp, ps = ctypes.byref(p), ctypes.byref(s)
    px, py = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr())
    wpad = torch.zeros(n_fft, device="cuda")
    wpad[col0:col0 + L] = bhw.window(p, L, dtype=torch.float32)
    f1 = B.make_frames(frames, hop, shift=shift, y_stride=n_fft)
    pf = ctypes.byref(f1)
    with bhw.ResidentTable(p) as t:
        h = t.handle

        def work():
            y.zero_()
            xp = F.pad(x, [pad, pad], mode="reflect")
            for b in range(nb):
                _ok(lib.bhw_apply_frames_f32_from_table(h, pp, L, st, pf, ctypes.c_void_p(xp[b].data_ptr() + 4 * col0),
                                                        ctypes.c_void_p(y[b].data_ptr() + 4 * col0)))

        framed = F.pad(x, [pad, pad], mode="reflect").unfold(-1, n_fft, hop)
        fns = {"stft_table": lambda: _ok(lib.bhw_stft_frames_f32_from_table(h, pp, L, st, ps, px, py)),
               "stft_library": lambda: _ok(lib.bhw_stft_frames_f32_device(pp, L, dev, st, ps, px, py)),
               "copy": lambda: y.copy_(framed),
               "torch": lambda: torch.mul(F.pad(x, [pad, pad], mode="reflect").unfold(-1, n_fft, hop), wpad, out=y)}
        if workaround:
            fns["workaround"] = work
        if frames_f32:                  # the f32 frames kernel on the same rows of the padded signal (center=False), same leg
            xpad = F.pad(x, [pad, pad], mode="reflect")
            pxp = ctypes.c_void_p(xpad.data_ptr())
            fns["frames_f32_table"] = lambda: _ok(lib.bhw_apply_frames_f32_from_table(h, pp, L, st, pf, pxp, py))
        fns["stft_table"]()
        ref = y.clone()
        fns["torch"]()
        torch_equal = bool(torch.equal(y, ref))
        if workaround:
            work()
            work_equal = bool(torch.equal(y, ref))
        res = timed(fns, steps, reps)
        plans = {"stft_table": B.describe_stft(p, L, s, table=h), "stft_library": B.describe_stft(p, L, s)}
    m = {k: v["median_ms"] for k, v in res.items()}
    out = {"leg": name, "kind": "frames", "batch": nb, "T": T, "n_fft": n_fft, "L": L, "hop": hop, "frames": frames, "plans": plans,
           "results": res, "bytes_written": nb * frames * n_fft * 4, "bytes_read_distinct": nb * T * 4,
           "torch_equal": torch_equal,
           "table_over_copy": m["stft_table"] / m["copy"], "library_over_copy": m["stft_library"] / m["copy"],
           "table_over_torch": m["stft_table"] / m["torch"]}
    if workaround:
        out["workaround_bit_equal"] = work_equal
        out["table_over_workaround"] = m["stft_table"] / m["workaround"]
    if frames_f32:
        out["table_over_frames_f32"] = m["stft_table"] / m["frames_f32_table"]
    return out


def ola_leg(name, p, nb, T, n_fft, L, hop, steps, reps):
    pad, col0, shift = n_fft // 2, (n_fft - L) // 2, p.dat_width - 1
    frames = 1 + (T + 2 * pad - n_fft) // hop
    g = torch.Generator(device="cuda").manual_seed(2)
    y = torch.randn((nb, frames, n_fft), device="cuda", generator=g)
    x = torch.empty((nb, T), device="cuda")
    dev, st, lib = _ctx()
    s = B.make_stft(nb, T, frames, hop, n_fft, col0=col0, pad=pad, shift=shift)
    pp, ps = ctypes.byref(p), ctypes.byref(s)
    px, py = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr())
    ext = (nb * frames - 1) * hop + L
    xu = torch.empty(ext, device="cuda")
    ou = B.make_ola(nb * frames, hop, ext, shift=shift, y_stride=n_fft)
    o1 = B.make_ola(frames, hop, T, t0=pad - col0, shift=shift, y_stride=n_fft)
    po, po1 = ctypes.byref(ou), ctypes.byref(o1)
    wpad = torch.zeros(n_fft, device="cuda")
    wpad[col0:col0 + L] = bhw.window(p, L, dtype=torch.float32)
    padded_len = n_fft + hop * (frames - 1)
    env = F.fold((wpad * wpad).expand(1, frames, n_fft).transpose(1, 2), (1, padded_len), (1, n_fft), stride=(1, hop)).reshape(-1)
    envc = env[pad:pad + T].clamp_min(1e-30)
    yoff = ctypes.c_void_p(y.data_ptr() + 4 * col0)

    def torch_fold():
        z = F.fold((y * wpad).transpose(1, 2), (1, padded_len), (1, n_fft), stride=(1, hop)).reshape(nb, -1)
        torch.div(z[:, pad:pad + T], envc, out=x)

    with bhw.ResidentTable(p) as t:
        h = t.handle

        def per_signal():
            for b in range(nb):
                _ok(lib.bhw_overlap_add_f32_from_table(h, pp, L, st, po1, 1, ctypes.c_void_p(y[b].data_ptr() + 4 * col0),
                                                       ctypes.c_void_p(x[b].data_ptr())))

        fns = {"istft_table": lambda: _ok(lib.bhw_istft_ola_f32_from_table(h, pp, L, st, ps, 1, py, px)),
               "istft_library": lambda: _ok(lib.bhw_istft_ola_f32_device(pp, L, dev, st, ps, 1, py, px)),
               "unbatched": lambda: _ok(lib.bhw_overlap_add_f32_from_table(h, pp, L, st, po, 1, yoff, ctypes.c_void_p(xu.data_ptr()))),
               "torch": torch_fold, "per_signal": per_signal}
        fns["istft_table"]()
        ref = x.clone()
        per_signal()
        per_signal_equal = bool(torch.equal(x, ref))
        res = timed(fns, steps, reps)
        plans = {"istft_table": B.describe_stft(p, L, s, inverse=True, normalize=True, table=h),
                 "unbatched": B.describe_f32(p, L, ola=ou, normalize=True, table=h)}
    m = {k: v["median_ms"] for k, v in res.items()}
    return {"leg": name, "kind": "overlap-add", "batch": nb, "T": T, "n_fft": n_fft, "L": L, "hop": hop, "frames": frames, "plans": plans,
            "results": res, "per_signal_bit_equal": per_signal_equal,
            "table_over_unbatched": m["istft_table"] / m["unbatched"], "table_over_torch": m["istft_table"] / m["torch"],
            "table_over_per_signal": m["istft_table"] / m["per_signal"]}


def dup_leg(name, p, N, hop, frames, C, steps, reps):
    """The new frames kernel at B = 1, pad 0, col0 0, n_fft = L against the f32 frames kernel (k_frames_f32_*), same rows."""
    shift = p.dat_width - 1
    g = torch.Generator(device="cuda").manual_seed(3)
    T = (frames - 1) * hop + N
    x = torch.randn(T * C, device="cuda", generator=g)
    y = torch.empty(frames * N * C, device="cuda")
    dev, st, lib = _ctx()
    s = B.make_stft(1, T, frames, hop, N, channels=C, shift=shift)
    f = B.make_frames(frames, hop, channels=C, shift=shift)
    pp, ps, pf = ctypes.byref(p), ctypes.byref(s), ctypes.byref(f)
    px, py = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr())
    with bhw.ResidentTable(p) as t:
        h = t.handle
        fns = {"stft_table": lambda: _ok(lib.bhw_stft_frames_f32_from_table(h, pp, N, st, ps, px, py)),
               "frames_f32_table": lambda: _ok(lib.bhw_apply_frames_f32_from_table(h, pp, N, st, pf, px, py))}
        fns["stft_table"]()
        ref = y.clone()
        fns["frames_f32_table"]()
        equal = bool(torch.equal(y, ref))
        res = timed(fns, steps, reps)
    m = {k: v["median_ms"] for k, v in res.items()}
    return {"leg": name, "kind": "duplicate path", "N": N, "hop": hop, "frames": frames, "channels": C, "results": res, "bit_equal": equal,
            "stft_over_frames_f32": m["stft_table"] / m["frames_f32_table"]}


def ola_repeat_leg(name, p, N, hop, frames, C, steps, reps, old):
    """Section 13's unbatched overlap-add legs, the calls unchanged (the in-place batch dimension)."""
    shift = p.dat_width - 1
    ext = (frames - 1) * hop + N
    g = torch.Generator(device="cuda").manual_seed(2)
    yf = torch.randn((frames, N * C), device="cuda", generator=g) * 1000
    xf = torch.empty((ext, C), device="cuda")
    dev, st, lib = _ctx()
    o = B.make_ola(frames, hop, ext, channels=C, shift=shift)
    pp, po = ctypes.byref(p), ctypes.byref(o)
    pxf, pyf = ctypes.c_void_p(xf.data_ptr()), ctypes.c_void_p(yf.data_ptr())
    with bhw.ResidentTable(p) as t:
        h = t.handle
        fns = {"f32_table": lambda: _ok(lib.bhw_overlap_add_f32_from_table(h, pp, N, st, po, 0, pyf, pxf)),
               "f32_table_norm": lambda: _ok(lib.bhw_overlap_add_f32_from_table(h, pp, N, st, po, 1, pyf, pxf))}
        res = timed(fns, steps, reps)
    out = {"leg": name, "kind": "overlap-add repeat", "N": N, "hop": hop, "frames": frames, "channels": C, "results": res}
    if old:
        out["r10_median_ms"] = {k: old["results"][k]["median_ms"] for k in fns}
        out["over_r10"] = {k: res[k]["median_ms"] / old["results"][k]["median_ms"] for k in fns}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="smaller shapes (a profiler pass)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_stft.json"))
    a = ap.parse_args()
    torch.cuda.init()
    q = 4 if a.quick else 0
    bh4, bh7 = B.make_params(B.WIN_BH4, 24, 32), B.make_params(B.WIN_BH7, 12, 32)
    try:
        with open(os.path.join(ROOT, "profiles", "r10_f32.json")) as fh:
            r10 = {lg["leg"]: lg for lg in json.load(fh)["legs"]}
    except OSError:
        r10 = {}
    S, R = a.steps, a.reps
    wt, _, aa = B.coeffs_preset("nuttall", 24)
    legs = [frames_leg("T1_batch", bh4, 64 >> q, 160000, 512, 400, 160, S, R),
            frames_leg("T2_long", bh7, 1, 1 << (24 - q), 4096, 4096, 1024, S, R, workaround=False, frames_f32=True),
            frames_leg("T3_clips", bh4, 4096 >> q, 16000, 512, 400, 160, S, R),
            ola_leg("S1_batch", bh4, 64 >> q, 160000, 512, 400, 160, S, R),
            ola_leg("S3_clips", bh4, 4096 >> q, 16000, 512, 400, 160, S, R),
            dup_leg("D_L1_stft", bh7, 1 << 12, 1 << 10, 1 << (14 - q), 1, S, R),
            dup_leg("D_L2_welch", B.make_params(wt, 16, 24, aa=aa), 1 << 16, 1 << 15, 1 << (10 - q), 1, S, R),
            dup_leg("D_L3_iq", B.make_params(B.WIN_BH4, 14, 16), 1 << 14, 1 << 13, 1 << (11 - q), 2, S, R),
            dup_leg("D_F1_len400", B.make_params(B.WIN_BH7, 24, 32), 400, 160, 1 << (16 - q), 1, S, R),
            ola_repeat_leg("R_S1_stft", bh7, 1 << 12, 1 << 10, 1 << (14 - q), 1, S, R, r10.get("S1_stft")),
            ola_repeat_leg("R_S2_hann", B.make_params(B.WIN_HANN, 16, 24), 1 << 16, 1 << 15, 1 << (10 - q), 1, S, R, r10.get("S2_hann")),
            ola_repeat_leg("R_S3_iq", B.make_params(B.WIN_BH4, 14, 16), 1 << 14, 1 << 13, 1 << (11 - q), 2, S, R, r10.get("S3_iq")),
            ola_repeat_leg("R_O1_len400", B.make_params(B.WIN_BH7, 24, 32), 400, 160, 1 << (16 - q), 1, S, R, r10.get("O1_len400"))]
    rec = {"tool": "tools/bench_stft.py", "device": torch.cuda.get_device_name(0), "steps": a.steps, "reps": a.reps, "quick": a.quick,
           "legs": legs}
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
