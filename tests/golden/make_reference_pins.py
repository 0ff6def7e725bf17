#!/usr/bin/env python3
"""Generate tests/golden/reference_pins.json: what the tests pin against the reference, stored as data so that they run
on a checkout that has neither the upstream sources nor oracle/_ref.

Run in the build container (needs the upstream checkout and oracle/_ref built from it):
    make -C oracle REF=<upstream checkout> && python tests/golden/make_reference_pins.py <upstream checkout>

  lut_literals : the 48 arctangent literals of each ROM in the upstream sources (numbers only, read as text).
  windows      : md5 of whole windows (and of one ragged range that wraps the period) as the reference's own compiled
                 cordic() evaluates them (oracle/_ref, model CPP) in the HLS cosine-sum -- tests/test_gpu_reference_pin.py.
  hls_windows  : md5 of windows of the HLS model in the HLS rule as the reference's own compiled win_function() evaluates them
                 (oracle/_ref/libref_hls_win_*, hls/windows/win_function.cpp against oracle/shim/ap_int.h): per width pair, all six
                 windows whole where the period is small, one whole window with an md5 per block of 2^20 coefficients where it is
                 large, ragged ranges alone at 30/28.
  hls_sincos   : md5 of (sin, cos) from the cordic() of that binary and of the compiled hls/cordic/cordic.cpp.
Everything hashed for the last two keys is first compared with the oracle (oracle/liboracle.so); any difference ends the run.
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402

# (name, win, phi_width, dat_width): the configurations of tests/test_gpu_reference_pin.py
WINDOWS = [("C1", 1, 12, 16), ("C2", 4, 20, 24), ("C4", 4, 16, 24), ("C3", 7, 26, 32),
           ("cpp_26_16", 7, 26, 16), ("cpp_24_30", 5, 24, 30), ("cpp_18_32", 7, 18, 32)]
RAGGED_BACK, RAGGED_COUNT = 777, 5000   # a range from n - 777 that wraps the period


# the HLS model: (NPHASE, NWIDTH) pairs of oracle/Makefile's REF_HLS_PAIRS
WIN_TYPES = (1, 2, 3, 4, 5, 7)
HLS_SMALL = [(10, w) for w in range(8, 33)] + [(12, 16), (16, 24), (4, 16), (16, 16), (17, 16), (6, 8), (4, 32), (13, 31)]
HLS_LARGE = [(20, 24, 4), (26, 32, 7), (18, 32, 7), (24, 30, 5)]      # one window each
HLS_RANGES_ONLY = [(30, 28)]
HLS_CORDIC = [(10, 16), (12, 16), (20, 24), (26, 32), (10, 8), (17, 16), (30, 28)]   # REF_HLS_CORDIC_PAIRS
BLOCK = 1 << 20
WORKERS = max(1, min(8, len(os.sched_getaffinity(0))))


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def literals(ref):
    def grab(rel, pattern, start, end):
        txt = open(os.path.join(ref, rel)).read()
        return ["%012X" % int(x, 16) for x in re.findall(pattern, txt.split(start)[1].split(end)[0])]
    return {"cpp/cordic_sincos.cpp": grab("cpp/cordic_sincos.cpp", r"0x([0-9A-Fa-f]{12})\b", "lut_table", "};"),
            "hls/windows/win_function.cpp": grab("hls/windows/win_function.cpp", r"0x([0-9A-Fa-f]{12})\b", "lut_table", "};"),
            "src/cordic_dds.vhd": grab("src/cordic_dds.vhd", r'x"([0-9A-Fa-f]{12})"', "ROM_LUT : rom_array", ");")}


def windows():
    out = {}
    for name, win, pw, w in WINDOWS:
        p = O.oparams(win, pw, w, model=O.MODEL_CPP)
        n = 1 << pw
        full = O.reference_window(p, 0, n)
        ragged = O.reference_window(p, n - RAGGED_BACK, RAGGED_COUNT)
        out[name] = {"win": win, "phi_width": pw, "dat_width": w, "model": "cpp", "combine": "hls", "md5": md5(full),
                     "ragged": {"n0": n - RAGGED_BACK, "count": RAGGED_COUNT, "md5": md5(ragged)}}
        print(name, out[name]["md5"], flush=True)
    return out


def ragged_ranges(pw, quadrants=False):
    """(n0, count): the range that wraps the period and, on request (where the period is too long to hash whole), one across each
    quadrant boundary.  None below 2^10 (the range would start before the period)."""
    n = 1 << pw
    if pw < 10:
        return []
    out = [(n - RAGGED_BACK, RAGGED_COUNT)]
    if quadrants:
        out += [(q * (n >> 2) - RAGGED_COUNT // 2, RAGGED_COUNT) for q in (1, 2, 3)]
    return out


def hls_window_slices(win, pw, w, n0, count):
    """reference_hls_window over worker PROCESSES (the reference's cordic() keeps a static table: never threads): one
    `python -c` child per slice, each writing its slice to a temporary .npy."""
    if count < (1 << 22) or WORKERS == 1:
        return O.reference_hls_window_type(win, pw, w, n0, count)
    step = -(-count // WORKERS)
    with tempfile.TemporaryDirectory() as tmp:
        jobs = []
        for k in range(WORKERS):
            a, b = k * step, min(count, (k + 1) * step)
            code = ("import sys, numpy as np; sys.path.insert(0, %r); import oracle_lib as O; "
                    "np.save(%r, O.reference_hls_window_type(%d, %d, %d, %d, %d))"
                    % (os.path.dirname(HERE), os.path.join(tmp, "s%d.npy" % k), win, pw, w, n0 + a, b - a))
            jobs.append(subprocess.Popen([sys.executable, "-c", code]))
        for j in jobs:
            if j.wait() != 0:
                raise RuntimeError("a reference worker failed")
        return np.concatenate([np.load(os.path.join(tmp, "s%d.npy" % k)) for k in range(WORKERS)])


def same_as_oracle(what, ref, ora):
    if not np.array_equal(ref, ora):
        bad = np.flatnonzero(ref != ora)
        raise SystemExit("%s: the oracle differs from the compiled reference at %d points, first at offset %d: %d vs %d"
                         % (what, bad.size, bad[0], ora[bad[0]], ref[bad[0]]))
    return ref.size


def hls_windows():
    out, compared = {}, 0
    for pw, w in HLS_SMALL:
        n = 1 << pw
        e = {"phi_width": pw, "dat_width": w, "model": "hls", "combine": "hls", "windows": {}}
        for win in WIN_TYPES:
            p = O.oparams(win, pw, w)
            full = O.reference_hls_window(p, 0, n)
            compared += same_as_oracle("hls %d/%d win %d" % (pw, w, win), full, O.generate(p, 0, n))
            we = {"md5": md5(full), "ranges": []}
            for n0, cnt in ragged_ranges(pw):
                r = O.reference_hls_window(p, n0, cnt)
                compared += same_as_oracle("hls %d/%d win %d at %d" % (pw, w, win, n0), r, O.generate(p, n0, cnt))
                we["ranges"].append({"n0": n0, "count": cnt, "md5": md5(r)})
            e["windows"][str(win)] = we
        out["%d_%d" % (pw, w)] = e
    for pw, w, win in HLS_LARGE:
        n = 1 << pw
        p = O.oparams(win, pw, w)
        full = hls_window_slices(win, pw, w, 0, n)
        compared += same_as_oracle("hls %d/%d win %d" % (pw, w, win), full, O.generate_mt(p, 0, n))
        we = {"md5": md5(full), "block": BLOCK, "block_md5": [md5(full[i:i + BLOCK]) for i in range(0, n, BLOCK)], "ranges": []}
        for n0, cnt in ragged_ranges(pw):
            r = O.reference_hls_window(p, n0, cnt)
            compared += same_as_oracle("hls %d/%d win %d at %d" % (pw, w, win, n0), r, O.generate(p, n0, cnt))
            we["ranges"].append({"n0": n0, "count": cnt, "md5": md5(r)})
        out["%d_%d" % (pw, w)] = {"phi_width": pw, "dat_width": w, "model": "hls", "combine": "hls", "windows": {str(win): we}}
        print("hls", pw, w, win, we["md5"], flush=True)
    for pw, w in HLS_RANGES_ONLY:
        e = {"phi_width": pw, "dat_width": w, "model": "hls", "combine": "hls", "windows": {}}
        for win in WIN_TYPES:
            p = O.oparams(win, pw, w)
            we = {"ranges": []}
            for n0, cnt in ragged_ranges(pw, quadrants=True):
                r = O.reference_hls_window(p, n0, cnt)
                compared += same_as_oracle("hls %d/%d win %d at %d" % (pw, w, win, n0), r, O.generate(p, n0, cnt))
                we["ranges"].append({"n0": n0, "count": cnt, "md5": md5(r)})
            e["windows"][str(win)] = we
        out["%d_%d" % (pw, w)] = e
    print("hls_windows: %d pairs, %d coefficients equal to the oracle" % (len(out), compared), flush=True)
    return out


def hls_sincos():
    """Per pair: both compiled sources (where hls/cordic/cordic.cpp was built at that pair) and the oracle agree; one md5 stands
    for all of them."""
    out, compared = {}, 0
    pairs = HLS_SMALL + [(pw, w) for pw, w, _ in HLS_LARGE] + HLS_RANGES_ONLY
    assert all(pr in pairs for pr in HLS_CORDIC)
    for pw, w in pairs:
        n = 1 << pw
        p = O.oparams(1, pw, w)
        kinds = ["win"] + (["cordic"] if (pw, w) in HLS_CORDIC else [])
        e = {"phi_width": pw, "dat_width": w, "model": "hls", "sources": kinds, "ranges": []}
        spans = ([(0, n)] if pw <= 20 else []) + ragged_ranges(pw, quadrants=pw > 20)
        for t0, cnt in spans:
            so, co = (O.sincos_mt if cnt >= (1 << 18) else O.sincos)(p, t0, cnt)
            for kind in kinds:
                s, c = O.reference_hls_sincos(p, t0, cnt, kind)
                compared += same_as_oracle("hls sin %d/%d %s at %d" % (pw, w, kind, t0), s, so)
                compared += same_as_oracle("hls cos %d/%d %s at %d" % (pw, w, kind, t0), c, co)
            if (t0, cnt) == (0, n):
                e["sin_md5"], e["cos_md5"] = md5(so), md5(co)
            else:
                e["ranges"].append({"theta0": t0, "count": cnt, "sin_md5": md5(so), "cos_md5": md5(co)})
        out["%d_%d" % (pw, w)] = e
    print("hls_sincos: %d pairs, %d values equal to the oracle" % (len(out), compared), flush=True)
    return out


def main():
    ref = sys.argv[1]
    built = {(pw, w) for pw, w, _ in O.ref_hls_pairs()}
    missing = [pr for pr in HLS_SMALL + [(pw, w) for pw, w, _ in HLS_LARGE] + HLS_RANGES_ONLY if pr not in built]
    if missing or {(pw, w) for pw, w, _ in O.ref_hls_pairs("cordic")} < set(HLS_CORDIC):
        raise SystemExit("oracle/_ref lacks HLS binaries (make -C oracle REF=...): %s" % missing)
    res = {"_readme": "see make_reference_pins.py; md5 over the little-endian int32 vector",
           "lut_literals": literals(ref), "windows": windows(), "hls_windows": hls_windows(), "hls_sincos": hls_sincos()}
    with open(os.path.join(HERE, "reference_pins.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
