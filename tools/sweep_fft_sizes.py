#!/usr/bin/env python3
"""Every n_fft of the fused FFT kernels on one GPU, on the rows of tests/fft_sweep_rows.py (noise, an impulse train, three exact-bin
tones, DC plus Nyquist): the figures tests/test_gpu_fft_size_sweep.py gates, recorded.  Run once, by hand, outside pytest; prints a
summary and writes --out (profiles/r21_fft_size_sweep.json by default).

Per family (mixed radix: the 95 sizes of bhw.stft_mixed / istft_mixed; power of two, real: bhw.stft / istft at 16..4096; power of two,
I/Q: bhw.stft_iq / istft_iq at 16..2048), size, direction and row type: the fused call's error, the yardstick's error on the same GPU
(torch.fft.rfft / fft over the parent's rows; torch.fft.irfft / ifft + istft_overlap_add) and the cap 2^-24 log2 n_fft, by the references
and metrics of the test file (its *_figures functions, which also hold everything around the transform word for word).  For the mixed
radix sizes also the round trip istft_mixed(stft_mixed(x)) against torch.istft(torch.stft(x)).  The summary names, per family, direction
and row type, the worst fused / cap and the worst fused / yardstick and the size each occurred at.

    python tools/sweep_fft_sizes.py [--out FILE]

--epilogues runs the other sweep instead: every size of the four forward families under the power, filter-bank, Welch and hold
epilogues (tests/epilogue_sweep_rows.py, the figures tests/test_gpu_epilogue_size_sweep.py holds), written to
profiles/r39_epilogue_size_sweep.json by default.

    python tools/sweep_fft_sizes.py --epilogues [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import fft_sweep_rows as R  # noqa: E402
import test_gpu_fft_size_sweep as S  # noqa: E402

FAMILIES = (("mixed", "mixed radix", R.SIZES), ("real", "power of two, real", R.POW2_REAL), ("iq", "power of two, I/Q", R.POW2_IQ))


def worst(sizes, names, key):
    """Per row type: the largest key(entry, b) over the sizes and the n_fft it occurred at."""
    out = {}
    for b, name in enumerate(names):
        n, e = max(((e["n_fft"], key(e, b)) for e in sizes), key=lambda t: t[1])
        out[name] = {"value": e, "n_fft": n}
    return out


def epilogues(out):
    """--epilogues: every size of the four families under every epilogue that is not the stored spectrum, by
    tests/test_gpu_epilogue_size_sweep.epilogue_figures (the function its tests hold): per family and front the number of sizes, the
    differing words against the exact contract (expected 0) and the worst ratio to the derived float64 bound, with the size and row
    type it occurred at."""
    import epilogue_sweep_rows as E
    import test_gpu_epilogue_size_sweep as G
    tables = S.Tables()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": "tests/epilogue_sweep_rows.py",
           "bounds": {"power": "2 g + g^2 + 2^-23", "bank": "power x max |W|", "welch": "power + 2^-24", "hold": "power, of the loudest frame",
                      "stored spectrum": "g = fft_sweep_rows.gate(n, row)"},
           "families": {}}
    for fam, sizes in E.FAMILIES.items():
        names = E.row_types(fam)
        fronts = {}
        for n in sizes:
            for e in G.epilogue_figures(torch, tables, fam, n):
                f = fronts.setdefault(e["front"], {"sizes": set(), "calls": 0, "words": 0, "differing_words": 0, "worst_ratio": None})
                f["sizes"].add(n)
                f["calls"] += 1
                if e["differ"] is not None:
                    f["words"] += e["words"]
                    f["differing_words"] += e["differ"]
                if e["ratios"] is not None:
                    b = max(range(len(names)), key=lambda i: e["ratios"][i])
                    if f["worst_ratio"] is None or e["ratios"][b] > f["worst_ratio"]["value"]:
                        f["worst_ratio"] = {"value": e["ratios"][b], "n_fft": n, "row": names[b], "form": e["form"]}
        for name, f in fronts.items():
            f["sizes"] = len(f["sizes"])
            w = f["worst_ratio"]
            print(f"{fam}, {name}: {f['sizes']} sizes, {f['differing_words']} differing words of {f['words']}"
                  + (f", worst ratio to the bound {w['value']:.3f} at n_fft {w['n_fft']}, {w['row']}" if w else ""))
        rec["families"][fam] = {"sizes": len(sizes), "row_types": list(names), "fronts": fronts}
    torch.cuda.synchronize()
    tables.close()
    with open(out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--epilogues", action="store_true", help="the epilogue size sweep (profiles/r39_epilogue_size_sweep.json)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if a.epilogues:
        return epilogues(a.out or os.path.join(ROOT, "profiles", "r39_epilogue_size_sweep.json"))
    a.out = a.out or os.path.join(ROOT, "profiles", "r21_fft_size_sweep.json")
    tables = S.Tables()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": "tests/fft_sweep_rows.py",
           "gates": {"noise": "fused <= 2 x yardstick and fused <= cap", "structured": "fused <= 2 x cap; the yardstick is not gated"},
           "families": {}, "summary": {}}
    for kind, title, sizes in FAMILIES:
        names = list(S._names(kind))
        fam = {"row_types": names, "forward": [], "inverse": []}
        for n in sizes:
            for direction, fn in (("forward", S.forward_figures), ("inverse", S.inverse_figures)):
                fig = fn(torch, tables, n, kind)
                fam[direction].append({"n_fft": n, "cap": R.cap(n), "fused": [f for f, _ in fig], "yardstick": [y for _, y in fig]})
        if kind == "mixed":
            fam["round_trip"] = []
            for n in sizes:
                err, yard = S.round_trip_figures(torch, n)
                fam["round_trip"].append({"n_fft": n, "fused": err, "torch": yard})
            n, r = max(((e["n_fft"], e["fused"] / e["torch"]) for e in fam["round_trip"]), key=lambda t: t[1])
            rec["summary"][f"{title}, round trip"] = {"worst fused / torch": {"value": r, "n_fft": n}}
        rec["families"][title] = fam
        for direction in ("forward", "inverse"):
            rec["summary"][f"{title}, {direction}"] = {
                "worst fused / cap": worst(fam[direction], names, lambda e, b: e["fused"][b] / e["cap"]),
                "worst fused / yardstick": worst(fam[direction], names, lambda e, b: e["fused"][b] / e["yardstick"][b] if e["yardstick"][b] else 0.0),
                "worst yardstick / cap": worst(fam[direction], names, lambda e, b: e["yardstick"][b] / e["cap"])}
    torch.cuda.synchronize()
    tables.close()
    for title, s in rec["summary"].items():
        for what, rows in s.items():
            if "value" in rows:
                print(f"{title}: {what} {rows['value']:.3f} at n_fft {rows['n_fft']}")
                continue
            for name, w in rows.items():
                print(f"{title}, {name}: {what} {w['value']:.3f} at n_fft {w['n_fft']}")
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=None, separators=(",", ":")).replace('{"n_fft"', '\n{"n_fft"').replace('"summary"', '\n"summary"') + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
