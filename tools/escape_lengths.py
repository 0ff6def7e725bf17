"""Choose the window lengths whose gathers reach listed entries of a nibble + escapes table, and record them.

A nibble + escapes table lists about one entry in 10^4 exactly (the entries whose deviation leaves the four-bit fields); a window of
L <= 4096 coefficients gathers about L distinct entries, the angles round(m 2^P / L), so a test case reaches a listed entry by luck or
not at all.  tools/sim_build.cpp --escapes (the host model of the build kernel) prints which entries are listed;
tests/table_source_cases.choose_lengths takes, per cap on L, the length that reaches the most of them.

  python tools/escape_lengths.py            print the record of every escapes table of tests/table_source_cases.py
  python tools/escape_lengths.py --write    also write tests/golden/table_source_escapes.json
  python tools/escape_lengths.py --top 12   also print the 12 best lengths per cap

No GPU.  tests/test_table_source_cases.py derives the same record again and compares it with the fixture."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import table_source_cases as C  # noqa: E402

MODEL_ARG = {"hls": 0, "cpp": 1, "vhdl": 2}


def compile_sim(directory):
    exe = os.path.join(str(directory), "sim_build")
    subprocess.check_call(["g++", "-O2", "-o", exe, os.path.join(ROOT, "tools", "sim_build.cpp"), "-lquadmath"])
    return exe


def listed_entries(exe, model, pw, w, precision=1):
    """The entries the nibble + escapes format lists at this configuration, ascending (sim_build --escapes)."""
    r = subprocess.run([exe, "--escapes", str(MODEL_ARG[model]), str(pw), str(w), str(precision)], capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("listed entries:")]
    assert r.returncode == 0 and len(lines) == 1, (model, pw, w, r.returncode, r.stdout + r.stderr)
    return [int(v) for v in lines[0].split(":")[1].split()]


def records(exe):
    return [C.escape_record(t, listed_entries(exe, *C.TABLES[t][:3])) for t in C.ESC_TABLES]


def dumps(rows):
    return "[\n" + ",\n".join(" " + json.dumps(r) for r in rows) + "\n]\n"


def main(argv):
    with tempfile.TemporaryDirectory() as d:
        exe = compile_sim(d)
        rows = records(exe)
        sys.stdout.write(dumps(rows))
        if "--top" in argv:
            top = int(argv[argv.index("--top") + 1])
            for t in C.ESC_TABLES:
                model, pw, w = C.TABLES[t][:3]
                listed = np.asarray(listed_entries(exe, model, pw, w), dtype=np.int64)
                for name, cap in C.CAPS.items():
                    best = sorted(range(C.L_MIN, cap + 1), key=lambda n: (-len(C.reached(listed, n, pw)), -n))[:top]
                    print(t, name, [(n, len(C.reached(listed, n, pw))) for n in best])
    if "--write" in argv:
        with open(C.ESCAPES_JSON, "w") as f:
            f.write(dumps(rows))


if __name__ == "__main__":
    main(sys.argv[1:])
