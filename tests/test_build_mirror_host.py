"""The mirror build kernel's short cuts at EVERY configuration the planner sends to it at PW 22..26 (no GPU): tools/sim_build.cpp,
the CPU model of k_table_build_mirror's arithmetic, compares every entry of every one of the 176 tables with the plain rotation
loop -- each configuration has its own ROM words, zero events, wide groups and tail-margin misses (test_build_algorithm.py runs
the same model at nine of them).  The same runs give, per configuration,

  * the deferred images of the fullest workgroup, for both workgroup shapes: the kernel's worklist holds kWorkMax = 8 x (groups per
    workgroup) of them, and its in-place fallback behind "list full" is reached only beyond that;
  * the entries outside the four-bit fields of the nibble formats and the longest escape list of one workgroup: the format the
    device settles on.  tests/golden/build_mirror_host.json pins them, and test_gpu_build_mirror_sweep.py holds the device to it.

`python tests/test_build_mirror_host.py --write` writes the fixture again and prints the per-configuration table kept in
profiles/r29_build_mirror_sweep.txt.
"""
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)                                                  # (run as a script: --write)

import build_mirror_cases as C  # noqa: E402

MODEL_ARG = {"hls": 0, "cpp": 1, "vhdl": 2}
FIGURES = re.compile(
    r"entries (?P<entries>\d+), groups (?P<groups>\d+), wide-state groups (?P<wide>\d+) .*unsafe tail lane (?P<unsafe_waves>\d+) \(lanes (?P<unsafe_lanes>\d+)\), "
    r"deferred images (?P<deferred>\d+) \(prefix zeros (?P<prefix_zeros>\d+)\), biased-narrow groups (?P<biased>\d+), mismatches (?P<mismatches>\d+), "
    r"deferred per workgroup max (?P<deferred_wg64>\d+) of 64 groups \| (?P<deferred_wg256>\d+) of 256 groups, cell log (?P<cell_log>\d+), "
    r"outside nibble fields (?P<nibble_misses>\d+), escape lists (?P<esc_total>\d+) \(max (?P<esc_wg_max>\d+) in one workgroup of (?P<wg_groups>\d+) groups\)")


def compile_sim(directory):
    exe = os.path.join(str(directory), "sim_build")
    subprocess.check_call(["g++", "-O2", "-o", exe, os.path.join(ROOT, "tools", "sim_build.cpp"), "-lquadmath"])
    return exe


def run_sweep(exe):
    """{configuration: figures} of all mirror configurations: one sim_build process each, at most 16 at a time."""
    def one(c):
        model, pw, w, precision = c
        r = subprocess.run([exe, str(MODEL_ARG[model]), str(pw), str(w), str(precision)], capture_output=True, text=True, timeout=600)
        m = FIGURES.search(r.stdout)
        assert r.returncode == 0 and m, (c, r.returncode, r.stdout + r.stderr)
        return c, {k: int(v) for k, v in m.groupdict().items()}
    cfgs = sorted(C.configurations(), key=lambda c: -c[1])                    # the long runs first
    with ThreadPoolExecutor(max_workers=max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        return dict(pool.map(one, cfgs))


def fixture_rows(sweep):
    return [{"model": c[0], "pw": c[1], "w": c[2], "precision": c[3], "nibble_misses": sweep[c]["nibble_misses"], "esc_wg_max": sweep[c]["esc_wg_max"]}
            for c in C.configurations()]


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    return run_sweep(compile_sim(tmp_path_factory.mktemp("sim_sweep")))


def test_every_entry_of_every_mirror_table_matches_the_plain_chain(sweep):
    assert len(sweep) == 176
    assert {c: f["mismatches"] for c, f in sweep.items() if f["mismatches"]} == {}
    for c, f in sweep.items():
        assert f["entries"] == 1 << (c[1] - 2) and f["cell_log"] == C.mirror_rule(*c)[2], (c, f)


def test_the_host_model_accepts_vhdl_at_pw_equal_w(sweep):
    """The only route to the 21-rotation instances <21, *, 256>: z_shr = 0 with z_shl = P (bhwp_resolve_cordic)."""
    assert C.mirror_rule("vhdl", 22, 22, 1)[0] == 21
    assert sweep[("vhdl", 22, 22, 1)]["mismatches"] == 0
    assert sum(1 for c in sweep if c[0] == "vhdl" and c[1] == c[2]) == 15         # PW == W at 22..26, precisions 1, 2 and 7


def test_worklist_never_fills(sweep):
    """kWorkMax = 8 x groups per workgroup: 512 at 64 groups (256 threads), 2 048 at 256 groups (1 024 threads).  Both shapes are
    counted at every configuration, whichever the dispatch picks, so the "list full" branch of the kernel is unreached at PW <= 26
    -- the fullest workgroup holds 72 of 512 (cpp at 26 / 32) and 250 of 2 048 (cpp at 22 / 28): a factor of seven to spare."""
    worst64 = max(sweep.values(), key=lambda f: f["deferred_wg64"])["deferred_wg64"]
    worst256 = max(sweep.values(), key=lambda f: f["deferred_wg256"])["deferred_wg256"]
    print("fullest worklist: %d of 512 (64 groups), %d of 2048 (256 groups)" % (worst64, worst256))
    for c, f in sweep.items():
        assert f["deferred_wg64"] < 8 * 64 and f["deferred_wg256"] < 8 * 256, (c, f)
        assert 7 * f["deferred_wg64"] < 8 * 64 and 7 * f["deferred_wg256"] < 8 * 256, (c, f)      # the margin the kernel's comment states
        assert f["deferred_wg64"] >= 1 and f["deferred"] >= 1, (c, f)             # the deferred path is taken everywhere (the middle entry at least)


def test_rare_paths_are_taken_somewhere(sweep):
    """What differs between the configurations is present in the sweep: wide groups, biased groups, waves outside the tail margins,
    zero events inside a shared prefix, entries outside the nibble fields, and both verdicts of each nibble format."""
    for key in ("wide", "biased", "unsafe_waves", "prefix_zeros", "nibble_misses", "esc_total"):
        assert any(f[key] for f in sweep.values()), key
    rows = {c: {"nibble_misses": f["nibble_misses"], "esc_wg_max": f["esc_wg_max"]} for c, f in sweep.items()}
    assert {C.predicted_format(r, "nibble") for r in rows.values()} == {"nibble", "nibble+esc", None}


def test_fixture_holds_these_figures(sweep):
    with open(C.HOST_JSON) as f:
        assert json.load(f) == fixture_rows(sweep)


def test_settled_table_of_the_build_loop_test_agrees():
    """test_gpu_build_loop.py pins the format nine (model, width) rows settle on at PW 25 and 26 (width 28: also 22), recorded from
    the device; the host figures predict the same."""
    from test_gpu_build_loop import SETTLED
    rows = C.host_rows()
    assert len(SETTLED) == 9
    for (model, width), name in SETTLED.items():
        for pw in (22, 25, 26) if width == 28 else (25, 26):
            if width == 28:
                assert name == "residual" and C.mirror_rule(model, pw, width, 1)      # reached under the residual limit: no narrower format is tried
            else:
                assert C.predicted_format(rows[(model, pw, width, 1)], "nibble") == name, (model, pw, width)


def write_records():
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        sweep = run_sweep(compile_sim(d))
    with open(C.HOST_JSON, "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in fixture_rows(sweep)) + "\n]\n")
    lines = ["model  PW  W  P  cell  groups  wide  biased  unsafe-waves  deferred  per-wg-max(64|256)  prefix-zeros  outside-nibble  esc-total  esc-wg-max  mismatches"]
    for c in C.configurations():
        f = sweep[c]
        lines.append("%-5s %3d %2d %2d %5d %7d %5d %7d %13d %9d %11d | %-6d %13d %15d %10d %11d %11d" % (
            c[0], c[1], c[2], c[3], f["cell_log"], f["groups"], f["wide"], f["biased"], f["unsafe_waves"], f["deferred"], f["deferred_wg64"],
            f["deferred_wg256"], f["prefix_zeros"], f["nibble_misses"], f["esc_total"], f["esc_wg_max"], f["mismatches"]))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    if "--write" in sys.argv:
        sys.stdout.write(write_records())
