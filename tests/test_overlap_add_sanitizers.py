"""AddressSanitizer + UBSan over the planner's part of the weighted overlap-add (bhw_plan.cpp, HIP-free): argument checks, Q, lane
layout, grid shape, overflow checks and the describe text, over a lattice of widths, hops, frame counts, channels, strides and output
ranges -- and, on small windows, a host replay of the kernel's lane arithmetic that every product is summed exactly once."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ola_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_ola")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    os.path.join(ROOT, "tests", "cpp", "san_ola.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 100000
