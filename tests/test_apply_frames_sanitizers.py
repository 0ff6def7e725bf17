"""AddressSanitizer + UBSan over the planner's part of the overlapped-frame apply (bhw_plan.cpp, HIP-free): argument checks, route
rule, frame-group size, grid shape, overflow checks and the describe text, over a lattice of widths, hops, frame counts, channels and
strides."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frames_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_frames")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    os.path.join(ROOT, "tests", "cpp", "san_frames.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 100000
