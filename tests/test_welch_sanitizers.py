"""AddressSanitizer + UBSan over the planner's part of Welch's method around the FFT (bhw_plan.cpp, HIP-free): the argument checks,
workspace sizes and plans over a lattice of batches, signal lengths, window lengths, FFT sizes, hops and channels with the frame count
at 1, BLOCK - 1, BLOCK, BLOCK + 1 and many, and host replays of the mean order, of the lane and row ownership of the segments kernel,
of the block cut of the periodogram and of the join of the split sum-of-squares counters at its bound (tests/cpp/san_welch.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_welch_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_welch")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_welch.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 1000000
