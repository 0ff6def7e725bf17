"""AddressSanitizer + UBSan over the planner's part of the Welch cross spectra (bhw_plan.cpp, HIP-free): the argument checks, workspace
sizes and plans over a lattice of B, F (1, 2, BLOCK - 1, BLOCK, BLOCK + 1, many), K, strides, output masks and the broadcast flag, and a
host replay of the kernel's ownership: every (b, f, k) loaded once per operand and entering each chain once, in ascending f within its
block, the block sums joined in block order, the plan's LDS within 64 KiB (tests/cpp/san_csd.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_csd_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_csd")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_csd.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 1000000
