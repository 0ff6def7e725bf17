"""AddressSanitizer + UBSan over the planner's part of the float32 frame apply and overlap-add (bhw_plan.cpp, HIP-free): the argument
checks, the float32 frames plans (never the per-frame route), the describe text -- and, on small windows, a host replay of the float32
overlap-add's lane arithmetic that every product is summed exactly once and in ascending frame order."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_f32_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_f32")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_f32.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 100000
