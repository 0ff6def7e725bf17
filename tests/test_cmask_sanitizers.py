"""AddressSanitizer + UBSan over the planner's part of the fused STFT + complex gain + inverse STFT calls (bhw_plan.cpp, HIP-free), in a
stand-alone program with its own main (nothing is loaded into Python, nothing runs on a GPU): the checks, the plan and the describe
line of both families over all 8 + 73 supported n_fft at the edges of L, hop, frames and length, the 8-byte alignment and the overlaps
in 8-byte elements, and a lane-by-lane host replay of the gain-pair reads on float arrays of exactly the contract's size under every
stride form (tests/cpp/san_cmask.cpp): every float index 2 * (...) and 2 * (...) + 1 inside the extent and never in a gap, k
ascending and M - k descending, M odd and M even."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cmask_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_cmask")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_cmask.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 1000000 and int(r.stdout.split()[3]) > 1000 and "gain replays" in r.stdout
