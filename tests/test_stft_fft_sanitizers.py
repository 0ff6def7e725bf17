"""AddressSanitizer + UBSan over the planner's part of the fused window + FFT calls (bhw_plan.cpp, HIP-free): the argument checks and
the plan over every supported n_fft against L, hop, batch and frames at the edges, the plan's invariants (LDS within 64 KiB, every row
owned by exactly one workgroup slot, grid within its bound), and host replays of the kernel's group loop, loads, mean order, Stockham
passes and stores (tests/cpp/san_stft_fft.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stft_fft_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_stft_fft")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_stft_fft.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 1000000
