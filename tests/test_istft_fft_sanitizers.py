"""AddressSanitizer + UBSan over the planner's part of the fused inverse FFT + overlap-add calls (bhw_plan.cpp, HIP-free): the argument
checks and the plan over every supported n_fft against L, hop, batch, frames and samples at the edges, the plan's invariants (LDS
within 64 KiB, S against the halo, the spans covering the outputs, grid within its bound), and host replays of the kernel's span
walk, pre-split, Stockham passes, ring and flush (tests/cpp/san_istft_fft.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_istft_fft_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_istft_fft")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_istft_fft.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 1000000
