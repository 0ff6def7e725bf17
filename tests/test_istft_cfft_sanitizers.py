"""AddressSanitizer + UBSan over the planner's part of the fused inverse complex FFT + overlap-add calls (bhw_plan.cpp, HIP-free): the
argument checks and their order, the plan over every supported n_fft against L, hop, batch, frames and samples at the edges with all
four flag combinations, the plan's invariants (LDS within 48 KiB, the forward's lanes and passes, S against the halo, the spans
covering the outputs, grid within its bound), and host replays of the kernel's span walk, load (shifted and in order), inverse
Stockham passes in float against a direct binary64 inverse DFT, ring and flush (tests/cpp/san_istft_cfft.cpp).  A stand-alone
program: nothing of it is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_istft_cfft_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_istft_cfft")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_istft_cfft.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 1000000
    # the float32 inverse passes against a direct binary64 inverse DFT: the largest relative l2 error as a share of 2^-24 * log2 n
    print(r.stdout.strip())
    share = float(re.search(r"worst error ([0-9.]+) of the cap", r.stdout).group(1))
    assert 0.0 < share <= 1.0, r.stdout
