"""AddressSanitizer + UBSan over the planner's part of the fused window + complex FFT calls for I/Q input (bhw_plan.cpp, HIP-free):
the argument checks of bhwp_stft_cfft_checks and the plan swept over every supported n_fft and flag combination, and a host replay,
lane by lane, of the kernel's index arithmetic -- every sample index inside x under both padding modes, the order of the two means,
every point written exactly once per pass, the passes in float against a direct binary64 DFT within 2^-24 * log2(n_fft), every output
column written exactly once with and without the shift (tests/cpp/san_stft_cfft.cpp).  A stand-alone program: nothing is loaded into
Python under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stft_cfft_planning_and_index_arithmetic_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_stft_cfft")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_stft_cfft.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    words = r.stdout.split()
    assert int(words[1]) > 1000000 and int(words[3]) > 2000 and int(words[6]) == 24
