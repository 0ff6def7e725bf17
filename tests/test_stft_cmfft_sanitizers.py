"""AddressSanitizer + UBSan over the planner's part of the mixed-radix fused window + complex FFT calls for I/Q input (bhw_plan.cpp,
HIP-free): the argument checks of bhwp_stft_cmfft_checks and the plan swept over EVERY supported n_fft, flag combination and route,
and a host replay, lane by lane, at all 91 sizes, of the kernel's index arithmetic -- ownership of every row, every sample index
inside x under both padding modes, the order of the two means, i mod Ns by the float multiply, every point read and written exactly
once per pass, every twiddle index below the table's entries after the fold (never folded at an odd n_fft), the passes in float
against a direct binary64 DFT within 2^-24 * log2(n_fft), every output column written exactly once in both forms, with and without
the shift (tests/cpp/san_stft_cmfft.cpp).  A stand-alone program: nothing is loaded into Python under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stft_cmfft_planning_and_index_arithmetic_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_stft_cmfft")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_stft_cmfft.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    print(r.stdout.strip())
    words = r.stdout.replace(",", "").split()
    # checks, supported sizes (every 2^a 3^b 5^c in 16..2047 that is no power of two), the odd ones, refused sizes of 1..5000
    assert int(words[1]) > 1000000 and int(words[3]) == 91 and int(words[5]) == 18 and int(words[7]) == 4909
    worst = float(words[words.index("error") + 1])
    assert 0.0 < worst < 1.0                               # the worst float error as a share of the cap
