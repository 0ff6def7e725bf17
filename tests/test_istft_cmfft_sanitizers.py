"""AddressSanitizer + UBSan over the planner's part of the fused inverse mixed-radix complex FFT + overlap-add calls for I/Q output
(bhw_plan.cpp, HIP-free): the argument checks of bhwp_istft_cmfft_checks and the plan at EVERY supported n_fft, and a host replay, lane
by lane, of the kernel's index arithmetic -- at all 91 sizes every bin read once with and without the shift and the parts swapped,
every point read and written once per pass, every twiddle index below the table's entries after the fold (never folded at an odd
n_fft), the float32 row (the passes in float plus the multiply by fl32(1 / n_fft)) against a direct binary64 inverse DFT within
2^-24 * log2(n_fft); on the case table's geometries and a sweep every output pair stored once, inside x and never in a gap, the
products of an output exactly those of the frames reaching it in ascending f, every accumulator clear when a slot leaves a span, and
the stepped base mod n_fft equal to the true modulo (tests/cpp/san_istft_cmfft.cpp).  A stand-alone program: nothing is loaded into
Python under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_istft_cmfft_planning_and_index_arithmetic_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_istft_cmfft")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_istft_cmfft.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    print(r.stdout.strip())
    words = r.stdout.replace(",", "").split()
    # checks, supported sizes (every 2^a 3^b 5^c in 16..2047 that is no power of two), the odd ones, refused sizes of 1..5000
    assert int(words[1]) > 1000000 and int(words[3]) == 91 and int(words[5]) == 18 and int(words[7]) == 4909
    assert int(words[words.index("pass") - 1]) == 182        # every size, in order and shifted
    worst = float(words[words.index("error") + 1])
    assert 0.0 < worst < 1.0                               # the worst float error as a share of the cap
