"""AddressSanitizer + UBSan over the planner's part of the fused inverse mixed-radix FFT + overlap-add calls (bhw_plan.cpp, HIP-free), in
a stand-alone program with its own main (nothing is loaded into Python, nothing runs on a GPU): the argument checks and the plan over
every supported n_fft against L, hop, batch, frames and samples at the edges, the plan's invariants, and a lane-by-lane host replay of
the kernel's pre-split (odd and even M), Stockham passes (the float i mod Ns, the twiddle fold), float32 row against a binary64
inverse DFT under 2^-24 * log2(n_fft), span walk, ring with its stepped base mod n_fft, and flush (tests/cpp/san_istft_mfft.cpp).  The
replay is a second copy of the kernel's index arithmetic, kept in step with bhw_istft_mfft.hip by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_istft_mfft_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_istft_mfft")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_istft_mfft.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 1000000 and "95 pass replays" in r.stdout
