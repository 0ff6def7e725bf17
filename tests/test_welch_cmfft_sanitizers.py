"""AddressSanitizer + UBSan over the planner's part of the fused Welch PSD calls for I/Q input at a mixed-radix n_fft (bhw_plan.cpp,
HIP-free), in a stand-alone program with its own main (nothing is loaded into Python, nothing runs on a GPU): the argument checks, the
workspace bytes and the plan over all 91 supported n_fft against L, hop, batch and frames at the edges of a chunk, a run and a block,
and a lane-by-lane host replay of run ownership, the padded frame map, the accumulate step in both regimes with the
compare-and-subtract column turn of BHW_CFFT_SHIFT and the two join launches on arrays of exactly the contract's sizes
(tests/cpp/san_welch_cmfft.cpp): every group visited once by the workgroup that owns it, every chunk sum written once and none outside
the workspace, every (b, f < F, k) added once in ascending f, P bit for bit the contract's three loops; the call of 131 142 frames is
among the replays.  The replay is a second copy of the kernel's index arithmetic, kept in step with bhw_welch_cmfft.hip and
bhw_stft_cmfft.h by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_welch_cmfft_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_welch_cmfft")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_welch_cmfft.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 1000000 and "call replays over 91 sizes" in r.stdout and "three-level sums" in r.stdout
