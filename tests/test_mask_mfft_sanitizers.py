"""AddressSanitizer + UBSan over the planner's part of the mixed-radix fused STFT + mask + inverse STFT calls (bhw_plan.cpp, HIP-free),
in a stand-alone program with its own main (nothing is loaded into Python, nothing runs on a GPU): the checks, the plan and the
describe line over all 73 supported n_fft at the edges of L, hop, frames and length, and a lane-by-lane host replay of the index
arithmetic that is new in bhw_mask_mfft.hip on arrays of exactly the contract's sizes (tests/cpp/san_mask_mfft.cpp): every sample
index inside [0, T) under both padding rules, every gain index inside its extent under every stride form, the forward pass indices
and the float i mod Ns, no phase writing the buffer it reads for either parity of the pass count, every pre-split point (M odd and M
even) and every output written once.  The replay is a second copy of the kernel's index arithmetic, kept in step with
bhw_mask_mfft.hip, bhw_stft_mfft.h and bhw_istft_mfft.h by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mask_mfft_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_mask_mfft")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_mask_mfft.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 1000000 and int(r.stdout.split()[3]) > 1000 and "call replays" in r.stdout
