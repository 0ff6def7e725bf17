"""AddressSanitizer + UBSan over the planner's part of the batched, centred STFT framing and overlap-add (bhw_plan.cpp, HIP-free): the
argument checks and plans over a lattice of batches, lengths, FFT sizes, window lengths, hops, channels and pad modes, and host replays
of the frames kernel's lane and row-pool arithmetic, of the reflect map and of the batched overlap-add (tests/cpp/san_stft.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stft_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_stft")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_stft.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 1000000
