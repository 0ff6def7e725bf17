"""AddressSanitizer + UBSan over the planner's part of the fused STFT + gain + inverse STFT calls for I/Q input (bhw_plan.cpp,
HIP-free), in a stand-alone program with its own main (nothing is loaded into Python, nothing runs on a GPU): the checks, the plan and
the describe line of both families over all 8 + 91 supported n_fft at the edges of L, hop, frames and length, the overlap of d_out
with the second half of d_x's last complex sample, and a lane-by-lane host replay, on float arrays of exactly the contract's size, of
the sample reads (floats 2 t and 2 t + 1, 8-byte and 4-byte forms, reflection at both ends, T below the pad) and of the gain reads
under every stride form, with and without the shift, n_fft odd and even (tests/cpp/san_mask_iq.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mask_iq_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_mask_iq")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_mask_iq.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    words = r.stdout.split()
    assert int(words[1]) > 1000000 and int(words[3]) > 10000 and "sample replays" in r.stdout and "gain replays" in r.stdout
