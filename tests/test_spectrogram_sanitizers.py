"""AddressSanitizer + UBSan over the planner's part of the fused spectrogram calls (bhw_plan.cpp, HIP-free): the argument checks of
bhwp_spectrogram_checks swept over every supported n_fft, both modes and the bank's refusals, the plan against the forward plan, and
a host replay, lane by lane, of the kernel's epilogue for consistent banks and for deliberately inconsistent ones -- every output
column written exactly once, every power read inside the slot's K floats, every weight read inside [0, weights)
(tests/cpp/san_spectrogram.cpp).  Inconsistent banks are tested only here, never on a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spectrogram_planning_and_epilogue_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_spectrogram")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_spectrogram.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    words = r.stdout.split()
    assert int(words[1]) > 1000000 and int(words[3]) >= 81 and int(words[6]) >= 500
