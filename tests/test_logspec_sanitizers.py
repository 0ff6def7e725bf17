"""AddressSanitizer + UBSan over the planner's part of the fused log spectrogram / MFCC calls (bhw_plan.cpp, HIP-free): the checks of
bhwp_logspec_checks swept over every supported n_fft of both radix families and every refusal of the log descriptor in the header's
order, the plans against their parents', and a host replay, lane by lane, of the kernels' epilogue (log_row of bhw_logspec.h) for
consistent banks and for deliberately inconsistent ones -- every output column written exactly once, every read inside its array, the
log row never read before the second barrier and never written while a power may still be formed (tests/cpp/san_logspec.cpp).  A
stand-alone program; inconsistent banks are tested only here, never on a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_logspec_planning_and_epilogue_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_logspec")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_logspec.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    words = r.stdout.split()
    assert int(words[1]) > 1000000 and int(words[3]) == 104 and int(words[5]) >= 1000 and int(words[8]) >= 1000
