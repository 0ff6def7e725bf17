"""AddressSanitizer + UBSan over the planner's part of the fused multichannel filter-and-sum calls (bhw_plan.cpp, HIP-free), in a
stand-alone program with its own main (nothing is loaded into Python, nothing runs on a GPU): the checks, the plan and the describe
line of both families over all 8 + 73 supported n_fft at the edges of L, hop, frames, length and n_ch, the channel axis at its bounds,
the overlaps of d_out with the last channel of d_x and of d_g, and a lane-by-lane, channel-by-channel host replay of the sample reads
and the gain-pair reads on float arrays of exactly the contract's extents under every stride form (tests/cpp/san_beam.cpp): every
index inside the extent and never in a gap, M odd and M even."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_beam_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_beam")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_beam.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 1000000 and int(r.stdout.split()[3]) > 1000 and "read replays" in r.stdout
