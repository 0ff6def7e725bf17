"""AddressSanitizer + UBSan over the planner's part of the fused max-hold / min-hold calls for real input, both families
(bhw_plan.cpp, HIP-free), in a stand-alone program with its own main (nothing is loaded into Python, nothing runs on a GPU): the
argument checks -- both outputs NULL, each alone, every overlap -- the workspace bytes and the plan over all 9 + 95 supported n_fft
against L, hop, batch and frames at the edges of a chunk, a run and a block, and a lane-by-lane host replay of run ownership, the
live-slot mask, the reduce step in both regimes with bin M aside where the Welch siblings take it aside, and the two join launches with
the one-sided factor, on arrays of exactly the contract's sizes (tests/cpp/san_hold_real.cpp): every chunk pair written once and none
outside the workspace, every (b, f < F, k) reduced exactly once -- bin M by one owner -- and no f >= F at all, the traces equal to a
plain loop over the frames bit for bit, NaN and infinite powers included, and the trace not asked for untouched; the calls of 131 142
frames are among the replays.  The replay is a second copy of the kernels' index arithmetic, kept in step with bhw_hold_real.h,
bhw_hold_cfft.hip and the two row-function headers by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hold_real_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_hold_real")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "san_hold_real.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 1000000 and "call replays over 9 + 95 sizes" in r.stdout
