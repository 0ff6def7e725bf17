"""AddressSanitizer + UBSan over the planner's part of the resident tables (bhw_plan.cpp, HIP-free): creation checks, key match,
layout, format candidates, the kernel of every piece and the text of bhw_table_describe, over the parameter lattice."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resident_table_planning_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_resident")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    os.path.join(ROOT, "tests", "cpp", "san_resident.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 10000
