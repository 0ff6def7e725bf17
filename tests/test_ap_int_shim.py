"""AddressSanitizer + UBSan over oracle/shim/ap_int.h, the project's stand-in for the arbitrary-width integer header that the
reference's HLS sources include (oracle/Makefile compiles them against it into oracle/_ref).  tests/cpp/san_ap_int_shim.cpp holds the
contract written at the top of the header -- compute exactly, wrap on every store -- against unsigned __int128 arithmetic and
hand-computed constants: wraps at widths 1 .. 127, sign extension, << at the width of its left operand, >> of negative values,
~x + 1, double construction, the 65 x 32-bit product of the cosine sum, and the quadrant taken from a negative phase."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ap_int_shim_contract_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_ap_int_shim")
    subprocess.run(["g++", "-g", "-O1", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    "-I" + os.path.join(ROOT, "oracle", "shim"), os.path.join(ROOT, "tests", "cpp", "san_ap_int_shim.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 100000
