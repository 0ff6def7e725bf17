"""AddressSanitizer + UBSan over the host side of the windows of any length (bhw_len.h, bhw_plan.cpp, HIP-free): the phase map against
exact integer arithmetic with the no-tie property, the argument checks and the frames / overlap-add plans for any L, and a host replay of
the overlap-add lane arithmetic at non-power-of-two L.  The same binary then maps random (L, P, m) up to L = 2^30 and 64-bit indices,
which are compared here with Python integers."""
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "san_len")
    csrc = os.path.join(ROOT, "blackman_harris_win_amd", "csrc")
    subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                    os.path.join(ROOT, "tests", "cpp", "san_len.cpp"), os.path.join(csrc, "bhw_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    return exe


def theta_exact(L, P, n, k=1):
    """round(((k * (n mod L)) mod L) * 2^P / L) mod 2^P, in Python integers (no ties can occur: asserted)."""
    mk = (k * (n % L)) % L
    q, r = divmod(mk << P, L)
    assert 2 * r != L
    return (q + (2 * r > L)) % (1 << P)


def test_len_host_side_clean_under_asan_ubsan(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.split()[1]) > 1000000


def test_phase_map_matches_python_integers(tmp_path):
    rng = random.Random(20261016)
    cases = []
    for _ in range(20000):
        P = rng.randint(4, 30)
        L = rng.randint(1, 1 << P)
        n = rng.getrandbits(64) if rng.random() < 0.5 else rng.randrange(L)
        cases.append((L, P, n))
    for P in (24, 30):                                  # the extremes: L = 2^30, L = 2^P - 1, the largest index
        for L in (1, 2, 3, (1 << P) - 1, 1 << P, 3 << (P - 2)):
            cases += [(L, P, 0), (L, P, L - 1), (L, P, (1 << 64) - 1), (L, P, (1 << 40) + 5)]
    src = tmp_path / "cases.txt"
    src.write_text("".join(f"{L} {P} {n}\n" for L, P, n in cases))
    r = subprocess.run([_build(tmp_path), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(v) for v in r.stdout.split()]
    assert len(got) == len(cases)
    bad = [(c, g) for c, g in zip(cases, got) if g != theta_exact(*c)]
    assert not bad, bad[:5]
    # at L = 2^P the map is the identity of the power-of-two windows
    assert all(theta_exact(1 << P, P, n) == n % (1 << P) for P in (4, 12, 30) for n in (0, 5, (1 << P) - 1, 1 << 40))
