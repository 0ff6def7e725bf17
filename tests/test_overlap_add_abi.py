"""Weighted overlap-add (bhw_overlap_add_device / bhw_overlap_add_from_table / bhw_overlap_add_describe): the checks that need no
GPU -- exports, every argument error before any HIP call, count == 0 as a no-op, the plan the describe line names, the C++ wrapper."""
import ctypes
import os
import subprocess

from blackman_harris_win_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "blackman_harris_win_amd")
BADARG, UNSUPPORTED = -1, -2

NEW_SYMBOLS = ("bhw_overlap_add_device", "bhw_overlap_add_from_table", "bhw_overlap_add_describe")
Y, X = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000)     # never dereferenced: every call below fails or has nothing to do


def test_new_symbols_are_exported_and_listed():
    L = B.lib()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
    assert L.bhw_abi_version() == 4
    assert ctypes.sizeof(B.BhwOla) == 56
    assert B.BhwOla.shift.offset == 48


def _dev(p, o, y=Y, x=X):
    return B.lib().bhw_overlap_add_device(ctypes.byref(p) if p is not None else None, 0, None,
                                          ctypes.byref(o) if o is not None else None, y, x)


def _desc(p, o, table=None):
    buf = ctypes.create_string_buffer(384)
    rc = B.lib().bhw_overlap_add_describe(table, ctypes.byref(p), ctypes.byref(o), buf, 384)
    return rc, buf.value.decode()


def _dbg_desc(pt, pc, o, table_format=B.TABLE_BEST):
    buf = ctypes.create_string_buffer(384)
    rc = B.lib().bhw_dbg_describe_ola_from_table(ctypes.byref(pt), table_format, ctypes.byref(pc), ctypes.byref(o), buf, 384)
    return rc, buf.value.decode()


def _err():
    return B.lib().bhw_last_error().decode()


def _whole(frames, hop, N, **kw):
    return B.make_ola(frames, hop, (frames - 1) * hop + N, **kw)


def test_argument_errors_come_before_any_hip_call():
    """BADARG / UNSUPPORTED whatever the machine: none of these reaches the device (the CPU tests run where there is none)."""
    p = B.make_params(B.WIN_BH7, 12, 32)
    N = 1 << 12
    ok = _whole(8, N // 4, N, shift=31)
    assert _dev(None, ok) == BADARG and "params" in _err()
    assert _dev(p, None) == BADARG and "NULL" in _err()
    cases = [
        ("channels", _whole(8, 1024, N, channels=0)), ("channels", _whole(8, 1024, N, channels=3)),
        ("hop", B.make_ola(8, 0, 100)), ("shift", _whole(8, 1024, N, shift=63)),
        ("y_stride", _whole(8, 1024, N, y_stride=N - 1)), ("y_stride", _whole(8, 1024, N, channels=2, y_stride=2 * N - 2)),
        ("frames", B.make_ola(0, 1024, 1)),
        ("2^34", B.make_ola((1 << 22) + 1, 1024, 1)),                               # frames * N
        ("extent", B.make_ola(3, 1 << 40, 1)),                                      # (frames - 1) * hop + N
        ("extent", B.make_ola(2, (1 << 64) - 1, 1)),                                # ... taken in 128 bits
        ("t0 + count", B.make_ola(8, 1024, 7 * 1024 + N + 1)),                      # one past the extent
        ("t0 + count", B.make_ola(8, 1024, 1, t0=7 * 1024 + N)),
        ("t0 + count", B.make_ola(8, 1024, 2, t0=(1 << 64) - 1)),
    ]
    for what, o in cases:
        assert _dev(p, o) == BADARG, what
        assert what in _err(), (what, _err())
        assert _desc(p, o)[0] == BADARG, what
    o = _whole(8, 1024, N)
    o.reserved = 1
    assert _dev(p, o) == BADARG and "reserved" in _err()
    o = _whole(8, 1024, N)
    o.struct_size = 40
    assert _dev(p, o) == BADARG and "struct_size" in _err()
    # NULL pointers
    assert _dev(p, ok, y=None) == BADARG and "NULL" in _err()
    assert _dev(p, ok, x=None) == BADARG and "NULL" in _err()
    # x over y: y spans (frames - 1) * y_stride + N * C int32 from its base, x count * C
    y = 0x10000000
    ye = (7 * N + N) * 4
    assert _dev(p, ok, y=ctypes.c_void_p(y), x=ctypes.c_void_p(y + ye - 4)) == BADARG and "overlap" in _err()
    xe = ((8 - 1) * (N // 4) + N) * 4
    assert _dev(p, ok, y=ctypes.c_void_p(y + xe - 4), x=ctypes.c_void_p(y)) == BADARG and "overlap" in _err()
    # adjacent ranges are fine up to the point of the HIP call (which this machine may not have): not BADARG for overlap
    rc = _dev(p, ok, y=ctypes.c_void_p(y), x=ctypes.c_void_p(y + ye))
    assert rc != BADARG or "overlap" not in _err()
    # a bad configuration is the parameter check's
    bad = B.make_params(B.WIN_BH4, 12, 16)
    bad.n_terms = 6
    assert _dev(bad, ok) == BADARG
    # the Taylor sources: no per-coefficient form to sum frames with, whatever the channels
    for st, nt in ((B.SIN_TAYLOR, B.WIN_HANN), (B.SIN_TAYLOR_ALL, B.WIN_BH7)):
        t = B.make_params(nt, 12, 16, sin_type=st)
        for C in (1, 2):
            assert _dev(t, _whole(8, 1024, N, channels=C)) == UNSUPPORTED
            assert "Taylor" in _err() and "generate" in _err(), _err()
            assert _desc(t, _whole(8, 1024, N, channels=C))[0] == UNSUPPORTED


def test_from_table_argument_errors():
    p = B.make_params(B.WIN_BH7, 12, 32)
    L = B.lib()
    o = _whole(8, 1024, 1 << 12)
    assert L.bhw_overlap_add_from_table(None, ctypes.byref(p), None, ctypes.byref(o), Y, X) == BADARG and "table is NULL" in _err()
    assert L.bhw_overlap_add_from_table(None, ctypes.byref(p), None, ctypes.byref(B.make_ola(0, 1, 0)), Y, X) == BADARG


def test_from_table_key_mismatch_and_checks():
    pt = B.make_params(B.WIN_BH7, 16, 24)
    other = B.make_params(B.WIN_BH7, 16, 25)
    assert _dbg_desc(pt, other, B.make_ola(4, 100, 10))[0] == BADARG and "dat_width" in _err()
    assert _dbg_desc(pt, pt, B.make_ola(4, 0, 10))[0] == BADARG and "hop" in _err()
    taylor = B.make_params(B.WIN_BH7, 16, 24, sin_type=B.SIN_TAYLOR_ALL)
    assert _dbg_desc(pt, taylor, B.make_ola(4, 100, 10))[0] == BADARG and "sin_type" in _err()


def test_zero_count_is_a_no_op():
    p = B.make_params(B.WIN_BH7, 12, 32)
    assert _dev(p, B.make_ola(8, 1024, 0), y=None, x=None) == 0
    assert _dev(p, B.make_ola(8, 1024, 0), y=Y, x=Y) == 0              # nothing is read or written, so nothing overlaps
    assert _dev(p, B.make_ola(0, 1024, 0), y=None, x=None) == 0        # no frames and nothing asked for
    assert _dev(p, B.make_ola(8, 1024, 0, t0=1 << 50), y=None, x=None) == 0
    rc, d = _desc(p, B.make_ola(8, 1024, 0))
    assert rc == 0 and "nothing" in d, d
    # the descriptor's own fields are still checked
    assert _dev(p, B.make_ola(8, 0, 0), y=None, x=None) == BADARG and "hop" in _err()


def test_describe_names_the_plan():
    # S1: BH-7 2^12 / 32 bits, hop N/4, 2^14 frames: 4 residue workgroups, Q = 16, the mad-form direct kernel
    p = B.make_params(B.WIN_BH7, 12, 32)
    rc, d = _desc(p, _whole(1 << 14, 1 << 10, 1 << 12))
    assert rc == 0 and d.startswith("overlap-add direct: k_ola_direct<2>, 1 channel, Q = 16 hops per lane"), d
    assert "up to 4 frames per output" in d and "grid 4 x 1025 x 256 lanes (256 along r, 1 along q)" in d, d
    # I/Q
    rc, d = _desc(B.make_params(B.WIN_BH4, 14, 16), _whole(1 << 11, 1 << 13, 1 << 14, channels=2))
    assert rc == 0 and "k_ola_direct<2>" in d and "2 channels" in d, d
    # a short hop spreads the workgroup over q as well: hop 3 -> 4 lanes along r, 64 along q
    rc, d = _desc(B.make_params(B.WIN_HANN, 8, 16), _whole(1000, 3, 1 << 8))
    assert rc == 0 and "(4 along r, 64 along q)" in d and "Q = 16" in d, d
    # hop 1: every lane along q
    rc, d = _desc(B.make_params(B.WIN_HANN, 8, 16), _whole(100, 1, 1 << 8))
    assert rc == 0 and "(1 along r, 256 along q)" in d, d
    # a long window: the residues fill the chip alone
    rc, d = _desc(B.make_params(B.WIN_BH7, 22, 32), _whole(16, 1 << 21, 1 << 22))
    assert rc == 0 and "grid 8192 x 2 x 256" in d and "up to 2 frames" in d, d
    # hop > N: gaps, one frame per output at most
    rc, d = _desc(B.make_params(B.WIN_BH7, 10, 32), _whole(5, 1029, 1 << 10))
    assert rc == 0 and "up to 1 frames per output" in d, d
    # from a table: the table kernel of the table's format
    pt = B.make_params(B.WIN_BH7, 26, 32)
    rc, d = _dbg_desc(pt, pt, B.make_ola(4, 1 << 25, 1 << 20))
    assert rc == 0 and d.startswith("overlap-add table: k_ola_table<3,7,0>"), d
    rc, d = _dbg_desc(pt, pt, B.make_ola(4, 1 << 25, 1 << 20), table_format=B.TABLE_PLAIN)
    assert rc == 0 and "k_ola_table<0,7,0>" in d, d
    nut = B.make_params(B.WIN_BH4, 26, 32, combine=B.COMBINE_VHDL, aa=B.coeffs_preset("nuttall", 32)[2])
    assert "k_ola_table<3,5,2>" in _dbg_desc(pt, nut, B.make_ola(4, 1 << 25, 1 << 20))[1]
    # the Python helper takes the whole extent by default
    assert B.describe_ola(p, 1 << 14, 1 << 10) == _desc(p, _whole(1 << 14, 1 << 10, 1 << 12))[1]


def test_cpp_overlap_add_compiles_and_links(tmp_path):
    src = tmp_path / "ola.cpp"
    src.write_text(r'''
#include <cstdio>
#include "bhw.hpp"
int main()
{
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH7, 12, 32);
    bhw_ola o = bhw::ola(16, 1024, 15 * 1024 + 4096, 31);
    if (o.struct_size != sizeof(bhw_ola) || sizeof(bhw_ola) != 56 || o.channels != 1 || o.t0 || o.reserved) return 3;
    o.hop = 0;
    try {
        bhw::overlap_add(p, o, nullptr, nullptr);      // hop 0: BADARG, before any HIP call
        return 4;
    } catch (const bhw::error &e) {
        std::printf("%d\n", e.code);
    }
    bhw::resident_table t;                              // empty handle: the member calls compile and fail loudly
    try {
        t.overlap_add(p, nullptr, o, nullptr, nullptr);
        return 5;
    } catch (const bhw::error &) {
    }
    try {
        (void)t.describe_overlap_add(p, o);
        return 6;
    } catch (const bhw::error &) {
    }
    return 0;
}
''')
    exe = str(tmp_path / "ola")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L" + PKG, "-lbhw", "-Wl,-rpath," + PKG], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "-1", (r.returncode, r.stdout, r.stderr)


def test_python_surface_is_exported():
    import blackman_harris_win_amd as bhw
    assert callable(bhw.overlap_add) and "overlap_add" in bhw.__all__ and "describe_ola" in bhw.__all__
    assert callable(bhw.ResidentTable.overlap_add) and callable(bhw.ResidentTable.describe_overlap_add)
    o = B.make_ola(3, 7, 21, t0=2, channels=2, shift=5, y_stride=40)
    assert (o.frames, o.hop, o.count, o.t0, o.channels, o.shift, o.y_stride) == (3, 7, 21, 2, 2, 5, 40)
    assert o.struct_size == ctypes.sizeof(B.BhwOla)
