"""Overlapped-frame apply (bhw_apply_frames_device / bhw_apply_frames_from_table / bhw_apply_frames_describe): the checks that need
no GPU -- exports, every argument error before any HIP call, frames == 0 as a no-op, the route the planner names, the C++ wrapper."""
import ctypes
import os
import subprocess

import pytest

from blackman_harris_win_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "blackman_harris_win_amd")
BADARG, UNSUPPORTED = -1, -2

NEW_SYMBOLS = ("bhw_apply_frames_device", "bhw_apply_frames_from_table", "bhw_apply_frames_describe")
X, Y = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000)     # never dereferenced: every call below fails or has nothing to do


def test_new_symbols_are_exported_and_listed():
    L = B.lib()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
    assert L.bhw_abi_version() == 4
    assert ctypes.sizeof(B.BhwFrames) == 40


def _dev(p, f, x=X, y=Y):
    return B.lib().bhw_apply_frames_device(ctypes.byref(p) if p is not None else None, 0, None,
                                           ctypes.byref(f) if f is not None else None, x, y)


def _tab(p, f, x=X, y=Y):
    return B.lib().bhw_apply_frames_from_table(ctypes.c_void_p(0x1000) if p is not None else None,
                                               ctypes.byref(p) if p is not None else None, None, ctypes.byref(f), x, y)


def _desc(p, f, table=None):
    buf = ctypes.create_string_buffer(384)
    rc = B.lib().bhw_apply_frames_describe(table, ctypes.byref(p), ctypes.byref(f), buf, 384)
    return rc, buf.value.decode()


def _err():
    return B.lib().bhw_last_error().decode()


def test_argument_errors_come_before_any_hip_call():
    """BADARG / UNSUPPORTED whatever the machine: none of these reaches the device (the CPU tests run where there is none)."""
    p = B.make_params(B.WIN_BH7, 12, 32)
    N = 1 << 12
    ok = B.make_frames(8, N // 4, shift=31)
    assert _dev(None, ok) == BADARG
    assert _dev(p, None) == BADARG
    cases = [
        ("channels", B.make_frames(8, 1024, channels=0)), ("channels", B.make_frames(8, 1024, channels=3)),
        ("hop", B.make_frames(8, 0)), ("shift", B.make_frames(8, 1024, shift=63)),
        ("y_stride", B.make_frames(8, 1024, y_stride=N - 1)), ("y_stride", B.make_frames(8, 1024, channels=2, y_stride=2 * N - 2)),
        ("2^34", B.make_frames((1 << 22) + 1, 1024)),
    ]
    for what, f in cases:
        assert _dev(p, f) == BADARG, what
        assert what in _err(), (what, _err())
        assert _desc(p, f)[0] == BADARG, what
    f = B.make_frames(8, 1024)
    f.reserved = 1
    assert _dev(p, f) == BADARG and "reserved" in _err()
    f = B.make_frames(8, 1024)
    f.struct_size = 32
    assert _dev(p, f) == BADARG and "struct_size" in _err()
    # NULL pointers
    assert _dev(p, ok, x=None) == BADARG and "NULL" in _err()
    assert _dev(p, ok, y=None) == BADARG and "NULL" in _err()
    # y over x: x spans ((frames - 1) * hop + N) * C int32 from its base, y (frames - 1) * y_stride + N * C
    x = 0x10000000
    xe = ((8 - 1) * (N // 4) + N) * 4
    assert _dev(p, ok, x=ctypes.c_void_p(x), y=ctypes.c_void_p(x + xe - 4)) == BADARG and "overlap" in _err()
    assert _dev(p, ok, x=ctypes.c_void_p(x + 8 * N * 4 - 4), y=ctypes.c_void_p(x)) == BADARG and "overlap" in _err()
    # a bad configuration is the parameter check's
    bad = B.make_params(B.WIN_BH4, 12, 16)
    bad.n_terms = 6
    assert _dev(bad, ok) == BADARG
    # Taylor with two channels: the per-frame route has no I/Q form
    t = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    assert _dev(t, B.make_frames(8, 1024, channels=2)) == UNSUPPORTED
    assert _desc(t, B.make_frames(8, 1024, channels=2))[0] == UNSUPPORTED


def test_from_table_argument_errors():
    p = B.make_params(B.WIN_BH7, 12, 32)
    assert _tab(None, B.make_frames(8, 1024)) == BADARG and "table is NULL" in _err()
    L = B.lib()
    assert L.bhw_apply_frames_from_table(None, ctypes.byref(p), None, ctypes.byref(B.make_frames(0, 1)), X, Y) == BADARG


def _dbg_desc(pt, pc, f, table_format=B.TABLE_BEST):
    buf = ctypes.create_string_buffer(384)
    rc = B.lib().bhw_dbg_describe_frames_from_table(ctypes.byref(pt), table_format, ctypes.byref(pc), ctypes.byref(f), buf, 384)
    return rc, buf.value.decode()


def test_from_table_key_mismatch_and_frame_checks():
    pt = B.make_params(B.WIN_BH7, 16, 24)
    other = B.make_params(B.WIN_BH7, 16, 25)
    assert _dbg_desc(pt, other, B.make_frames(4, 100))[0] == BADARG and "dat_width" in _err()
    assert _dbg_desc(pt, pt, B.make_frames(4, 0))[0] == BADARG and "hop" in _err()
    taylor = B.make_params(B.WIN_BH7, 16, 24, sin_type=B.SIN_TAYLOR_ALL)
    assert _dbg_desc(pt, taylor, B.make_frames(4, 100))[0] == BADARG and "sin_type" in _err()


def test_zero_frames_is_a_no_op():
    p = B.make_params(B.WIN_BH7, 12, 32)
    assert _dev(p, B.make_frames(0, 1024), x=None, y=None) == 0
    assert _dev(p, B.make_frames(0, 1024), x=X, y=X) == 0            # nothing is read or written, so nothing overlaps
    rc, d = _desc(p, B.make_frames(0, 1024))
    assert rc == 0, _err()


def test_describe_names_the_route():
    # short window, many frames: the frames kernel with the direct CORDIC source, frame groups sized to fill the chip
    p = B.make_params(B.WIN_BH7, 12, 32)
    rc, d = _desc(p, B.make_frames(1 << 14, 1 << 10))
    assert rc == 0 and d.startswith("frames kernel: k_frames_direct<2>"), d
    assert "G = 64 frames per lane" in d and "grid 16 x 256" in d, d
    rc, d = _desc(B.make_params(B.WIN_BH4, 14, 16), B.make_frames(1 << 11, 1 << 13, channels=2))
    assert rc == 0 and "k_frames_direct<2>" in d and "2 channels" in d, d
    # windows shorter than a workgroup: several frames side by side
    rc, d = _desc(B.make_params(B.WIN_HANN, 4, 16), B.make_frames(1000, 3))
    assert rc == 0 and "(16 along k)" in d, d
    # Taylor: one bhw_apply_device per frame
    t = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    rc, d = _desc(t, B.make_frames(16, 1024))
    assert rc == 0 and d.startswith("per-frame: 16 x bhw_apply_device") and "taylor" in d, d
    # a long window with a single frame: the per-frame route; with many frames the frames kernel
    long = B.make_params(B.WIN_BH7, 22, 32)
    assert _desc(long, B.make_frames(1, 1 << 21))[1].startswith("per-frame"), _desc(long, B.make_frames(1, 1 << 21))
    assert _desc(long, B.make_frames(7, 1 << 21))[1].startswith("per-frame")           # the crossover at 2^22: 8 frames
    assert _desc(long, B.make_frames(8, 1 << 21))[1].startswith("frames kernel"), _desc(long, B.make_frames(8, 1 << 21))
    assert _desc(B.make_params(B.WIN_BH7, 17, 32), B.make_frames(1, 1 << 16))[1].startswith("frames kernel")   # below 2^18: never
    # ... and always the frames kernel for I/Q
    assert _desc(long, B.make_frames(1, 1 << 21, channels=2))[1].startswith("frames kernel")
    # from a table: the table kernel of the table's format
    pt = B.make_params(B.WIN_BH7, 26, 32)
    rc, d = _dbg_desc(pt, pt, B.make_frames(1, 1 << 25))
    assert rc == 0 and d.startswith("frames kernel: k_frames_table<3,7,0>"), d
    rc, d = _dbg_desc(pt, pt, B.make_frames(8, 1 << 20), table_format=B.TABLE_PLAIN)
    assert rc == 0 and "k_frames_table<0,7,0>" in d, d
    nut = B.make_params(B.WIN_BH4, 26, 32, combine=B.COMBINE_VHDL, aa=B.coeffs_preset("nuttall", 32)[2])
    assert "k_frames_table<3,5,2>" in _dbg_desc(pt, nut, B.make_frames(8, 1 << 20))[1]


def test_cpp_apply_frames_compiles_and_links(tmp_path):
    src = tmp_path / "af.cpp"
    src.write_text(r'''
#include <cstdio>
#include "bhw.hpp"
int main()
{
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH7, 12, 32);
    bhw_frames f = bhw::frames(16, 1024, 31);
    if (f.struct_size != sizeof(bhw_frames) || f.channels != 1 || f.reserved) return 3;
    f.hop = 0;
    try {
        bhw::apply_frames(p, f, nullptr, nullptr);      // hop 0: BADARG, before any HIP call
        return 4;
    } catch (const bhw::error &e) {
        std::printf("%d\n", e.code);
    }
    return 0;
}
''')
    exe = str(tmp_path / "af")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L" + PKG, "-lbhw", "-Wl,-rpath," + PKG], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "-1", (r.returncode, r.stdout, r.stderr)


@pytest.mark.parametrize("channels", [1, 2])
def test_python_surface_is_exported(channels):
    import blackman_harris_win_amd as bhw
    assert callable(bhw.apply_frames) and "apply_frames" in bhw.__all__
    assert callable(bhw.ResidentTable.apply_frames)
    f = B.make_frames(3, 7, channels=channels)
    assert f.channels == channels and f.struct_size == ctypes.sizeof(B.BhwFrames)
