"""Windows of any length (bhw_*_len_* / bhw_describe_len): the checks that need no GPU -- exports, every argument error before any HIP
call, the describe lines (L = 2^phi_width takes the existing routes), the C++ wrapper and the Python surface."""
import ctypes
import os
import subprocess

import pytest

from blackman_harris_win_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "blackman_harris_win_amd")
BADARG, UNSUPPORTED = -1, -2

NEW_SYMBOLS = ("bhw_generate_len_device", "bhw_generate_len_from_table", "bhw_apply_frames_len_device", "bhw_apply_frames_len_from_table",
               "bhw_overlap_add_len_device", "bhw_overlap_add_len_from_table", "bhw_describe_len")
A, Z = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000)     # never dereferenced: every call below fails or has nothing to do


def _err():
    return B.lib().bhw_last_error().decode()


def _desc(p, length, n0=0, count=None, f=None, o=None):
    buf = ctypes.create_string_buffer(512)
    rc = B.lib().bhw_describe_len(None, ctypes.byref(p), int(length), int(n0), int(length if count is None else count),
                                  ctypes.byref(f) if f is not None else None, ctypes.byref(o) if o is not None else None, buf, 512)
    return rc, buf.value.decode()


def test_new_symbols_are_exported_and_listed():
    L = B.lib()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
    assert hasattr(L, "bhw_dbg_len_force_kernels") and "bhw_dbg_len_force_kernels" not in B.ABI_SYMBOLS
    assert L.bhw_abi_version() == 4


def test_length_and_source_errors_come_before_any_hip_call():
    L = B.lib()
    p = B.make_params(B.WIN_BH7, 12, 32)
    f = B.make_frames(4, 100)
    o = B.make_ola(4, 100, 700)
    calls = (
        lambda q, n: L.bhw_generate_len_device(q, n, 0, None, 0, 10, A),
        lambda q, n: L.bhw_generate_len_from_table(None, q, n, None, 0, 10, A),
        lambda q, n: L.bhw_apply_frames_len_device(q, n, 0, None, ctypes.byref(f), A, Z),
        lambda q, n: L.bhw_apply_frames_len_from_table(None, q, n, None, ctypes.byref(f), A, Z),
        lambda q, n: L.bhw_overlap_add_len_device(q, n, 0, None, ctypes.byref(o), A, Z),
        lambda q, n: L.bhw_overlap_add_len_from_table(None, q, n, None, ctypes.byref(o), A, Z),
    )
    for call in calls:
        assert call(None, 400) == BADARG and "params" in _err()
        assert call(ctypes.byref(p), 0) == BADARG and "length 0" in _err(), _err()
        assert call(ctypes.byref(p), (1 << 12) + 1) == BADARG and "length" in _err()
        taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
        assert call(ctypes.byref(taylor), 400) == UNSUPPORTED and "CORDIC" in _err(), _err()
        dds = B.make_params(B.WIN_BH7, 12, 32)
        dds.model = B.MODEL_DDS48
        assert call(ctypes.byref(dds), 400) == UNSUPPORTED
    # from a table: a NULL handle after the length checks
    assert L.bhw_generate_len_from_table(None, ctypes.byref(p), 400, None, 0, 10, A) == BADARG and "table is NULL" in _err()
    assert L.bhw_apply_frames_len_from_table(None, ctypes.byref(p), 400, None, ctypes.byref(f), A, Z) == BADARG and "table" in _err()
    assert L.bhw_overlap_add_len_from_table(None, ctypes.byref(p), 400, None, ctypes.byref(o), A, Z) == BADARG and "table" in _err()


def test_descriptor_errors_use_the_length():
    L = B.lib()
    p = B.make_params(B.WIN_BH7, 12, 32)
    # y_stride below L * C: 400 is enough for L = 400 (no error from the stride) but not for L = 401
    f = B.make_frames(4, 100, y_stride=400)
    assert L.bhw_apply_frames_len_device(ctypes.byref(p), 401, 0, None, ctypes.byref(f), A, A) == BADARG and "y_stride" in _err()
    # d_x and d_y overlap at L = 400 (a stride-400 check passed first)
    assert L.bhw_apply_frames_len_device(ctypes.byref(p), 400, 0, None, ctypes.byref(f), A, A) == BADARG and "overlap" in _err()
    # frames * L above 2^34
    big = B.make_frames((1 << 34) // 400 + 1, 400)
    assert L.bhw_apply_frames_len_device(ctypes.byref(p), 400, 0, None, ctypes.byref(big), A, Z) == BADARG and "2^34" in _err()
    assert L.bhw_apply_frames_len_device(ctypes.byref(p), 400, 0, None, ctypes.byref(B.make_frames(4, 0)), A, Z) == BADARG
    # overlap-add: the extent is (frames - 1) * hop + L
    o = B.make_ola(4, 100, 3 * 100 + 401)
    assert L.bhw_overlap_add_len_device(ctypes.byref(p), 400, 0, None, ctypes.byref(o), A, Z) == BADARG and "extent" in _err()
    o = B.make_ola(4, 100, 3 * 100 + 400, y_stride=399)
    assert L.bhw_overlap_add_len_device(ctypes.byref(p), 400, 0, None, ctypes.byref(o), A, Z) == BADARG and "y_stride" in _err()
    # a generate range: NULL output, count above 2^34
    assert L.bhw_generate_len_device(ctypes.byref(p), 400, 0, None, 0, 10, None) == BADARG and "d_out" in _err()
    assert L.bhw_generate_len_device(ctypes.byref(p), 400, 0, None, 0, (1 << 34) + 1, A) == BADARG and "2^34" in _err()
    # nothing to do: no HIP call either
    assert L.bhw_generate_len_device(ctypes.byref(p), 400, 0, None, 5, 0, None) == 0
    assert L.bhw_apply_frames_len_device(ctypes.byref(p), 400, 0, None, ctypes.byref(B.make_frames(0, 100)), None, None) == 0
    assert L.bhw_overlap_add_len_device(ctypes.byref(p), 400, 0, None, ctypes.byref(B.make_ola(4, 100, 0)), None, None) == 0


def test_describe_names_the_route():
    p = B.make_params(B.WIN_BH7, 12, 32)
    N = 1 << 12
    # L = 2^P: the existing route, with the existing describe text after the prefix
    rc, d = _desc(p, N, 0, N)
    assert rc == 0 and d == "power-of-two route (L = 2^12): " + B.describe_plan(p, 0, N), d
    f = B.make_frames(64, N // 4)
    rc, d = _desc(p, N, f=f)
    assert rc == 0 and d == "power-of-two route (L = 2^12): " + B.describe_frames(p, 64, N // 4), d
    o = B.make_ola(64, N // 4, 63 * N // 4 + N)
    rc, d = _desc(p, N, o=o)
    assert rc == 0 and d == "power-of-two route (L = 2^12): " + B.describe_ola(p, 64, N // 4), d
    # any other length: the any-length kernels
    rc, d = _desc(p, 400, 5, 1000)
    assert rc == 0 and d.startswith("any-length route (L = 400, phi_width 12): k_direct_len<2>"), d
    assert "n0 mod L = 5" in d
    rc, d = _desc(p, 400, f=B.make_frames(1 << 16, 160))
    assert rc == 0 and "k_frames_direct_len<2>" in d and "grid 2 x " in d and "(256 along k)" in d, d
    rc, d = _desc(p, 100, f=B.make_frames(1000, 40))
    assert rc == 0 and "grid 1 x " in d and "(128 along k)" in d, d
    rc, d = _desc(p, 1000, o=B.make_ola(64, 250, 63 * 250 + 1000))
    assert rc == 0 and "k_ola_direct_len<2>" in d and "up to 4 frames per output" in d, d
    # the 64-bit-state configurations take the other direct forms
    wide = B.make_params(B.WIN_BH7, 24, 32, model=B.MODEL_CPP)
    rc, d = _desc(wide, 1000)
    assert rc == 0 and "k_direct_len<" in d, d
    # both descriptors: refused
    buf = ctypes.create_string_buffer(64)
    assert B.lib().bhw_describe_len(None, ctypes.byref(p), 400, 0, 400, ctypes.byref(f), ctypes.byref(o), buf, 64) == BADARG
    # the Python helper
    assert B.describe_len(p, 400, n0=5, count=1000) == _desc(p, 400, 5, 1000)[1]
    assert B.describe_len(p, 400, frames=B.make_frames(1 << 16, 160)).startswith("any-length route")


def test_forcing_the_any_length_kernels_changes_the_route():
    L = B.lib()
    p = B.make_params(B.WIN_BH7, 12, 32)
    prev = L.bhw_dbg_len_force_kernels(1)
    try:
        rc, d = _desc(p, 1 << 12)
        assert rc == 0 and d.startswith("any-length route (L = 4096, phi_width 12): k_direct_len<2>"), d
    finally:
        L.bhw_dbg_len_force_kernels(prev)
    assert _desc(p, 1 << 12)[1].startswith("power-of-two route")


def test_cpp_len_wrappers_compile_and_link(tmp_path):
    src = tmp_path / "len.cpp"
    src.write_text(r'''
#include <cstdio>
#include "bhw.hpp"
int main()
{
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH7, 12, 32);
    if (bhw::describe_len(p, 400, 0, 400).rfind("any-length route", 0) != 0) return 2;
    bhw_frames f = bhw::frames(4, 160, 31);
    if (bhw::describe_len(p, 4096, 0, 0, &f).rfind("power-of-two route", 0) != 0) return 3;
    try {
        bhw::generate_len(p, 0, 0, 10, nullptr);           // length 0: BADARG, before any HIP call
        return 4;
    } catch (const bhw::error &e) {
        std::printf("%d\n", e.code);
    }
    try {
        bhw::apply_frames_len(p, 5000, f, nullptr, nullptr);
        return 5;
    } catch (const bhw::error &) {
    }
    bhw_ola o = bhw::ola(4, 160, 880, 31);
    o.hop = 0;
    try {
        bhw::overlap_add_len(p, 400, o, nullptr, nullptr);
        return 6;
    } catch (const bhw::error &) {
    }
    bhw::resident_table t;                                  // empty handle: the member calls compile and fail loudly
    try {
        t.generate_len(p, 400, nullptr, 0, 400, nullptr);
        return 7;
    } catch (const bhw::error &) {
    }
    try {
        t.apply_frames_len(p, 400, nullptr, f, nullptr, nullptr);
        return 8;
    } catch (const bhw::error &) {
    }
    try {
        t.overlap_add_len(p, 400, nullptr, bhw::ola(4, 160, 880, 31), nullptr, nullptr);
        return 9;
    } catch (const bhw::error &) {
    }
    if (t.describe_len(p, 400, 0, 400).rfind("any-length route", 0) != 0) return 10;   // no table: the library call's route
    return 0;
}
''')
    exe = str(tmp_path / "len")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L" + PKG, "-lbhw", "-Wl,-rpath," + PKG], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "-1", (r.returncode, r.stdout, r.stderr)


def test_python_surface_is_exported():
    import inspect

    import blackman_harris_win_amd as bhw
    assert callable(bhw.window) and "window" in bhw.__all__ and "describe_len" in bhw.__all__
    for fn in (bhw.generate, bhw.apply_frames, bhw.overlap_add, bhw.ResidentTable.generate, bhw.ResidentTable.apply_frames,
               bhw.ResidentTable.overlap_add):
        assert inspect.signature(fn).parameters["length"].default is None, fn
    sig = inspect.signature(bhw.window).parameters
    assert list(sig)[:2] == ["params", "length"] and sig["sym"].default is False
    with pytest.raises(ValueError):
        bhw.window(B.make_params(B.WIN_HANN, 10, 16), 1, sym=True)
