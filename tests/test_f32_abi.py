"""Float32 frame apply and overlap-add (bhw_*_f32_* / bhw_describe_f32): the checks that need no GPU -- exports and declarations,
every argument error before any HIP call, the describe lines, the C++ wrappers and the Python surface."""
import ctypes
import inspect
import os
import re
import subprocess

from blackman_harris_win_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "blackman_harris_win_amd")
BADARG, UNSUPPORTED = -1, -2

NEW_SYMBOLS = ("bhw_apply_frames_f32_device", "bhw_apply_frames_f32_from_table", "bhw_overlap_add_f32_device",
               "bhw_overlap_add_f32_from_table", "bhw_describe_f32")
A, Z = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x80000000)     # never dereferenced: every call below fails or has nothing to do


def _err():
    return B.lib().bhw_last_error().decode()


def _desc(p, length, f=None, o=None, flags=0):
    buf = ctypes.create_string_buffer(512)
    rc = B.lib().bhw_describe_f32(None, ctypes.byref(p), int(length), ctypes.byref(f) if f is not None else None,
                                  ctypes.byref(o) if o is not None else None, flags, buf, 512)
    return rc, buf.value.decode()


def _calls(f, o, flags=0):
    L = B.lib()
    return (
        lambda q, n: L.bhw_apply_frames_f32_device(q, n, 0, None, f, A, Z),
        lambda q, n: L.bhw_apply_frames_f32_from_table(None, q, n, None, f, A, Z),
        lambda q, n: L.bhw_overlap_add_f32_device(q, n, 0, None, o, flags, A, Z),
        lambda q, n: L.bhw_overlap_add_f32_from_table(None, q, n, None, o, flags, A, Z),
    )


def test_new_symbols_are_exported_declared_and_listed():
    L = B.lib()
    with open(os.path.join(ROOT, "include", "bhw.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert re.search(r"#define BHW_OLA_NORMALIZE 1u", header) and B.OLA_NORMALIZE == 1
    assert L.bhw_abi_version() == 4


def test_length_flag_and_source_errors_come_before_any_hip_call():
    p = B.make_params(B.WIN_BH7, 12, 32)
    f = ctypes.byref(B.make_frames(4, 100))
    o = ctypes.byref(B.make_ola(4, 100, 700))
    taylor = B.make_params(B.WIN_HANN, 12, 16, sin_type=B.SIN_TAYLOR)
    for call in _calls(f, o):
        assert call(None, 400) == BADARG and "params" in _err()
        assert call(ctypes.byref(p), 0) == BADARG and "length 0" in _err(), _err()
        assert call(ctypes.byref(p), (1 << 12) + 1) == BADARG and "length" in _err()
        assert call(ctypes.byref(taylor), 400) == UNSUPPORTED and "CORDIC" in _err(), _err()
        assert call(ctypes.byref(taylor), 1 << 12) == UNSUPPORTED                     # also at L = 2^phi_width
    for flags in (2, 3, 0x80000000):
        for call in _calls(f, o, flags)[2:]:
            assert call(ctypes.byref(p), 400) == BADARG and "flags" in _err(), _err()
    # from a table: a NULL handle after the length and flag checks
    L = B.lib()
    assert L.bhw_apply_frames_f32_from_table(None, ctypes.byref(p), 400, None, f, A, Z) == BADARG and "table is NULL" in _err()
    assert L.bhw_overlap_add_f32_from_table(None, ctypes.byref(p), 400, None, o, 1, A, Z) == BADARG and "table is NULL" in _err()


def test_descriptor_errors_of_the_int32_counterparts():
    L = B.lib()
    p = B.make_params(B.WIN_BH7, 12, 32)

    def frames(fd, x=A, y=Z, n=400):
        return L.bhw_apply_frames_f32_device(ctypes.byref(p), n, 0, None, ctypes.byref(fd) if fd is not None else None, x, y)

    def ola(od, y=A, x=Z, n=400, flags=0):
        return L.bhw_overlap_add_f32_device(ctypes.byref(p), n, 0, None, ctypes.byref(od) if od is not None else None, flags, y, x)

    assert frames(None) == BADARG
    bad = B.make_frames(4, 100)
    bad.struct_size = 8
    assert frames(bad) == BADARG and "struct_size" in _err()
    bad = B.make_frames(4, 100)
    bad.reserved = 1
    assert frames(bad) == BADARG and "reserved" in _err()
    assert frames(B.make_frames(4, 100, channels=3)) == BADARG and "channels" in _err()
    assert frames(B.make_frames(4, 0)) == BADARG and "hop" in _err()
    assert frames(B.make_frames(4, 100, shift=63)) == BADARG and "shift" in _err()
    assert frames(B.make_frames(4, 100, y_stride=399)) == BADARG and "y_stride" in _err()
    assert _desc(p, 400, f=B.make_frames(4, 100, y_stride=400))[0] == 0                   # L * C itself passes (host-only check)
    assert frames(B.make_frames(4, 100), A, A) == BADARG and "overlap" in _err()
    assert frames(B.make_frames(4, 100), None, Z) == BADARG and "NULL" in _err()
    assert frames(B.make_frames((1 << 34) // 400 + 1, 400)) == BADARG and "2^34" in _err()
    assert frames(B.make_frames(0, 100), None, None) == 0                                  # nothing to do: pointers unchecked
    assert ola(None) == BADARG
    bad = B.make_ola(4, 100, 700)
    bad.reserved = 1
    assert ola(bad) == BADARG and "reserved" in _err()
    assert ola(B.make_ola(4, 0, 700)) == BADARG and "hop" in _err()
    assert ola(B.make_ola(4, 100, 701)) == BADARG and "extent" in _err()                  # extent (4 - 1) * 100 + 400 = 700
    assert ola(B.make_ola(0, 100, 10)) == BADARG and "frames is 0" in _err()
    assert ola(B.make_ola(4, 100, 700, shift=63)) == BADARG and "shift" in _err()
    assert ola(B.make_ola(4, 100, 700), A, A) == BADARG and "overlap" in _err()
    assert ola(B.make_ola(4, 100, 0), None, None, flags=1) == 0                           # count 0: nothing to do
    # the same descriptors pass every check of the host-only describe call (no launch: A and Z are never handed to a kernel)
    assert _desc(p, 400, f=B.make_frames(4, 100))[0] == 0
    assert _desc(p, 400, o=B.make_ola(4, 100, 700), flags=1)[0] == 0


def test_describe_lines():
    p = B.make_params(B.WIN_BH4, 10, 24)
    rc, d = _desc(p, 1 << 10, f=B.make_frames(64, 256))
    assert rc == 0 and d.startswith("f32 frames direct (L = 2^10): k_frames_f32_direct<2>, 1 channel, G = "), d
    rc, d = _desc(p, 400, f=B.make_frames(64, 100, channels=2))
    assert rc == 0 and d.startswith("f32 frames direct (L = 400): k_frames_f32_direct_len<2>, 2 channels"), d
    rc, d = _desc(p, 1 << 10, o=B.make_ola(64, 256, 1000), flags=B.OLA_NORMALIZE)
    assert rc == 0 and d.startswith("f32 overlap-add direct (L = 2^10), normalised by the window envelope: k_ola_f32_direct<2>, 1 channel, Q = "), d
    rc, d = _desc(p, 400, o=B.make_ola(64, 100, 1000))
    assert rc == 0 and d.startswith("f32 overlap-add direct (L = 400), not normalised: k_ola_f32_direct_len<2>"), d
    rc, d = _desc(p, 400, o=B.make_ola(64, 100, 0))
    assert rc == 0 and d.endswith("nothing (count 0)"), d
    # no per-frame route, even where the int32 call takes it (one long window, few frames)
    q = B.make_params(B.WIN_BH7, 22, 32)
    assert B.describe_frames(q, 2, 1 << 22).startswith("per-frame")
    assert _desc(q, 1 << 22, f=B.make_frames(2, 1 << 22))[1].startswith("f32 frames direct"), _desc(q, 1 << 22, f=B.make_frames(2, 1 << 22))
    # exactly one descriptor; no flags on the frames call
    assert _desc(p, 400)[0] == BADARG
    assert _desc(p, 400, f=B.make_frames(4, 100), o=B.make_ola(4, 100, 700))[0] == BADARG
    assert _desc(p, 400, f=B.make_frames(4, 100), flags=1)[0] == BADARG and "frames call" in _err()
    assert _desc(p, 400, o=B.make_ola(4, 100, 700), flags=2)[0] == BADARG and "flags" in _err()
    # the Python helper, and the resident-table kernels named by the table describe hooks' format rule
    assert B.describe_f32(p, 400, frames=B.make_frames(64, 100)) == _desc(p, 400, f=B.make_frames(64, 100))[1]
    assert "normalised by" in B.describe_f32(p, ola=B.make_ola(64, 256, 1000), normalize=True)
    # the forced any-length kernels at L = 2^phi_width
    L = B.lib()
    prev = L.bhw_dbg_len_force_kernels(1)
    try:
        assert "k_frames_f32_direct_len<" in _desc(p, 1 << 10, f=B.make_frames(64, 256))[1]
    finally:
        L.bhw_dbg_len_force_kernels(prev)


def test_cpp_f32_wrappers_compile_and_link(tmp_path):
    src = tmp_path / "f32.cpp"
    src.write_text(r'''
#include <cstdio>
#include "bhw.hpp"
int main()
{
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 10, 24);
    bhw_frames f = bhw::frames(4, 256, 23);
    bhw_ola o = bhw::ola(4, 256, 1792, 23);
    if (bhw::describe_f32(p, 1024, &f, nullptr).rfind("f32 frames direct", 0) != 0) return 2;
    if (bhw::describe_f32(p, 1024, nullptr, &o, BHW_OLA_NORMALIZE).find("normalised by the window envelope") == std::string::npos) return 3;
    try {
        bhw::apply_frames_f32(p, 0, f, nullptr, nullptr);   // length 0: BADARG, before any HIP call
        return 4;
    } catch (const bhw::error &e) {
        std::printf("%d\n", e.code);
    }
    try {
        bhw::overlap_add_f32(p, 1024, o, 2u, nullptr, nullptr);
        return 5;
    } catch (const bhw::error &) {
    }
    bhw::resident_table t;                                  // empty handle: the member calls compile and fail loudly
    try {
        t.apply_frames_f32(p, 1024, nullptr, f, nullptr, nullptr);
        return 6;
    } catch (const bhw::error &) {
    }
    try {
        t.overlap_add_f32(p, 1024, nullptr, o, BHW_OLA_NORMALIZE, nullptr, nullptr);
        return 7;
    } catch (const bhw::error &) {
    }
    if (t.describe_f32(p, 1024, &f, nullptr).rfind("f32 frames direct", 0) != 0) return 8;
    return 0;
}
''')
    exe = str(tmp_path / "f32")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L" + PKG, "-lbhw", "-Wl,-rpath," + PKG], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "-1", (r.returncode, r.stdout, r.stderr)


def test_python_surface():
    import blackman_harris_win_amd as bhw
    assert "describe_f32" in bhw.__all__ and bhw.describe_f32 is B.describe_f32
    for fn in (bhw.overlap_add, bhw.ResidentTable.overlap_add):
        assert inspect.signature(fn).parameters["normalize"].default is False, fn
    sig = inspect.signature(bhw.window).parameters
    assert sig["dtype"].default is None and sig["shift"].default is None
    p = B.make_params(B.WIN_HANN, 10, 16)
    try:
        B.describe_f32(p, 400)
    except ValueError:
        pass
    else:
        raise AssertionError("describe_f32 with neither descriptor must raise")
