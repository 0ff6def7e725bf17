"""Resident CORDIC tables (bhw_table_create and the *_from_table calls): the checks that need no GPU -- exports, argument errors
before any HIP call, the planner's key match and its description of a from-table call, the C++ RAII wrapper."""
import ctypes
import os
import subprocess

import pytest

from blackman_harris_win_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "blackman_harris_win_amd")

NEW_SYMBOLS = ("bhw_table_create", "bhw_table_destroy", "bhw_table_bytes", "bhw_table_describe", "bhw_generate_from_table",
               "bhw_apply_from_table", "bhw_generate_part_from_table")


def test_new_symbols_are_exported_and_listed():
    L = B.lib()
    for name in NEW_SYMBOLS:
        assert name in B.ABI_SYMBOLS, name
        assert hasattr(L, name), name
    assert L.bhw_abi_version() == 4


def _create(p, table_format=B.TABLE_BEST):
    h = ctypes.c_void_p()
    rc = B.lib().bhw_table_create(ctypes.byref(p) if p is not None else None, 0, None, table_format, ctypes.byref(h))
    return rc, h


def test_argument_errors_come_before_any_hip_call():
    """BADARG / UNSUPPORTED whatever the machine: these never reach the device (the CPU tests run where there is none)."""
    L = B.lib()
    p = B.make_params(B.WIN_BH7, 20, 32)
    assert L.bhw_table_create(ctypes.byref(p), 0, None, 0, None) == B_ERR_BADARG
    assert _create(None)[0] == B_ERR_BADARG
    assert _create(p, table_format=6)[0] == B_ERR_BADARG
    # Taylor (the ROM is cached already), the variant generators
    t = B.make_params(B.WIN_HANN, 16, 16, sin_type=B.SIN_TAYLOR)
    assert _create(t)[0] == B_ERR_UNSUPPORTED
    for model in (B.MODEL_DDS48, B.MODEL_SCALED):
        v = B.make_params(B.WIN_BH4, 16, 16, model=model, validate=False)
        assert _create(v)[0] == B_ERR_UNSUPPORTED
    bad = B.make_params(B.WIN_BH4, 16, 16)
    bad.n_terms = 6
    assert _create(bad)[0] == B_ERR_BADARG
    # NULL handles
    buf = ctypes.create_string_buffer(64)
    out = ctypes.c_void_p(0x1000)
    assert L.bhw_table_destroy(None) == 0
    assert L.bhw_table_bytes(None) == 0
    assert L.bhw_table_describe(None, ctypes.byref(p), 0, 16, buf, 64) == B_ERR_BADARG
    assert L.bhw_generate_from_table(None, ctypes.byref(p), None, 0, 16, out) == B_ERR_BADARG
    assert L.bhw_apply_from_table(None, ctypes.byref(p), None, 0, 16, out, ctypes.c_void_p(0x2000), 0) == B_ERR_BADARG
    assert L.bhw_generate_part_from_table(None, ctypes.byref(p), None, 0, 2, out) == B_ERR_BADARG


B_ERR_BADARG, B_ERR_UNSUPPORTED = -1, -2


def _matches(pt, pc):
    return B.lib().bhw_dbg_table_key_matches(ctypes.byref(pt), ctypes.byref(pc))


@pytest.mark.parametrize("model", [B.MODEL_HLS, B.MODEL_CPP, B.MODEL_VHDL])
def test_key_accepts_the_ports_and_rejects_the_generics(model):
    pt = B.make_params(B.WIN_BH7, 22, 24, model=model, precision=3)
    # the run-time ports: weights, term count, window type, cosine-sum rule
    for win in (B.WIN_HANN, B.WIN_BH4, B.WIN_BH5):
        pc = B.make_params(win, 22, 24, model=model, precision=3, combine=B.COMBINE_VHDL)
        assert _matches(pt, pc) == 0
    pc = B.make_params(B.WIN_BH7, 22, 24, model=model, precision=3, aa=[1, 2, 3, 4, 5, 6, 7])
    assert _matches(pt, pc) == 0
    # the generics
    for field, kw in (("model", dict(model=(model + 1) % 3)), ("phi_width", dict(phi_width=21)), ("dat_width", dict(dat_width=25))):
        args = dict(win_type=B.WIN_BH7, phi_width=22, dat_width=24, model=model, precision=3)
        args.update(kw)
        pc = B.make_params(args.pop("win_type"), args.pop("phi_width"), args.pop("dat_width"), **args)
        assert _matches(pt, pc) == B_ERR_BADARG, field
        assert field in B.lib().bhw_last_error().decode()
    pc = B.make_params(B.WIN_BH7, 22, 24, model=model, precision=5)
    if model == B.MODEL_VHDL:
        assert _matches(pt, pc) == B_ERR_BADARG and "precision" in B.lib().bhw_last_error().decode()
    else:
        assert _matches(pt, pc) == 0                       # PRECISION is a generic of cordic_dds only


def test_key_rejects_a_call_with_the_taylor_source():
    pt = B.make_params(B.WIN_HANN, 16, 16)
    pc = B.make_params(B.WIN_HANN, 16, 16, sin_type=B.SIN_TAYLOR)
    assert _matches(pt, pc) == B_ERR_BADARG and "sin_type" in B.lib().bhw_last_error().decode()


def _describe(pt, pc, n0, count, table_format=B.TABLE_BEST):
    buf = ctypes.create_string_buffer(384)
    rc = B.lib().bhw_dbg_describe_from_table(ctypes.byref(pt), table_format, ctypes.byref(pc), n0, count, buf, 384)
    assert rc == 0, B.lib().bhw_last_error()
    return buf.value.decode()


def test_describe_names_the_kernels_of_a_from_table_call():
    p = B.make_params(B.WIN_BH7, 26, 32)
    whole = _describe(p, p, 0, 1 << 26)
    assert "nibble" in whole and "split" not in whole and "k_tile9<0,3>" in whole and "k_range_combine" not in whole
    assert "17301760 bytes" in whole or "bytes" in whole
    ragged = _describe(p, p, 12345, 1 << 20)
    assert "k_range_combine<3,7,0>" in ragged and "k_tile9" not in ragged
    both = _describe(p, p, 5, 3 << 26)
    assert "k_tile9<0,3>" in both and "k_replicate" in both and "k_range_combine<3,7,0> on the ragged ends" in both
    eighth = _describe(p, p, 1 << 23, 1 << 24)                       # two whole eighths: the tile kernel over an image subset
    assert "image subset" in eighth
    # the forced plain table is split; a natural plain table below 2^22 (fold kernel); the escape format of the cpp model
    assert "k_range_combine<0,7,0>" in _describe(p, p, 3, 1000, table_format=B.TABLE_PLAIN)
    short = B.make_params(B.WIN_BH7, 18, 32)
    s = _describe(short, short, 0, 1 << 18)
    assert "plain, natural" in s and "k_table_combine_fold_t<7,0>" in s
    cpp = B.make_params(B.WIN_BH4, 26, 32, model=B.MODEL_CPP)
    assert "k_range_combine<5,5,1>" in _describe(cpp, cpp, 1, 99, table_format=B.TABLE_NIBBLE_ESC)
    vh = B.make_params(B.WIN_BH5, 24, 16, model=B.MODEL_CPP, combine=B.COMBINE_VHDL)
    assert "k_runlength_window<5,2,true>" in _describe(vh, vh, 0, 1 << 24)


def test_table_bytes_rule_in_the_planner_matches_the_workspace_rule():
    """The table's size for a format is bhwp_table_layout's, the same rule bhw_workspace_bytes_ex applies (16.5 MiB nibble at 2^26)."""
    p = B.make_params(B.WIN_BH7, 26, 32)
    d = _describe(p, p, 0, 1 << 26)
    nbytes = int(d.split(" bytes]")[0].split(", ")[-1])
    assert nbytes <= 17 * 2 ** 20 and nbytes >= 16 * 2 ** 20


def test_cpp_resident_table_compiles_and_links(tmp_path):
    src = tmp_path / "rt.cpp"
    src.write_text(r'''
#include <cstdio>
#include <utility>
#include "bhw.hpp"
int main()
{
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH7, 20, 32);
    bhw::resident_table none;
    bhw::resident_table moved = std::move(none);
    if (moved) return 3;
    p.sin_type = BHW_SIN_TAYLOR_ALL;
    try {
        bhw::resident_table t(p);                     // the Taylor source keeps no table: UNSUPPORTED, before any HIP call
        return 4;
    } catch (const bhw::error &e) {
        std::printf("%d\n", e.code);
    }
    return 0;
}
''')
    exe = str(tmp_path / "rt")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L" + PKG, "-lbhw", "-Wl,-rpath," + PKG], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "-2", (r.returncode, r.stdout, r.stderr)
