"""The mirror build kernel's walk over its groups (GPU): k_table_build_mirror runs it in two copies -- with the format check while a
packed format is still unverified, without it afterwards -- and steps its cell records and table indices from group to group
instead of deriving them from the group number.  Whatever it builds, the whole window from the table strategy must equal the whole
window from ALGO_DIRECT (one chain per coefficient: independent code), bit for bit, compared on the device:

  * the three bit-models;
  * PW 22 and 25 (256-thread workgroups; at PW 25 with cells of 2^9 entries a wave's step of 256 entries is NOT whole cells) and
    PW 26 (1 024-thread workgroups);
  * widths 32 and 31 under the best format (nibble, or nibble + escapes) and width 28 under the residual format (two-byte entries in
    the split layout);
  * first with every verdict of the configuration's packed formats forgotten, so that the call settles them by trial builds with
    the check on (the checked copy; whose only product is the verdict, pinned below), then again after prepare() (the unchecked copy).

PW 22 is the smallest window whose table has group 0, the group of the last own entry, the middle entry and a cell-opening image in
separate workgroups; at widths 32 and 31 its table is plain and comes from another kernel (asserted, so that a change there shows).
"""
import ctypes

import pytest

from blackman_harris_win_amd import binding as B

pytestmark = pytest.mark.gpu

MODELS = {"hls": B.MODEL_HLS, "cpp": B.MODEL_CPP, "vhdl": B.MODEL_VHDL}
WIDTHS = [(32, B.TABLE_BEST), (31, B.TABLE_BEST), (28, B.TABLE_RESIDUAL)]

# The format each (model, width) settles on, the same at PW 25 and 26 (and at PW 22 for width 28): the verdicts of the checked trial
# builds (the overflow test of every stored field, and for nibble + escapes the length of the escape lists), recorded from the
# kernel as it was before the walk was split in two.
SETTLED = {
    ("hls", 32): "nibble", ("hls", 31): "nibble",
    ("cpp", 32): "nibble+esc", ("cpp", 31): "nibble+esc",
    ("vhdl", 32): "nibble+esc", ("vhdl", 31): "nibble+esc",
    ("hls", 28): "residual", ("cpp", 28): "residual", ("vhdl", 28): "residual",
}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _forget_verdicts(p):
    """Every packed format of the configuration back to "unknown": the next call settles them again by checked builds."""
    L = B.lib()
    L.bhw_dbg_table_format_info.argtypes = [ctypes.POINTER(B.BhwParams), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.bhw_dbg_table_format_verdict.argtypes = [ctypes.POINTER(B.BhwParams), ctypes.c_uint32, ctypes.c_int]
    d = ctypes.c_uint32(0)
    L.bhw_dbg_table_format_info(ctypes.byref(p), ctypes.byref(d), None)
    for dlog in (16 + d.value, 48 + d.value, d.value, 6):           # nibble, nibble + escapes, residual, delta16
        if d.value or dlog == 6:
            assert L.bhw_dbg_table_format_verdict(ctypes.byref(p), dlog, 3) == 0


@pytest.mark.parametrize("width,table_format", WIDTHS, ids=["w32", "w31", "w28-residual"])
@pytest.mark.parametrize("pw", [22, 25, 26])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_table_window_equals_direct_window(torch, model, pw, width, table_format):
    import blackman_harris_win_amd as bhw
    p = B.make_params(B.WIN_BH7, pw, width, model=MODELS[model])
    n = 1 << pw
    _forget_verdicts(p)
    plan = B.describe_plan(p, 0, n, algo=B.ALGO_TABLE, table_format=table_format)
    if pw == 22 and width > 28:
        assert "table[plain]" in plan, plan
    else:
        assert "unverified" in plan and "k_table_build_mirror<" in plan and (",1024>" if pw == 26 else ",256>") in plan, plan
    want = bhw.generate(p, 0, n, algo=B.ALGO_DIRECT)
    got = torch.zeros(n, dtype=torch.int32, device=want.device)
    bhw.generate(p, 0, n, algo=B.ALGO_TABLE, table_format=table_format, out=got)           # settles the formats: checked builds
    assert torch.equal(got, want)
    plan = B.describe_plan(p, 0, n, algo=B.ALGO_TABLE, table_format=table_format)
    assert "unverified" not in plan, plan
    assert plan.startswith("table[%s]" % ("plain" if pw == 22 and width > 28 else SETTLED[(model, width)])), plan
    bhw.prepare(p)
    got.zero_()
    bhw.generate(p, 0, n, algo=B.ALGO_TABLE, table_format=table_format, out=got)           # the settled format: no check
    assert torch.equal(got, want)
