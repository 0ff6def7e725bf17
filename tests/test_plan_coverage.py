"""The case table of tests/plan_cases.py reaches every plan branch of the frame, overlap-add and spectra fronts: for every class of every
front at least one case claims it, and every claim holds on the describe line of the case's call (host arithmetic, no GPU).  A class is
covered by the cases that claim it, so removing the only case of a class fails exactly that class.  Where a class is about the table
route the same predicates are held on the from-table describe line (ct != NULL) through the host-only hooks of the int32 calls; the
other fronts' from-table lines need a table handle and are held in tests/test_gpu_plan_coverage.py."""
import ctypes
import itertools

import pytest

from blackman_harris_win_amd import binding as B

import plan_cases as PC

CLASSES = [(front, name) for front, (_, classes, _) in PC.FRONTS.items() for name in classes]
CLAIMS = [(front, c["id"], name) for front, (cases, _, _) in PC.FRONTS.items() for c in cases for name in c["classes"]]


def _line(front, c):
    return PC.FRONTS[front][2](c)


@pytest.mark.parametrize("front,name", CLASSES, ids=[f"{f}: {n}" for f, n in CLASSES])
def test_every_class_has_a_case(front, name):
    cases, classes, _ = PC.FRONTS[front]
    claimed = [c for c in cases if name in c["classes"]]
    assert claimed, f"no case of the {front} table claims the class {name!r}"
    for c in claimed:
        line = _line(front, c)
        assert classes[name](c, PC.parse(line)), f"{front} case {c['id']} is not of the class {name!r}: {line}"


@pytest.mark.parametrize("front,cid,name", CLAIMS, ids=[f"{f}/{c}: {n}" for f, c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(front, cid, name):
    cases, classes, _ = PC.FRONTS[front]
    assert name in classes, f"{front} case {cid} claims {name!r}, which is no class of the front"
    c = PC.case(front, cid)
    line = _line(front, c)
    assert classes[name](c, PC.parse(line)), f"{front} case {cid} is not of the class {name!r}: {line}"


@pytest.mark.parametrize("front", list(PC.FRONTS))
def test_case_ids_are_unique_and_every_case_is_there_for_a_class(front):
    cases = PC.FRONTS[front][0]
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids), ids
    # a case without a class of its own is only legitimate as the other half of a pair (a float32 shape run with and without the division)
    idle = [c["id"] for c in cases if not c["classes"]]
    assert all("norm" in i for i in idle), idle


def test_issue_shapes_take_the_plans_the_issue_names():
    """The shapes the issue was written from, as the planner sees them."""
    d = PC.parse(B.describe_welch(psd=B.make_psd(64, 200, 2049, 4096, 1.0, onesided=True)))
    assert d["kernels"]["k_welch_psd"] == ("0", "8"), d["line"]
    d = PC.parse(B.describe_welch(psd=B.make_psd(40, 1300, 513, 1024, 1.0, onesided=True)))
    assert d["kernels"]["k_welch_psd"] == ("1", "8") and d["blocks"] == 6, d["line"]
    p = PC.params(0)
    for (nb, T, n_fft, hop, C), (rows, fy, G) in (((64, 40000, 64, 16, 2), (160064, 4, 10)), ((300, 2000, 100, 7, 1), (85800, 2, 11)),
                                                  ((40000, 50, 32, 16, 1), (160000, 8, 5)), ((64, 160000, 512, 160, 1), (64064, 1, 32))):
        frames = 1 + T // hop
        d = PC.parse(B.describe_stft(p, n_fft, B.make_stft(nb, T, frames, hop, n_fft, pad=n_fft // 2, pad_mode=B.PAD_REFLECT, channels=C,
                                                           shift=31)))
        assert (d["rows"], d["fy"], d["G"]) == (rows, fy, G), d["line"]


def test_row_block_arithmetic_of_the_cases_beyond_one_grid():
    """Row blocks above kOlaMaxGridY do not show in a describe line (grid y is clamped) and a forced shape shows in none: the classes
    take them from rows / (fy * Q), checked here against the numbers the cases were sized by."""
    cases, _, line = PC.FRONTS["ola"]
    seen = 0
    for c in cases:
        if "rowblocks" not in c["id"] and "force" not in c:
            continue
        d = PC.parse(line(c))
        rows, fy, q, blocks = PC.ola_shape(c, d)
        if "force" in c:
            assert (rows, fy, q, blocks) == (70000, 1, 1, 70000), (c["id"], rows, fy, q, blocks)
        else:
            q_max = PC.Q_MAX_NORM if c["normalize"] else PC.Q_MAX
            assert (rows, fy, q, blocks) == (65535 * q_max + 100, 1, q_max, 65535 + -(-100 // q_max)), (c["id"], rows, fy, q, blocks)
            assert d["grid_y"] == 65535 and d["rx"] == 256 and d["jmax"] == 1, d["line"]
            assert c["frames"] * 256 * 4 <= (1 << 30) + (1 << 20), "y and x of a case stay at about 1 GiB each"
        seen += 1
    assert seen == 3


def test_table_route_lines_of_the_int32_calls_hold_the_same_classes():
    """ct != NULL: the from-table describe hooks of the power-of-two frames and overlap-add calls name the table kernel with the plan of
    the library call."""
    for front, hook, make in (("frames", "bhw_dbg_describe_frames_from_table", PC.frames_desc),
                              ("ola", "bhw_dbg_describe_ola_from_table", PC.ola_desc)):
        cases, classes, line = PC.FRONTS[front]
        seen = 0
        for c in cases:
            if c["kind"] != "pow2":
                continue
            p, desc = PC.params(c["setup"]), make(c)
            buf = ctypes.create_string_buffer(512)
            B.check(getattr(B.lib(), hook)(ctypes.byref(p), B.TABLE_BEST, ctypes.byref(p), ctypes.byref(desc), buf, 512))
            dt, dl = PC.parse(buf.value.decode()), PC.parse(line(c))
            assert dt["table"] and not dl["table"], (dt["line"], dl["line"])
            assert ("k_frames_table" if front == "frames" else "k_ola_table") in dt["kernels"], dt["line"]
            for key in ("G", "Q", "kx", "rx", "qy", "grid_x", "grid_y"):
                assert dt.get(key) == dl.get(key), (key, dt["line"], dl["line"])
            for name in c["classes"]:
                if "direct form" not in name:
                    assert classes[name](c, dt), (c["id"], name, dt["line"])
            seen += 1
        assert seen >= 2


def test_direct_form_0_is_unreachable():
    """No valid bhw_params names a k_*_direct<0> instance (plan_cases' docstring has the arithmetic): every model, rule, width and
    precision that validates takes direct form 1 or 2."""
    forms = set()
    for model, comb, W, prec in itertools.product((B.MODEL_HLS, B.MODEL_CPP, B.MODEL_VHDL), (B.COMBINE_HLS, B.COMBINE_VHDL), range(8, 33),
                                                  range(1, 8)):
        p = B.make_params(B.WIN_BH4, 8, W, model=model, combine=comb, precision=prec, validate=False)
        if B.lib().bhw_params_validate(ctypes.byref(p)) != 0:
            continue
        d = PC.parse(B.describe_len(p, 100, frames=B.make_frames(64, 50)))
        forms.add(d["kernels"]["k_frames_direct_len"])
    assert forms == {("1",), ("2",)}, forms
