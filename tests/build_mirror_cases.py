"""The configurations and kernel instances of the octant-mirror table build (k_table_build_mirror, csrc/bhw_build.hip), shared by
test_build_mirror_cases.py (no GPU), test_build_mirror_host.py (no GPU) and test_gpu_build_mirror_sweep.py.

A configuration is (model, PW, W, precision).  mirror_rule() restates in Python, independently of the planner, when a whole-period
table call of it builds its table with the mirror kernel; plan_instance() asks the planner (bhw_describe_plan, no GPU).  The
dispatch compiles 72 instances <NITER 21..32, FMT 2 | 3 | 5, THREADS 256 | 1024>.

The probe (probe_params): a two-term window with aa = [0, 2^(W-2)] under the HLS sum is -cos, word for word, so over one whole
period the quadrant map shows both c and s of every first-quadrant table entry, every bit of them -- where the built-in windows
weigh a table word's last bit by 0.43 of an output LSB and less (BH-7's largest harmonic at W = 32).
"""
import json
import os
import re

from blackman_harris_win_amd import binding as B

MODELS = {"hls": B.MODEL_HLS, "cpp": B.MODEL_CPP, "vhdl": B.MODEL_VHDL}
PRECISIONS = {"hls": (1,), "cpp": (1,), "vhdl": (1, 2, 7)}
LIMITS = (("nibble", B.TABLE_NIBBLE, 3), ("nibble+esc", B.TABLE_NIBBLE_ESC, 5), ("residual", B.TABLE_RESIDUAL, 2))   # name, limit, FMT
PW_TESTED = range(22, 27)
WIDTHS = range(8, 33)
ESC_FILL = 96            # kEscFill (csrc/bhw_plan.h): entries one workgroup's escape list may hold


def mirror_rule(model, pw, w, precision):
    """None, or (n_iter, threads, cell log) of the mirror kernel for this configuration: z_shr == 0, at least 21 rotations, the
    CORDIC state within 34 bits and a residual cell of at least 2^7 entries (restated from SURVEY App. A.2-A.4 and the half-LSB
    rule of the residual format, not read from the planner)."""
    vhdl = model == "vhdl"
    if pw < 22 or pw > w:                          # 2^20 table entries and more; z_shr == 0 (vhdl: up to PW == W)
        return None
    n_iter = w - 1 if vhdl else w
    out_shr = precision if vhdl else 2
    d = min(9, (2 * pw - w - 2) // 2)
    if n_iter < 21 or w + out_shr > 34 or d < 7:
        return None
    return n_iter, 1024 if pw >= 26 else 256, d


def bh7_params(model, pw, w, precision):
    return B.make_params(B.WIN_BH7, pw, w, model=MODELS[model], precision=precision)


def probe_params(model, pw, w, precision):
    return B.make_params(1, pw, w, model=MODELS[model], precision=precision, combine=B.COMBINE_HLS, aa=[0, 1 << (w - 2), 0, 0, 0, 0, 0],
                         n_terms=2)


def forget_verdicts(p):
    from test_gpu_build_loop import _forget_verdicts
    _forget_verdicts(p)


def plan_instance(p, limit):
    """(n_iter, FMT, threads) of the mirror kernel a whole-period table call of p under `limit` names with every verdict of the
    configuration forgotten, or None when it names another build kernel."""
    try:
        forget_verdicts(p)
        plan = B.describe_plan(p, 0, 1 << p.phi_width, algo=B.ALGO_TABLE, table_format=limit)
    except B.BhwError:
        return None
    m = re.search(r"k_table_build_mirror<(\d+),(\d+),(\d+)>", plan)
    return tuple(int(v) for v in m.groups()) if m else None


def grid(pws=PW_TESTED, precisions=PRECISIONS):
    for model in sorted(MODELS):
        for precision in precisions[model]:
            for pw in pws:
                for w in WIDTHS:
                    yield model, pw, w, precision


def configurations(pws=PW_TESTED, precisions=PRECISIONS):
    """The mirror configurations by the restated rule, in a fixed order."""
    return [c for c in grid(pws, precisions) if mirror_rule(*c)]


def case_id(c):
    return "%s-%d-%d-p%d" % c


ALL_INSTANCES = {(n, f, t) for n in range(21, 33) for f in (2, 3, 5) for t in (256, 1024)}
DEAD_INSTANCES = {(n, f, 1024) for n in range(21, 25) for f in (2, 3, 5)}


# ---- the host model's figures per configuration (tools/sim_build.cpp), recorded by tests/test_build_mirror_host.py ----
HOST_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "build_mirror_host.json")


def host_rows():
    """{configuration: row}: nibble_misses = entries of the table outside the four-bit fields of the plain nibble format,
    esc_wg_max = the longest escape list of one build workgroup under nibble + escapes."""
    with open(HOST_JSON) as f:
        return {(r["model"], r["pw"], r["w"], r["precision"]): r for r in json.load(f)}


def predicted_format(row, limit_name):
    """The format a call under the limit settles on as far as the host figures decide it: plain nibbles if and only if no entry
    misses the fields, nibble + escapes if and only if some do (or the limit starts there) and no workgroup's list overflows
    kEscFill; None = a wider one (residual and beyond: the host model does not restate those)."""
    if limit_name == "nibble" and row["nibble_misses"] == 0:
        return "nibble"
    if limit_name in ("nibble", "nibble+esc") and row["esc_wg_max"] <= ESC_FILL:
        return "nibble+esc"
    return None
