"""The case tables of test_gpu_table_source.py (tests/table_source_cases.py), held to their own rules without a GPU: every front meets
every table format, every term-count bound and every combine mode; ids are unique, every window fits its row and every n_fft is one its
family takes; the fronts are the ResidentTable methods; and the window lengths of the nibble + escapes cases reach listed entries of the
table, re-derived here from the host model of the build kernel (tools/sim_build.cpp --escapes) where g++ builds it."""
import inspect
import os
import subprocess
import sys

import numpy as np

import table_source_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_format_is_among_the_tables():
    assert {t[4] for t in C.TABLES.values()} == {0, 1, 2, 3, 5}
    assert all(C.TABLES[t][4] == 5 for t in C.ESC_TABLES)
    for name, (model, pw, w, limit, fmt) in C.TABLES.items():
        assert limit in C.LIMITS and model in C.MODELS and fmt in C.FMT_NAME, name
        assert pw == 22 or name == "nibble26", name
        assert w <= 25 or name == "nibble26", "fl32(w) must be exact where the coefficients reach a float front"
    assert C.TABLES["nibble26"][:3] == ("hls", 26, 32)
    model, pw, w = C.TABLES["zshr"][:3]
    assert model == "cpp" and pw - 1 - w == C.Z_SHR["zshr"] > 0


def test_every_front_meets_every_format_bound_and_mode():
    for f in C.FRONTS:
        mine = [c for c in C.cases() if c["front"] == f["name"]]
        assert {c["triple"][0] for c in mine} == {0, 1, 2, 3, 5}, f["name"]
        assert {c["triple"][1] for c in mine} == {3, 5, 7}, f["name"]
        assert {c["triple"][2] for c in mine} == {0, 1, 2}, f["name"]
        assert any(c["table"] == "zshr" for c in mine), f["name"]
        if f["family"] is not None:
            assert any(c["L"] < c["n_fft"] for c in mine) and any(c["L"] == c["n_fft"] for c in mine), f["name"]
            assert {c["n_fft"] for c in mine} == set(C.SIZES[f["family"]]), f["name"]
        # a power-of-two L gathers only the first entry of every block and cell: no packed table meets one below the whole period
        assert all(c["L"] & (c["L"] - 1) or c["whole"] or c["triple"][0] == 0 for c in mine), f["name"]
    for group in ("forward", "welch", "hold", "csd"):
        for fam in {f["fused"] for f in C.FRONTS if f["group"] == group}:
            assert any(c["detrend"] for c in C.cases() if C.FRONT[c["front"]]["fused"] == fam), fam
    # the benchmarked shape meets every fused front
    for f in C.FRONTS:
        if f["fused"]:
            assert any(c["table"] == "nibble26" for c in C.cases() if c["front"] == f["name"]), f["name"]


def test_triples_restate_the_weights():
    for c in C.cases():
        p = C.params(c["table"], c["weights"])
        fmt, nt, mode = c["triple"]
        assert fmt == C.TABLES[c["table"]][4]
        assert nt == (3 if p.n_terms <= 3 else 5 if p.n_terms <= 5 else 7)
        assert (mode == 2) == (p.combine == C.B.COMBINE_VHDL) and (mode == 1) == (p.combine == C.B.COMBINE_HLS and p.model == C.B.MODEL_CPP)
    for name, (_, K, _, heavy) in C.WEIGHTS.items():
        if heavy:
            for t in C.ESC_TABLES:
                p, w = C.params(t, name), C.TABLES[t][2]
                assert p.n_terms == K and all(abs(p.aa[k]) >= 1 << (w - 4) for k in range(K)), name
                assert sum(abs(p.aa[k]) for k in range(K)) < 1 << (w - 1), name
    for t in C.ESC_TABLES:
        assert all(C.WEIGHTS[c["weights"]][3] for c in C.cases() if c["table"] == t), "escape cases take the heavy weights"


def test_ids_shapes_and_sizes():
    ids = [c["id"] for c in C.cases()]
    assert len(set(ids)) == len(ids)
    for c in C.cases():
        f = C.FRONT[c["front"]]
        assert 1 <= c["L"] <= c["n_fft"], c["id"]
        assert c["L"] <= 1 << C.TABLES[c["table"]][1], c["id"]
        if f["family"] is not None:
            assert C.SUPPORTED[f["family"]](c["n_fft"]), c["id"]
            assert 10 <= c["frames"] <= 40, c["id"]
        if f["group"] == "inverse":
            assert c["center"], c["id"]
        if c["detrend"]:
            assert not c["center"], c["id"]
    assert C.SUPPORTED["fft"] is C.B.fft_supported and C.SUPPORTED["mfft"] is C.B.mfft_supported
    assert C.SUPPORTED["cfft"] is C.B.cfft_supported and C.SUPPORTED["cmfft"] is C.B.cmfft_supported
    assert set(C.gate_cases()) == set(C.FUSED_FAMILIES) and len(C.FUSED_FAMILIES) == 17


def test_fronts_are_the_table_methods():
    from blackman_harris_win_amd import selector
    for m in C.METHODS:
        assert callable(getattr(selector.ResidentTable, m)), m
    # every ResidentTable method that takes a window and launches a table kernel of its own is among them: the others are the
    # scipy-shaped wrappers (tests/spectral_front_cases.py), generate's power-of-two form, apply and generate_part (integer, by the
    # table tests), and plumbing
    other = {"welch", "welch_fused", "welch_fused_mixed", "welch_fused_iq", "welch_fused_iq_mixed", "hold_fused", "hold_fused_mixed",
             "hold_fused_iq", "hold_fused_iq_mixed", "cross_spectra", "csd", "coherence", "transfer_function", "cross_spectra_fused",
             "csd_fused", "coherence_fused", "transfer_function_fused", "apply", "generate_part", "window", "describe", "describe_frames",
             "describe_overlap_add", "close", "nbytes"}
    public = {n for n, _ in inspect.getmembers(selector.ResidentTable) if not n.startswith("_")}
    assert public == C.METHODS | other, public ^ (C.METHODS | other)


def test_escape_lengths_meet_the_condition_by_the_fixture():
    """Every fused-FFT family has a nibble + escapes case whose window reaches at least two distinct listed entries."""
    esc = C.escapes()
    assert set(esc) == set(C.ESC_TABLES)
    for fam in C.FUSED_FAMILIES:
        mine = [c for c in C.cases() if C.FRONT[c["front"]]["fused"] == fam and c["table"] in C.ESC_TABLES]
        assert mine, fam
        for c in mine:
            row = esc[c["table"]]
            hit = [v for v in row["lengths"].values() if v["L"] == c["L"]]
            assert hit and len(set(hit[0]["reached"])) >= C.MIN_REACHED, (fam, c["id"])
            assert c["L"] <= c["n_fft"]
    for f in C.FRONTS:
        if f["group"] == "framing":
            assert any(c["L"] == C.WHOLE and c["table"] in C.ESC_TABLES for c in C.cases() if c["front"] == f["name"]), f["name"]
    for row in esc.values():
        for v in row["lengths"].values():
            # the fixture's own arithmetic: every entry it names is gathered by that window
            assert set(v["reached"]) <= set(C.gathered_entries(v["L"], row["pw"]).tolist())


def test_fixture_is_what_the_host_model_gives(tmp_path):
    """Builds the host model with g++, as test_build_mirror_host.py does."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import escape_lengths as E
    finally:
        sys.path.pop(0)
    exe = E.compile_sim(tmp_path)
    rows = E.records(exe)
    assert rows == [C.escapes()[t] for t in C.ESC_TABLES]
    for row in rows:
        listed = E.listed_entries(exe, row["model"], row["pw"], row["w"])
        assert len(listed) == row["listed"] and listed == sorted(set(listed))
        assert all(0 <= u < 1 << (row["pw"] - 2) for u in listed)
        for v in row["lengths"].values():
            assert v["reached"] == C.reached(np.asarray(listed), v["L"], row["pw"]) and len(v["reached"]) >= C.MIN_REACHED
        # the option only adds a line: the figures the sweep's parsers read are the ones without it
        args = [exe, str(E.MODEL_ARG[row["model"]]), str(row["pw"]), str(row["w"]), "1"]
        plain = subprocess.run(args, capture_output=True, text=True, timeout=600).stdout
        with_list = subprocess.run(args[:1] + ["--escapes"] + args[1:], capture_output=True, text=True, timeout=600).stdout
        assert with_list.startswith(plain) and with_list[len(plain):].startswith("listed entries:")
