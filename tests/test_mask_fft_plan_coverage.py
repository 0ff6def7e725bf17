"""The case table of tests/mask_fft_cases.py reaches every plan class of the fused STFT + mask + inverse STFT front: every class has a
case, every claim holds on the describe line of its case (host arithmetic, no GPU), a sweep of the planner over every supported n_fft
emits no (schedule, spans per workgroup, columns per lane) shape the table lacks, and every plan field of the line is
describe_istft_fft's for the same synthesis descriptor but for the LDS bytes, which hold a second twiddle table."""
import pytest

from blackman_harris_win_amd import binding as B

import istft_fft_cases as IC
import mask_fft_cases as MC

CLAIMS = [(c["id"], name) for c in MC.CASES for name in c["classes"]]
PLAN_FIELDS = ("signals", "frames", "rows", "n_fft", "m", "lpf", "fy", "cpl", "S", "halo", "spans", "trips", "repeated", "groups", "grid",
               "L", "col0", "pad", "t0", "schedule", "normalize", "heavy")


@pytest.mark.parametrize("name", list(MC.CLASSES))
def test_every_class_has_a_case(name):
    claimed = [c for c in MC.CASES if name in c["classes"]]
    assert claimed, f"no case claims the class {name!r}"
    for c in claimed:
        line = MC.line(c)
        assert MC.CLASSES[name](c, MC.parse(line)), f"case {c['id']} is not of the class {name!r}: {line}"


@pytest.mark.parametrize("cid,name", CLAIMS, ids=[f"{c}: {n}" for c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(cid, name):
    assert name in MC.CLASSES, f"case {cid} claims {name!r}, which is no class"
    c = MC.case(cid)
    line = MC.line(c)
    assert MC.CLASSES[name](c, MC.parse(line)), f"case {cid} is not of the class {name!r}: {line}"


def test_the_cases_are_the_inverse_cases_with_every_padding_mode_and_gain_layout():
    assert MC.case_ids() == [c["id"] for c in IC.CASES if c["id"] != "n4096"]
    assert {c["pad_mode"] for c in MC.CASES} == {"reflect", "constant"}
    assert any(not c["center"] for c in MC.CASES)
    assert {c["gains"] for c in MC.CASES} == set(MC.LAYOUTS)
    assert any(c["gains"] == "padded" and c.get("padded") for c in MC.CASES)
    ids = MC.case_ids()
    assert len(set(ids)) == len(ids)
    for c in MC.CASES:
        assert c["classes"], c["id"]
        L, col0, pad, Tin, _ = MC.geometry(c)
        d = MC.parse(MC.line(c))
        assert (d["signals"], d["frames"], d["n_fft"], d["L"], d["col0"], d["pad"]) == (c["B"], c["F"], c["n_fft"], L, col0, pad), d["line"]
        assert (d["T_in"], d["pad_in"], d["pad_mode"]) == (Tin, pad, c["pad_mode"]), d["line"]
        assert d["normalize"] == c["normalize"] and not d["table"] and list(d["kernels"]) == ["k_mask_fft_direct"] and d["both_ffts"], d["line"]
        # the analysis input gives exactly the case's frames
        assert 1 + (Tin + 2 * pad - c["n_fft"]) // c["hop"] == c["F"]


def _lds(d):
    return 2 * d["fy"] * d["m"] * 8 + 2 * d["m"] * 8 + d["n_fft"] * 4


@pytest.mark.parametrize("cid", MC.case_ids())
def test_every_plan_field_is_the_inverse_calls(cid):
    c = MC.case(cid)
    sa, ss, L, _, _, gs, gbs = MC.desc(c)
    p = MC.params(c["setup"])
    d = MC.parse(MC.line(c))
    parent = IC.parse(B.describe_istft_fft(p, L, ss, normalize=c["normalize"]))
    for name in PLAN_FIELDS:
        assert d[name] == parent[name], (cid, name, d["line"], parent["line"])
    assert d["lds"] == _lds(d) == parent["lds"] + d["m"] * 8 and d["lds"] <= 65536


def _shape(d):
    return (d["n_fft"], d["schedule"], d["lpf"], d["fy"], d["cpl"], d["lds"])


def _sweep():
    for lg in range(4, 12):
        n = 1 << lg
        for L in (1, 13, n // 2 + 1, n):
            for hop in (1, 7, n // 4, n // 4 + 3, n + 5):
                for nb in (1, 3, 64):
                    for F in (1, 2, 65, 2049, 40000):
                        if nb * F * n > 1 << 34:
                            continue
                        yield n, L, hop, nb, F


def test_the_planner_emits_no_shape_without_a_case():
    """For every n_fft the checks accept, against windows, hops, batches and frame counts at the edges, with zero padding on the analysis
    side (reflection needs pad < T): the shape is one a case has, and every plan field is the inverse call's."""
    p = MC.params(4)
    covered = {_shape(MC.parse(MC.line(c))) for c in MC.CASES}
    seen = set()
    for n, L, hop, nb, F in _sweep():
        pad, col0 = n // 2, (n - L) // 2
        T = n + hop * (F - 1) - 2 * pad
        if T < 1:
            continue
        sa = B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, pad_mode=0, shift=31)
        ss = B.make_stft(nb, T, F, hop, n, col0=col0, pad=pad, shift=31)
        d = MC.parse(B.describe_mask_fft(p, L, sa, ss, normalize=True))
        parent = IC.parse(B.describe_istft_fft(p, L, ss, normalize=True))
        assert _shape(d) in covered, d["line"]
        for name in PLAN_FIELDS:
            assert d[name] == parent[name], (name, d["line"], parent["line"])
        assert d["lds"] == _lds(d) <= 65536
        seen.add(_shape(d))
    assert seen == covered                          # and no case is of a shape the planner would not emit


def test_unsupported_sizes_have_no_plan():
    p = MC.params(4)
    for n in (8, 15, 17, 100, 400, 4096, 8192):
        with pytest.raises(B.BhwError) as e:
            s = B.make_stft(1, 10000, 3, 7, n, pad=n // 2, shift=31)
            B.describe_mask_fft(p, min(n, 8), s, s)
        assert e.value.code == -2, e.value                 # BHW_ERR_UNSUPPORTED
