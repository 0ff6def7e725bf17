"""The case table of tests/spectrogram_cases.py reaches every class of the fused spectrogram: every class has a case, every claim
holds on the describe line and the dense bank of its case (host arithmetic, no GPU), the power cases are the forward kernel's table
unedited, and the plan fields of the describe line are those of describe_stft_fft for the same call."""
import numpy as np
import pytest

import blackman_harris_win_amd as bhw

import spectrogram_cases as SC
import stft_fft_cases as FC

CLAIMS = [(c["id"], name) for c in SC.CASES for name in c["classes"]]


@pytest.mark.parametrize("name", list(SC.CLASSES))
def test_every_class_has_a_case(name):
    claimed = [c for c in SC.CASES if name in c["classes"]]
    assert claimed, f"no case claims the class {name!r}"
    for c in claimed:
        line = SC.line(c)
        assert SC.CLASSES[name](c, SC.parse(line), SC.bank(c)), f"case {c['id']} is not of the class {name!r}: {line}"


@pytest.mark.parametrize("cid,name", CLAIMS, ids=[f"{c}: {n}" for c, n in CLAIMS])
def test_every_claim_names_a_class_and_holds(cid, name):
    assert name in SC.CLASSES, f"case {cid} claims {name!r}, which is no class"
    c = SC.case(cid)
    line = SC.line(c)
    assert SC.CLASSES[name](c, SC.parse(line), SC.bank(c)), f"case {cid} is not of the class {name!r}: {line}"


def test_the_power_cases_are_the_forward_table():
    ids = SC.case_ids()
    assert len(set(ids)) == len(ids), ids
    assert [c["id"] for c in SC.POWER_CASES] == ["power-" + i for i in FC.case_ids()]
    for c, f in zip(SC.POWER_CASES, FC.CASES):
        assert {k: v for k, v in c.items() if k not in ("id", "classes", "bank")} == {k: v for k, v in f.items() if k not in ("id", "classes")}
        assert c["bank"] is None
    assert all(c["classes"] and c["bank"] is not None for c in SC.BANK_CASES)


@pytest.mark.parametrize("cid", SC.case_ids())
def test_the_plan_fields_are_the_forward_calls(cid):
    c = SC.case(cid)
    d, f = SC.parse(SC.line(c)), FC.parse(SC.forward_line(c))
    for name in SC.PLAN_FIELDS:
        assert d[name] == f[name] and d[name] is not None, (name, d["line"], f["line"])
    assert d["kernels"] == {k.replace("k_stft_fft", "k_spectrogram"): a for k, a in f["kernels"].items()}, (d["line"], f["line"])
    w = SC.bank(c)
    if w is None:
        assert d["mode"] == "power" and d["W"] == c["n_fft"] // 2 + 1 and "filters" not in d
    else:
        assert d["mode"] == "bank" and d["W"] == d["filters"] == w.shape[1] and d["fpl"] == -(-d["filters"] // d["lpf"])
        assert d["weights"] == int(bhw.selector.fbank_bands(w)[1][-1])


def test_mel_256_80_has_two_empty_filters_by_a_float64_restatement():
    """The class 'an empty filter' on the mel case: with HTK spacing at n_fft 256 and 16 kHz the lowest mel points fall between two
    bins, so two triangles hold no bin.  Restated here in float64 from the formula, independently of mel_weights."""
    K, n_mels = 129, 80
    freqs = np.arange(K, dtype=np.float64) * (8000.0 / (K - 1))
    mel = np.linspace(0.0, 2595.0 * np.log10(1.0 + 8000.0 / 700.0), n_mels + 2)
    pts = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    empty = [m for m in range(n_mels) if not ((freqs > pts[m]) & (freqs < pts[m + 2])).any()]
    assert len(empty) == 2
    w = SC.bank(SC.case("bank-n256-mel80"))
    first, offset, _ = bhw.selector.fbank_bands(w)
    assert [m for m in range(n_mels) if offset[m + 1] == offset[m]] == empty
