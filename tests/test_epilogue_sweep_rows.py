"""The geometry, coverage, filter bank and bounds of tests/epilogue_sweep_rows.py without a GPU.

Geometry and coverage at every size of the four lists: the frame counts, the window's column, the regimes of the accumulating
epilogue read from the describe line of the Welch sibling (as the class tables parse it), `fy` dividing 16 or a multiple of it, the
sizes with bin M aside.  The filter bank's band edges.  The default-length signals of the older sweeps unchanged, by a hash taken at
the commit before the generators took a length.

And the proof that the derived bounds need no tuning: the float32 CPU library of tests/test_fft_sweep_rows.py (scipy.fft where SciPy
imports, else numpy.fft) stands in for the kernel, a NumPy Blackman window rounded to float32 for v; its spectrum is pushed through
the power, the bank, the frame average and the hold traces in NumPy as the contracts state them, and every front at every size and
row type must stay inside its bound.  The worst ratio to the bound is printed per family and front."""
import hashlib

import numpy as np
import pytest

import epilogue_sweep_rows as E
import fft_sweep_rows as R
import iq_mixed_sweep_rows as Q
from test_fft_sweep_rows import _fft, LIBRARY, _window

FAMS = list(E.FAMILIES)


def test_the_four_lists_are_whole():
    assert [len(E.FAMILIES[f]) for f in FAMS] == [95, 91, 9, 8] and FAMS == ["mixed", "iq_mixed", "real", "iq"]
    assert E.FAMILIES["mixed"] is R.SIZES and E.FAMILIES["iq_mixed"] is Q.SIZES
    assert E.FAMILIES["real"] is R.POW2_REAL and E.FAMILIES["iq"] is R.POW2_IQ


def test_the_default_length_signals_are_unchanged():
    h = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()     # noqa: E731
    assert R.forward_signals(400).shape == (6, 1607) and R.forward_signals(400, 1607).shape == (6, 1607)
    assert h(R.forward_signals(400)) == "39be2786efd4fbdda6c8e940cc7b26448809cc20cf1d2a97b5f1f74aeaae2e14"
    assert h(R.forward_signals_iq(400)) == "032edf2b03a767961b7915d22d7b05145453977f8ab081878a155b90019f88a0"
    assert h(Q.forward_signals_iq(400)) == "032edf2b03a767961b7915d22d7b05145453977f8ab081878a155b90019f88a0"
    assert h(Q.forward_signals_iq(75)) == "a68102b31cfa8f79cc8e1efaecd8bc4219a4a87664a0c835624ca9cbb84dbe3b"
    for gen, n in ((R.forward_signals, 400), (R.forward_signals_iq, 400), (Q.forward_signals_iq, 75)):
        assert h(gen(n, 4 * n + 7)) == h(gen(n)) and gen(n, 999).shape[1] == 999


@pytest.mark.parametrize("fam", FAMS)
def test_geometry_and_frame_counts_at_every_size(fam):
    setups = set()
    for i, n in enumerate(E.FAMILIES[fam]):
        c = E.case(fam, n)
        x = E.signals(fam, n)
        assert x.shape == (7 if E.IQ[fam] else 6, c["T"]) and x.dtype == (np.complex64 if E.IQ[fam] else np.float32)
        assert c["hop"] == n // 4 + 1 and c["setup"] == R.setup_for(i, c["L"]) and c["col0"] == 0
        if i % 2 == 0:
            assert (c["L"], c["mode"], c["detrend"], c["frames"], c["pad"]) == (n, "reflect", False, 35, n // 2)
            assert 1 + (c["T"] + 2 * c["pad"] - n) // c["hop"] == 35 and 1 + (c["T"] - 1 + 2 * c["pad"] - n) // c["hop"] == 34
        else:
            assert (c["L"], c["mode"], c["detrend"], c["frames"], c["pad"]) == (n - 3, None, True, 19, 0)
            assert c["T"] == 18 * c["hop"] + n - 3 and 1 + (c["T"] - c["L"]) // c["hop"] == 19
        # the library's own count of the frames, its column of the window and its chunks, from the Welch sibling's descriptor
        s, L, frames, det = E.WELCH_CASES[fam].desc(c)
        assert (L, frames, det, s.col0, s.pad) == (c["L"], c["frames"], c["detrend"], c["col0"], c["pad"])
        d = E.plan(fam, n)
        assert d["frames"] == c["frames"] and d["signals"] == c["B"] and d["chunk"] == E.CHUNK and d["blocks"] == 1
        assert d["chunks"] == -(-c["frames"] // E.CHUNK) == (3 if i % 2 == 0 else 2)
        r = E.rows(x, _window(c["L"]), c)
        assert r.shape == (c["B"], c["frames"], n) and r.dtype == x.dtype and not r[:, :, c["L"]:].any()
        setups.add(c["setup"])
    assert len(setups) >= (5 if len(E.FAMILIES[fam]) > 9 else 4)


@pytest.mark.parametrize("fam", FAMS)
def test_both_regimes_occur_and_fy_divides_16_or_is_a_multiple_of_it_at_every_size(fam):
    regimes, ragged = set(), set()
    for i, n in enumerate(E.FAMILIES[fam]):
        d = E.plan(fam, n)
        fy, F = d["fy"], d["frames"]
        assert fy >= 1 and (E.CHUNK % fy == 0 or fy % E.CHUNK == 0), (fam, n, fy)
        assert fy * d["lpf"] == E.LANES, (fam, n)
        if fy >= E.CHUNK:
            assert (d["gpr"], d["acc"], d["run"]) == (1, 0, fy), (fam, n)
            regimes.add("chunks")
        else:
            assert (d["gpr"], d["run"]) == (E.CHUNK // fy, E.CHUNK) and d["acc"] >= 1, (fam, n)
            regimes.add("carried")
        assert d["runs"] == d["signals"] * -(-F // d["run"]), (fam, n)
        if i % 2 == 0:                                                 # F = 35
            if fy == 2 * E.CHUNK:
                ragged.add("fy 32: a live chunk of 3 beside a chunk of padding")
                assert d["runs"] == 2 * d["signals"] and F - fy == 3
            if fy < E.CHUNK:
                assert d["runs"] == 3 * d["signals"]
            if fy == 2:
                ragged.add("fy 2: groups with 2, 1 and 0 live slots")
                assert [max(0, min(2, 3 - 2 * g)) for g in range(3)] == [2, 1, 0]
    assert regimes == {"chunks", "carried"}, (fam, regimes)
    if fam in ("mixed", "iq_mixed"):
        assert len(ragged) == 2, ragged


def test_every_size_with_bin_M_aside_is_present():
    aside = [n for n in E.FAMILIES["mixed"] if (n // 2) % E.LANES == 0]
    assert aside == list(E.ASIDE) == [1536, 2560, 3072]
    assert [n for n in E.FAMILIES["real"] if n // 2 >= E.LANES] == [512, 1024, 2048, 4096]
    for fam, sizes in (("mixed", aside), ("real", [512, 1024, 2048, 4096])):
        for n in sizes:
            d = E.plan(fam, n)
            assert d["m"] == n // 2 and d["m"] % E.LANES == 0 and d["fy"] < E.CHUNK, (fam, n)
            assert d["acc"] == d["m"] // E.LANES + 1, (fam, n)         # M / 256 bins on every lane and bin M on one more
    # the three mixed-radix aside sizes stand at odd positions (19 detrended frames); the power-of-two ones meet both geometries
    assert {E.case("mixed", n)["frames"] for n in aside} == {19}
    assert {E.case("real", n)["frames"] for n in (512, 1024, 2048, 4096)} == {35, 19}
    assert E.sentinel_sizes("mixed") == [18, 1536, 2560, 3072, 4050] and E.sentinel_sizes("iq_mixed") == [18, 2025]
    assert E.sentinel_sizes("real") == [16, 4096] and E.sentinel_sizes("iq") == [16, 2048]


@pytest.mark.parametrize("fam", ["mixed", "real"])
def test_the_banks_band_edges(fam):
    from blackman_harris_win_amd.selector import fbank_bands, fbank_dense
    for n in E.FAMILIES[fam]:
        M = n // 2
        K = M + 1
        W = E.bank(n)
        assert W.shape == (K, 6) and W.dtype == np.float64 and np.array_equal(W, W.astype(np.float32).astype(np.float64))
        assert (W >= 0).all() and W.max() == 1.0
        first, offset, weight = fbank_bands(W)
        edges = [(int(first[m]), int(first[m]) + int(offset[m + 1] - offset[m]) - 1) for m in range(6)]
        assert edges == E.bank_edges(n), (n, edges)
        assert (weight > 0).all(), "no zero inside a band"
        assert np.array_equal(fbank_dense(first, offset, weight, K), W.astype(np.float32))
        q = max(2, K // 4)
        assert edges[:5] == [(0, 0), (M, M), (0, q), (M - q, M), (0, M)]
        assert W[M, 3] == 1.0 and W[0, 0] == 1.0 and W[M, 1] == 0.5 and (W[:, 4] == 1.0).all()
        assert int(np.argmax(W[:, 2])) in (q // 2, (q + 1) // 2) and (np.diff(W[M - q:, 3]) > 0).all()
        lo, hi = edges[5]
        if K > E.LANES:
            assert lo <= 255 and hi >= 256 and hi <= M, n                # the band straddles the lanes' first and second bins
        else:
            assert lo <= K // 2 <= hi and 0 <= lo and hi <= M, n


# ---- the float32 stand-in through every epilogue --------------------------------------------------------------------------------------------

def _stand_in(fam, n):
    """{front: [ratio to its bound per signal]} of the float32 CPU library at size n."""
    c = E.case(fam, n)
    x = E.signals(fam, n)
    r = E.rows(x, _window(c["L"]), c)
    Y = _fft.fft(r, axis=-1) if E.IQ[fam] else _fft.rfft(r, axis=-1)
    assert Y.dtype == np.complex64, "the library keeps single precision"
    Y64 = E.spectrum64(r)
    g = [R.row_error(Y[b], Y64[b]) / E.gate(n, b) for b in range(c["B"])]
    P64 = E.power64(Y64)
    q = Y.real.astype(np.float64) ** 2 + Y.imag.astype(np.float64) ** 2
    P = q.astype(np.float32)
    out = {"stored spectrum / gate": g, "power": E.power_ratios(fam, n, P, P64)}
    for doubled in ((True, False) if not E.IQ[fam] else (False,)):
        s = E.sk(fam, n, E.WELCH_SCALE_C / c["frames"], doubled)
        w = (q.sum(axis=1) * s).astype(np.float32)
        out[f"welch{' doubled' if doubled else ''}"] = E.welch_ratios(fam, n, w, P64, s)
    s = E.sk(fam, n, E.HOLD_SCALE, True)
    out["hold max"] = E.hold_ratios(fam, n, (P.max(axis=1).astype(np.float64) * s).astype(np.float32), P64, s, "max")
    out["hold min"] = E.hold_ratios(fam, n, (P.min(axis=1).astype(np.float64) * s).astype(np.float32), P64, s, "min")
    if not E.IQ[fam]:
        W = E.bank(n)
        out["bank"] = E.bank_ratios(fam, n, (P.astype(np.float64) @ W).astype(np.float32), P64, W)
    return out


@pytest.mark.parametrize("fam", FAMS)
def test_the_float32_library_is_inside_every_derived_bound_at_every_size_and_row_type(fam):
    names = E.row_types(fam)
    worst = {}
    for n in E.FAMILIES[fam]:
        for front, ratios in _stand_in(fam, n).items():
            assert len(ratios) == len(names)
            for b, r in enumerate(ratios):
                if r > worst.get(front, (0.0, 0, 0))[0]:
                    worst[front] = (r, n, b)
    for front, (r, n, b) in worst.items():
        print(f"{LIBRARY} {fam}, {front}: worst ratio to the bound {r:.3f} at n_fft {n}, {names[b]}")
    for front, (r, n, b) in worst.items():
        assert r <= 1.0, (fam, front, n, names[b], r)


def test_a_dropped_chunk_a_stored_padding_chunk_and_a_missing_bin_fail_the_bounds():
    """What the float64 gates are there for, on the references themselves at two sizes: the last ragged chunk dropped from the frame
    sum, a frame of zeros taken into the minimum, bin M left out of the flat band."""
    for fam, n in (("mixed", 2560), ("iq_mixed", 75)):
        c = E.case(fam, n)
        x = E.signals(fam, n)
        P64 = E.power64(E.spectrum64(E.rows(x, _window(c["L"]), c)))
        s = E.sk(fam, n, E.WELCH_SCALE_C / c["frames"], False)
        whole = c["frames"] // E.CHUNK * E.CHUNK
        assert min(E.welch_ratios(fam, n, P64[:, :whole].sum(axis=1) * s, P64, s)) > 100.0
        assert max(E.welch_ratios(fam, n, E.welch64(P64, s), P64, s)) < 1e-6
        dead = np.concatenate([P64, np.zeros_like(P64[:, :1])], axis=1)
        assert E.hold_ratios(fam, n, dead.min(axis=1) * s, P64, s, "min")[0] > 100.0          # the noise row: no bin is ever near zero
        if not E.IQ[fam]:
            W = E.bank(n)
            short = W.copy()
            short[-1, 4] = 0.0
            assert max(E.bank_ratios(fam, n, P64 @ short, P64, W)) > 100.0
