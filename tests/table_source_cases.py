"""The tables, weight sets, fronts and shapes of the suite that runs every float and fused FFT front from a resident table of every
packed format (test_gpu_table_source.py), and the choice of window lengths whose gathers reach listed entries of a nibble + escapes
table.  Pure NumPy and the binding's host functions (no GPU, no torch): test_table_source_cases.py proves the coverage rules from
these tables alone, tools/escape_lengths.py writes the record of the listed entries.

Why: every front that takes a ResidentTable has a kernel k_*_table<FMT, NT, MODE> (FMT 0 plain, 1 delta16, 2 residual, 3 nibble,
5 nibble + escapes; NT 3, 5, 7 the bound of the term count; MODE 0 the HLS sum, 1 the HLS sum with the cpp quadrant map, 2 the VHDL
sum).  The packed formats are taken by tiled tables only (phi_width 22 and up, at 22 for widths up to 28), and the case tables of the
float and fused fronts stop at phi_width 16, so they only ever ran FMT 0.

TABLES: (model, PW, W, format limit, the FMT the table must settle on).  PW 22 wherever the format allows (tables of at most 8 MB,
built in microseconds) and W <= 25 wherever the coefficients reach a float front (fl32(w) is then exact: a wrong table LSB cannot
hide in the rounding).  nibble26 is the benchmarked shape (PW 26 / W 32: the 1024-thread build); zshr drops phase bits (cpp 22 / 16:
z_shr = 5, a plain table of 2^15 entries).  Two escapes tables: esc (cpp: MODE 1) and esc_vhdl (MODE 0, and MODE 2 under the VHDL
sum).

WEIGHTS: the weight sets, (win_type, combine) or heavy sets whose every |a_k| >= 2^(W-4), so that a wrong listed entry on any harmonic
moves w (one unit of c is a quarter of a unit of the term at least).  The heavy sets take the HLS sum: the VHDL sum halves every
product and quarters the total, a wrong listed entry then moves w by an eighth of that, and heavy weights under it let the mutation
of esc_fix_wave pass in every front they met (measured); heavy7/vhdl on esc_vhdl runs FMT 5 with MODE 2 all the same.  schedule() gives each front one weight set per table, rotated by the
front's position so that each front sees NT 3, 5, 7 and MODE 0, 1, 2 somewhere.

FRONTS: every ResidentTable method that launches a table kernel, by name, with its kernel, family (which n_fft it takes) and kind
(how the test calls it).  shape() gives the smallest shapes that run the prologue's branches: 2 signals, 10..40 frames, one n_fft per
schedule class (SIZES), win_length < n_fft nearly everywhere, detrend once per forward family (the residual table's case).  No
packed table meets a power-of-two L: such a window gathers only multiples of 2^PW / L, the first entry of every delta16 block and of
every residual or nibble cell, where the stored difference is zero and the predictor's slope is not used (the delta16 mutation passed
every power-of-two family while L was 2048).  L = n_fft is met at the mixed sizes and, at the power-of-two sizes, on the plain table.

Escapes: listed entries are about 1 in 10^4 of a table and a window of L <= 4096 gathers about L distinct angles round(m 2^P / L), so a
case reaches one by luck or not at all.  tools/sim_build.cpp --escapes prints the listed entries of a configuration, choose_lengths()
takes per cap on L the length that reaches the most (ties: the longer), golden/table_source_escapes.json records them, and the
nibble + escapes cases of every fused front use those lengths: "wide" under n_fft 2048 / 2160, "iq_mixed" under 2025 (CAPS).  The fronts
without an n_fft cap also take the whole period L = 2^22, which reaches every listed entry."""
import functools
import json
import os

import numpy as np

from blackman_harris_win_amd import binding as B

MODELS = {"hls": B.MODEL_HLS, "cpp": B.MODEL_CPP, "vhdl": B.MODEL_VHDL}
LIMITS = {"best": B.TABLE_BEST, "plain": B.TABLE_PLAIN, "delta16": B.TABLE_DELTA16, "residual": B.TABLE_RESIDUAL, "nibble": B.TABLE_NIBBLE,
          "nibble+esc": B.TABLE_NIBBLE_ESC}
FMT_NAME = {0: "plain", 1: "delta16", 2: "residual", 3: "nibble", 5: "nibble+esc"}

# name -> (model, PW, W, limit, FMT)
TABLES = {
    "plain": ("hls", 22, 24, "plain", 0),
    "delta16": ("hls", 22, 25, "delta16", 1),
    "residual": ("vhdl", 22, 24, "residual", 2),
    "nibble": ("hls", 22, 25, "nibble", 3),
    "esc": ("cpp", 22, 25, "nibble+esc", 5),
    "nibble26": ("hls", 26, 32, "nibble", 3),
    "zshr": ("cpp", 22, 16, "best", 0),
    "esc_vhdl": ("vhdl", 22, 24, "nibble+esc", 5),
}
ESC_TABLES = ("esc", "esc_vhdl")
Z_SHR = {"zshr": 5}                       # cpp: z_shr = PW - 1 - W

# name -> (win_type, n_terms, combine, heavy)
WEIGHTS = {
    "hann/hls": (B.WIN_HANN, 2, "hls", False), "hann/vhdl": (B.WIN_HANN, 2, "vhdl", False),
    "hamming/hls": (B.WIN_HAMMING, 2, "hls", False),
    "bh4/hls": (B.WIN_BH4, 4, "hls", False), "bh4/vhdl": (B.WIN_BH4, 4, "vhdl", False),
    "bh5/hls": (B.WIN_BH5, 5, "hls", False), "bh5/vhdl": (B.WIN_BH5, 5, "vhdl", False),
    "bh7/hls": (B.WIN_BH7, 7, "hls", False), "bh7/vhdl": (B.WIN_BH7, 7, "vhdl", False),
    "heavy3/hls": (B.WIN_BH3, 3, "hls", True), "heavy5/hls": (B.WIN_BH5, 5, "hls", True), "heavy7/hls": (B.WIN_BH7, 7, "hls", True),
    "heavy7/vhdl": (B.WIN_BH7, 7, "vhdl", True),
}
HEAVY_OFFSETS = (0, 1, 3, 5, 7, 11, 13)   # a_k = 2^(W-4) + offset: the sum of |a_k| stays below 2^(W-1), so w does not wrap
# table -> the weight set of a front at rotation 0, 1, 2
ROTATION = {
    "plain": ("hamming/hls", "bh5/vhdl", "bh7/hls"),
    "delta16": ("bh5/vhdl", "bh7/hls", "hann/vhdl"),
    "residual": ("bh7/hls", "hann/vhdl", "bh4/hls"),
    "nibble": ("bh4/hls", "hann/hls", "bh7/vhdl"),
    "esc": ("heavy7/hls", "heavy5/hls", "heavy3/hls"),
    "nibble26": ("bh4/vhdl", "bh7/hls", "hann/hls"),
    "zshr": ("hann/hls", "bh4/hls", "bh7/vhdl"),
    "esc_vhdl": ("heavy5/hls", "heavy7/vhdl", "heavy3/hls"),
}


def params(table, weights):
    """The bhw_params of weight set `weights` at the configuration of table `table`."""
    model, pw, w, _, _ = TABLES[table]
    win, K, comb, heavy = WEIGHTS[weights]
    combine = B.COMBINE_VHDL if comb == "vhdl" else B.COMBINE_HLS
    if not heavy:
        return B.make_params(win, pw, w, model=MODELS[model], combine=combine)
    aa = [(1 << (w - 4)) + HEAVY_OFFSETS[k] for k in range(K)]
    assert sum(aa) < 1 << (w - 1)
    return B.make_params(win, pw, w, model=MODELS[model], combine=combine, aa=aa, n_terms=K)


def triple(table, weights):
    """(FMT, NT, MODE) of the table kernel for this table and weight set (bhwp_range_form, restated)."""
    model, _, _, _, fmt = TABLES[table]
    _, K, comb, _ = WEIGHTS[weights]
    nt = 3 if K <= 3 else 5 if K <= 5 else 7
    mode = 2 if comb == "vhdl" else 1 if model == "cpp" else 0
    return fmt, nt, mode


# ---- fronts -------------------------------------------------------------------------------------------------------------------------
# family: which n_fft the front takes ("fft" B.fft_supported, "mfft", "cfft", "cmfft", "csd" a power of two up to 2048, None: no cap);
# kind: how test_gpu_table_source.py calls it.  group: the row of the issue's table; fused: the fused-FFT family the escape
# condition and the float64 gates speak of.
def _f(name, kernel, group, kind, family=None, fused=None, **kw):
    return dict(name=name, kernel=kernel, group=group, kind=kind, family=family, fused=fused, kw=kw)


FRONTS = [
    _f("apply_frames_f32", "k_frames_f32_table", "framing", "frames_f32", pow2=True),
    _f("apply_frames_f32_len", "k_frames_f32_table", "framing", "frames_f32", length=True),
    _f("overlap_add_f32", "k_ola_f32_table", "framing", "ola_f32", pow2=True),
    _f("overlap_add_f32_norm", "k_ola_f32_table", "framing", "ola_f32", pow2=True, normalize=True),
    _f("overlap_add_f32_len", "k_ola_f32_table", "framing", "ola_f32", length=True),
    _f("overlap_add_f32_norm_len", "k_ola_f32_table", "framing", "ola_f32", length=True, normalize=True),
    _f("stft_frames", "k_stft_frames_table", "framing", "stft_frames"),
    _f("istft_overlap_add", "k_ola_f32_table", "framing", "istft_ola"),
    _f("welch_frames", "k_welch_frames_table", "framing", "welch_frames"),
    _f("window_sums", "k_window_sums_table", "framing", "window_sums"),
    _f("stft", "k_stft_fft_table", "forward", "forward", "fft", "forward-fft"),
    _f("spectrogram", "k_spectrogram_table", "forward", "forward", "fft", "forward-fft"),
    _f("spectrogram_bank", "k_spectrogram_table", "forward", "forward", "fft", "forward-fft", bank=True),
    _f("stft_mixed", "k_stft_mfft_table", "forward", "forward", "mfft", "forward-mfft"),
    _f("spectrogram_mixed", "k_stft_mfft_table", "forward", "forward", "mfft", "forward-mfft"),
    _f("stft_iq", "k_stft_cfft_table", "forward", "forward", "cfft", "forward-cfft"),
    _f("spectrogram_iq", "k_stft_cfft_table", "forward", "forward", "cfft", "forward-cfft"),
    _f("stft_iq_mixed", "k_stft_cmfft_table", "forward", "forward", "cmfft", "forward-cmfft"),
    _f("spectrogram_iq_mixed", "k_stft_cmfft_table", "forward", "forward", "cmfft", "forward-cmfft"),
    _f("istft", "k_istft_fft_table", "inverse", "inverse", "fft", "inverse-fft"),
    _f("istft_mixed", "k_istft_mfft_table", "inverse", "inverse", "mfft", "inverse-mfft"),
    _f("istft_iq", "k_istft_cfft_table", "inverse", "inverse", "cfft", "inverse-cfft"),
    _f("istft_iq_mixed", "k_istft_cmfft_table", "inverse", "inverse", "cmfft", "inverse-cmfft"),
    _f("welch_fft", "k_welch_fft_table", "welch", "welch", "fft", "welch-fft"),
    _f("welch_fft_mixed", "k_welch_mfft_table", "welch", "welch", "mfft", "welch-mfft"),
    _f("welch_fft_iq", "k_welch_cfft_table", "welch", "welch", "cfft", "welch-cfft"),
    _f("welch_fft_iq_mixed", "k_welch_cmfft_table", "welch", "welch", "cmfft", "welch-cmfft"),
    _f("hold_fft", "k_hold_fft_table", "hold", "hold", "fft", "hold-fft"),
    _f("hold_fft_mixed", "k_hold_mfft_table", "hold", "hold", "mfft", "hold-mfft"),
    _f("hold_fft_iq", "k_hold_cfft_table", "hold", "hold", "cfft", "hold-cfft"),
    _f("hold_fft_iq_mixed", "k_hold_cmfft_table", "hold", "hold", "cmfft", "hold-cmfft"),
    _f("csd_fft", "k_csd_fft_table", "csd", "csd", "csd", "csd-fft"),
    _f("generate_len", "k_range", "integer", "generate_len"),
    _f("apply_frames_len", "k_frames_table", "integer", "frames_len"),
    _f("overlap_add_len", "k_ola_table", "integer", "ola_len"),
]
FRONT = {f["name"]: f for f in FRONTS}
FUSED_FAMILIES = sorted({f["fused"] for f in FRONTS if f["fused"]})
# the ResidentTable methods the fronts above call, for the CPU test to hold against the class
METHODS = {"apply_frames", "overlap_add", "stft_frames", "istft_overlap_add", "welch_frames", "window_sums", "stft", "spectrogram", "stft_mixed",
           "spectrogram_mixed", "stft_iq", "spectrogram_iq", "stft_iq_mixed", "spectrogram_iq_mixed", "istft", "istft_mixed", "istft_iq",
           "istft_iq_mixed", "welch_fft", "welch_fft_mixed", "welch_fft_iq", "welch_fft_iq_mixed", "hold_fft", "hold_fft_mixed", "hold_fft_iq",
           "hold_fft_iq_mixed", "csd_fft", "generate"}

SUPPORTED = {"fft": B.fft_supported, "mfft": B.mfft_supported, "cfft": B.cfft_supported, "cmfft": B.cmfft_supported,
             "csd": lambda n: B.fft_supported(n) and n <= 2048}
SIZES = {"fft": (64, 2048), "mfft": (400, 2160), "cfft": (64, 2048), "cmfft": (400, 2025), "csd": (64, 2048), None: (61, 1000)}
NB = 2
WHOLE = 1 << 22                           # the whole-period window of the PW 22 tables

# ---- escapes ------------------------------------------------------------------------------------------------------------------------
ESCAPES_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_source_escapes.json")
L_MIN, CAPS = 16, {"wide": 2048, "iq_mixed": 2025}     # the longest window under n_fft 2048 / 2160, and under the I/Q mixed 2025
MIN_REACHED = 2


def gathered_entries(L, P):
    """The table entries u = theta mod 2^(P-2) a window of length L gathers at z_shr = 0: theta = round(m 2^P / L) mod 2^P over
    m = 0..L-1 (harmonic k of coefficient n gathers m = k n mod L, and k = 1 alone visits every m)."""
    m = np.arange(L, dtype=np.uint64)
    q = ((m << np.uint64(P + 1)) + np.uint64(L)) // np.uint64(2 * L)
    return np.unique((q % np.uint64(1 << P)) % np.uint64(1 << (P - 2))).astype(np.int64)


def reached(listed, L, P):
    """The listed entries a window of length L reaches, ascending."""
    return sorted(int(u) for u in np.intersect1d(gathered_entries(L, P), np.asarray(listed, dtype=np.int64)))


def choose_lengths(listed, P):
    """{cap name: (L, reached)}: per cap the L in L_MIN..cap that reaches the most listed entries, the longest of equals."""
    listed = np.asarray(sorted(listed), dtype=np.int64)
    counts = {}
    for L in range(L_MIN, max(CAPS.values()) + 1):
        counts[L] = len(np.intersect1d(gathered_entries(L, P), listed, assume_unique=True))
    out = {}
    for name, cap in CAPS.items():
        L = max(range(L_MIN, cap + 1), key=lambda n: (counts[n], n))
        out[name] = (L, reached(listed, L, P))
    return out


def escape_record(table, listed):
    """The fixture row of an escapes table from the host model's list of listed entries."""
    model, pw, w, _, _ = TABLES[table]
    lengths = choose_lengths(listed, pw)
    return {"table": table, "model": model, "pw": pw, "w": w, "precision": 1, "listed": len(listed),
            "lengths": {name: {"L": L, "reached": r} for name, (L, r) in lengths.items()}}


@functools.lru_cache(maxsize=None)
def escapes():
    """{table: row} of golden/table_source_escapes.json."""
    with open(ESCAPES_JSON) as f:
        return {r["table"]: r for r in json.load(f)}


def escape_length(table, family):
    """The window length of the nibble + escapes cases of `table` under the n_fft of `family`."""
    row = escapes()[table]
    return row["lengths"]["iq_mixed" if family == "cmfft" else "wide"]["L"]


# ---- cases --------------------------------------------------------------------------------------------------------------------------

# the weight set of the whole-period cases (L = 2^22: the power-of-two forms, and every framing front on the escapes table), one per
# table so that the CPU model of a whole period is computed once per table
WHOLE_WEIGHTS = {"plain": "hamming/hls", "delta16": "bh7/hls", "residual": "bh4/hls", "nibble": "bh5/vhdl", "esc": "heavy7/hls", "zshr": "bh7/vhdl",
                 "esc_vhdl": "heavy7/hls"}


def schedule(front_index, table):
    return ROTATION[table][front_index % 3]


def shape(front, table, j):
    """n_fft, L, hop, frames, center, detrend of front `front` on table `table` (j: the table's position).  Tables at even positions
    take the small size, the others the large one; escapes tables take the recorded lengths under the large size."""
    small, big = SIZES[front["family"]]
    kind = front["kind"]
    if front["kw"].get("pow2"):
        # the power-of-two entry points take L = 2^PW: two frames of the whole period, half a period apart
        return dict(n_fft=WHOLE, L=WHOLE, hop=WHOLE // 2, frames=2, center=False, detrend=False)
    if front["family"] is None:
        # no transform: n_fft is the row length.  L odd and L a multiple of 8; the power-of-two forms take L = 2^PW at PW 22 only
        L = small if j % 2 == 0 else big
        if table in ESC_TABLES:
            L = escape_length(table, None)
        n, frames = L + (3 if kind in ("stft_frames", "istft_ola", "welch_frames") and j % 2 == 0 else 0), 12
        return dict(n_fft=n, L=L, hop=L // 4 + 1, frames=frames, center=kind in ("stft_frames", "istft_ola"), detrend=False)
    use_big = (j % 2 == 1) or table in ESC_TABLES
    n = big if use_big else small
    pow2 = n & (n - 1) == 0
    L = (n - 5 if pow2 else n) if use_big else (n if pow2 and table == "plain" else n - 3)
    if table in ESC_TABLES:
        L = escape_length(table, front["family"])
    frames, hop = (10, n // 2 + 1) if use_big else (24, n // 4 + 1)
    detrend = table == "residual" and front["group"] in ("forward", "welch", "hold", "csd")
    center = front["group"] == "inverse" or (front["group"] == "forward" and not detrend)
    return dict(n_fft=n, L=L, hop=hop, frames=frames, center=center, detrend=detrend)


@functools.lru_cache(maxsize=None)
def cases():
    """Every case, in a fixed order (built on first use: the shapes of the escapes tables read the fixture)."""
    out = []
    for i, f in enumerate(FRONTS):
        for j, table in enumerate(TABLES):
            pow2 = bool(f["kw"].get("pow2"))
            if pow2 and TABLES[table][1] != 22:
                continue                                   # (a whole period of 2^26 coefficients: the PW 22 nibble table stands for it)
            weights = WHOLE_WEIGHTS[table] if pow2 else schedule(i, table)
            c = dict(id=f"{f['name']}-{table}", front=f["name"], table=table, weights=weights, triple=triple(table, weights), whole=pow2,
                     seed=1000 * i + j)
            c.update(shape(f, table, j))
            out.append(c)
        if f["group"] == "framing":
            # the whole period on the escapes table: every listed entry is gathered
            for table in ESC_TABLES:
                if f["kw"].get("pow2"):
                    continue                               # (its case above is the whole period already)
                weights = WHOLE_WEIGHTS[table]
                out.append(dict(id=f"{f['name']}-{table}-whole", front=f["name"], table=table, weights=weights, triple=triple(table, weights),
                                whole=True, seed=1000 * i + 99, n_fft=WHOLE, L=WHOLE, hop=WHOLE // 2, frames=2, center=False, detrend=False))
    return out



def case(cid):
    return next(c for c in cases() if c["id"] == cid)


def case_ids(table=None):
    return [c["id"] for c in cases() if table in (None, c["table"])]


def window_pairs(table):
    """The distinct (weights, L) of a table's cases: the float window is checked once per pair."""
    return sorted({(c["weights"], c["L"]) for c in cases() if c["table"] == table})


# one packed-table case per fused family whose library-form result meets the family's float64 gate
def gate_cases():
    return {fam: next(c["id"] for c in cases() if FRONT[c["front"]]["fused"] == fam and c["table"] == "nibble") for fam in FUSED_FAMILIES}
