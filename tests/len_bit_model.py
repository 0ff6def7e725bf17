"""The bit model of a window of any length, restated in NumPy over the oracle's (and the reference's) CORDIC: the phase map thetas(),
the cosine sum combine() and the window model_window().  Shared by test_gpu_len.py (the integer any-length fronts) and
test_gpu_table_source.py (the float window every table format yields); no GPU and no torch here."""
import numpy as np

from blackman_harris_win_amd import binding as B

import oracle_lib as O


def thetas(L, P, n, K):
    """theta_k(n) for k = 1..K-1 in Python integers: round(((k * (n mod L)) mod L) * 2^P / L) mod 2^P."""
    m = np.asarray(n, dtype=np.uint64) % np.uint64(L)                  # L <= 2^30: every product below stays inside 64 bits
    out = []
    for k in range(1, K):
        mk = (m * np.uint64(k)) % np.uint64(L)
        q = ((mk << np.uint64(P + 1)) + np.uint64(L)) // np.uint64(2 * L)
        out.append((q % np.uint64(1 << P)).astype(np.int64))
    return out


def _wrap(v, bits):
    return ((v + (1 << (bits - 1))) % (1 << bits)) - (1 << (bits - 1))


def combine(p, cos_k):
    """The cosine-sum of the configured rule (HLS: truncating, VHDL: per-product and final rounding) over the cosines of harmonics
    1..K-1, in int64 NumPy."""
    W, K = p.dat_width, p.n_terms
    acc = np.full(cos_k[0].shape, int(p.aa[0]), dtype=np.int64)
    for k in range(1, K):
        m = (int(p.aa[k]) * cos_k[k - 1].astype(np.int64)) >> (W - 2)
        if p.combine == B.COMBINE_VHDL:
            r = _wrap(m, W + 1)
            m = _wrap((r >> 1) + (r & 1), W)
        acc = acc - m if k & 1 else acc + m
    if p.combine == B.COMBINE_VHDL:
        if K == 2:
            S = _wrap(acc, W + 1)
            acc = (S >> 1) + (S & 1)
        else:
            S = _wrap(acc, W + 2)
            acc = (S >> 2) + ((S >> 1) & 1)
    return _wrap(acc, W).astype(np.int32)


_cos_cache = {}


def full_cos(p, source="oracle"):
    """cos over the full circle of 2^phi_width angles: the oracle's model (over host threads from 2^20 angles on), or the reference's
    compiled cordic() (model CPP)."""
    key = (source, p.model, p.phi_width, p.dat_width, p.precision)
    if key not in _cos_cache:
        if source == "oracle":
            sweep = O.sincos_mt if p.phi_width >= 20 else O.sincos
            _cos_cache[key] = sweep(O.from_bhw(p), 0, 1 << p.phi_width)[1]
        else:
            lib = [f for P, W, f in O.ref_pairs() if P == p.phi_width and W == p.dat_width]
            _cos_cache[key] = O.RefCordic(lib[0]).sweep(range(1 << p.phi_width))[1]
    return _cos_cache[key]


SPARSE_ABOVE = 22          # phi_width above which cos_at() runs one chain per distinct angle instead of the full circle


def cos_at(p, angles):
    """The oracle's cos at each array of `angles` (a list of int64 arrays): from the full circle, or for phi_width > SPARSE_ABOVE one
    chain per distinct angle (a window of a few thousand coefficients touches a few thousand of 2^26 angles)."""
    if p.phi_width <= SPARSE_ABOVE:
        c = full_cos(p)
        return [c[t] for t in angles]
    uniq = np.unique(np.concatenate([np.asarray(t).ravel() for t in angles]))
    op = O.from_bhw(p)
    vals = np.array([O.sincos(op, int(t), 1)[1][0] for t in uniq], dtype=np.int32)
    return [vals[np.searchsorted(uniq, t)] for t in angles]


def model_window(p, L, n, source="oracle"):
    if source == "oracle":
        return combine(p, cos_at(p, thetas(L, p.phi_width, n, p.n_terms)))
    c = full_cos(p, source)
    return combine(p, [c[t] for t in thetas(L, p.phi_width, n, p.n_terms)])


def float_window(p, L, shift=None):
    """v = fl32(w) * 2^-shift of the window of length L (shift defaults to dat_width - 1): what the float fronts multiply by."""
    shift = p.dat_width - 1 if shift is None else int(shift)
    w = model_window(p, L, np.arange(L))
    return (w.astype(np.float32) * np.float32(2.0 ** -shift)).astype(np.float32)
