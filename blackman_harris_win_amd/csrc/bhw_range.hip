// bhw_range.hip -- any range [n0, n0 + count) of the coefficient stream over a resident first-quadrant table (bhw_table_create)
//
// Part of the hand-written HIP kernels for gfx950 (MI355X, CDNA4) behind include/bhw.h.  Hot path of the reference: phase
// accumulator -> CORDIC rotation chain (or Taylor LUT) -> weighted N-term cosine sum -> int32 coefficient (SURVEY section 8a
// rows a1-a11).  Integer semantics follow SURVEY App. A; reference lines are cited at each step.
//
// A resident table is held in the layout its configuration's whole periods read: packed and split (or natural, for the one-byte
// formats) where the tile kernel applies, plain and natural otherwise.  The ragged pieces of a from-table call -- a streaming
// chunk of WinSelector.enable(), the head and tail around whole periods -- read that same table directly, in whatever format it
// is, with no second 8-byte-per-entry copy.  k_table_combine does that too, but it reads the format from the configuration at
// run time in every gather and resolves a listed entry of the escape format per lane in a probe loop; here the format is a
// compile-time parameter, the K - 1 gathers of a lane issue together, and the escape format costs one test per lane (the
// minimum of its low fields over the harmonics) with the rare marked lane resolved on the scalar unit (esc_fix_wave).
#include "bhw_device.h"

namespace {

// One lane per coefficient.  FMT: the table format (fmt_of: 0 plain, 1 delta16, 2 residual, 3 nibble, 5 nibble + escapes);
// NT: bound of the term count (3, 5, 7: the harmonics k < win.n_terms are taken, a wave-uniform test); MODE as in
// k_table_combine_fold_t: 0 HLS rule, 1 HLS rule with the one's-complement quadrant map (cpp model), 2 VHDL rule.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kBlock) void k_range_combine(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table,
                                                           uint64_t n0, uint64_t count, int32_t *__restrict__ out)
{
    constexpr uint32_t COMBINE = MODE == 2 ? BHW_COMBINE_VHDL : BHW_COMBINE_HLS;
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const uint32_t pw = cfg.phi_width, W = cfg.dat_width;
    const uint32_t mask = (1u << pw) - 1u, tmask = (1u << (pw - 2u)) - 1u;
    const uint32_t lq = pw - 2u - cfg.z_shr;                       // log2 of the table's entries
    const uint32_t n = (uint32_t)(n0 + i) & mask;                  // the hardware counter wraps modulo 2^PW (N divides 2^64)
    const uint32_t nt = win.n_terms;
    int2 cs[NT];
    uint32_t q[NT];
    uint32_t ent[NT];                                              // FMT 5: entry index and stored byte, for the escape test
    uint32_t byte[NT];
    uint32_t low_min = 15u;
#pragma unroll
    for (int k = 1; k < NT; ++k) {
        cs[k] = make_int2(0, 0);
        q[k] = 0u;
        ent[k] = byte[k] = 0u;
        if ((uint32_t)k < nt) {
            const uint32_t theta = ((uint32_t)k * n) & mask;
            q[k] = theta >> (pw - 2u);
            const uint32_t u = (theta & tmask) >> cfg.z_shr;
            if constexpr (FMT == 5) {
                // the nibble decode of tab_fetch, the marker left to the test below
                const uint32_t d = fmt_cell_log(cfg.tab_dlog);
                const int4 rec = ld_off<int4>(cfg.tab_coarse, (u >> d) << 4);
                const uint32_t e = ld_off<uint8_t>(table, u);
                const int2 p = tab_predict_nib(rec, u & ((1u << d) - 1u), d), f = nib_fields(e);
                cs[k] = make_int2(p.x + f.x, p.y + f.y);
                ent[k] = u;
                byte[k] = e;
                low_min = min(low_min, e & 15u);
            } else {
                cs[k] = tab_fetch<FMT>(cfg, table, u, tab_index<0, -1>(u, lq, cfg.tab_split));
            }
        }
    }
    if constexpr (FMT == 5) {
        // one test per lane over all its harmonics; listed entries are a few per million, so the branch is almost never taken
        if (__builtin_expect(low_min == kEscMarker, 0)) {
#pragma unroll
            for (int k = 1; k < NT; ++k)
                if ((uint32_t)k < nt) esc_fix_wave(cfg.tab_esc, cfg.esc_wg_log, lq, ent[k], (byte[k] & 15u) == kEscMarker, cs[k]);
        }
    }
    Sum32 acc = MODE == 2 ? sum32_first(win.aa[0]) : Sum32{win.aa[0], win.aa[0]};
    const uint32_t ones_neg = MODE == 0 ? 0u : MODE == 1 ? 1u : cfg.ones_neg;
#pragma unroll
    for (int k = 1; k < NT; ++k) {
        if ((uint32_t)k < nt) {
            int32_t c, s;
            quadrant_map(q[k], cs[k].x, cs[k].y, ones_neg, c, s);
            w32_term<COMBINE>(acc, win.aa[k], c, (uint32_t)k, W);
        }
    }
    emit(win, out, i, w32_final<COMBINE>(acc, W, nt));
}

} // namespace

int bhwk_range_combine(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const int32_t *d_table,
                       uint64_t n0, uint64_t count, int32_t *d_out)
{
    const BhwCordicCfg c = table_layout(c_in);
    if (!count) return 0;
    int fmt, nt, mode;
    if (!bhwp_range_form(c, w, &fmt, &nt, &mode)) return bhwk_table_combine(l, c, w, d_table, n0, count, d_out);
    BHW_SET_DEVICE(l);
    hipStream_t st = (hipStream_t)l.stream;
    const dim3 grid(grid_for(count)), block(kBlock);
    const void *tab = (const void *)d_table;
#define BHW_RANGE_F(F, NT, M) BHW_LAUNCH((k_range_combine<F, NT, M>), grid, block, 0, st, c, w, tab, n0, count, d_out)
#define BHW_RANGE_NT(F, M)                                                                                               \
    do {                                                                                                                 \
        if (nt == 3)      BHW_RANGE_F(F, 3, M);                                                                          \
        else if (nt == 5) BHW_RANGE_F(F, 5, M);                                                                          \
        else              BHW_RANGE_F(F, 7, M);                                                                          \
    } while (0)
#define BHW_RANGE_M(F)                                                                                                   \
    do {                                                                                                                 \
        if (mode == 0)      BHW_RANGE_NT(F, 0);                                                                          \
        else if (mode == 1) BHW_RANGE_NT(F, 1);                                                                          \
        else                BHW_RANGE_NT(F, 2);                                                                          \
    } while (0)
    switch (fmt) {
    case 0: BHW_RANGE_M(0); break;
    case 1: BHW_RANGE_M(1); break;
    case 2: BHW_RANGE_M(2); break;
    case 3: BHW_RANGE_M(3); break;
    default: BHW_RANGE_M(5); break;
    }
#undef BHW_RANGE_M
#undef BHW_RANGE_NT
#undef BHW_RANGE_F
    return finish(hipSuccess);
}
