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

// One lane per coefficient (range_coeff in bhw_device.h: FMT the table format, NT the term-count bound, MODE the rule).
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kBlock) void k_range_combine(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table,
                                                           uint64_t n0, uint64_t count, int32_t *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const uint32_t n = (uint32_t)(n0 + i) & ((1u << cfg.phi_width) - 1u);   // the hardware counter wraps modulo 2^PW (N divides 2^64)
    emit(win, out, i, range_coeff<FMT, NT, MODE>(cfg, win, table, n));
}

} // namespace

int bhwk_range_combine(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const int32_t *d_table,
                       uint64_t n0, uint64_t count, int32_t *d_out)
{
    const BhwCordicCfg c = table_layout(c_in);
    if (!count) return 0;
    int fmt, nt, mode;
    if (!bhwp_range_form(c, w, &fmt, &nt, &mode)) return bhwk_table_combine(l, c, w, d_table, n0, count, d_out);
    hipStream_t st = (hipStream_t)l.stream;
    const dim3 grid(grid_for(count)), block(kBlock);
    const void *tab = (const void *)d_table;
    with_range_form(fmt, nt, mode, [&](auto F, auto NT, auto M) {
        launch(k_range_combine<F, NT, M>, grid, block, st, c, w, tab, n0, count, d_out);
    });
    return finish(hipSuccess);
}
