// bhw_len.hip -- any range [n0, n0 + count) of the coefficient stream of a window of any length L (bhw_generate_len_device /
// bhw_generate_len_from_table)
//
// Part of the hand-written HIP kernels for gfx950 (MI355X, CDNA4) behind include/bhw.h.  Hot path of the reference: phase
// accumulator -> CORDIC rotation chain -> weighted N-term cosine sum -> int32 coefficient, with the
// phase accumulator counting modulo L instead of 2^PHI_WIDTH and each harmonic read at the nearest phi_width-bit angle (bhw_len.h).
//
// One lane per coefficient: the lane reduces its index modulo L (m0 = n0 mod L from the host, then one multiply-high by the
// reciprocal of 2L), and takes the K - 1 harmonics either by the direct CORDIC chains of k_direct / k_frames_direct (direct_coeff_ph,
// direct_coeff_mad_ph) or by the gather of k_range_combine over a resident table (range_coeff_ph): a table holds every
// first-quadrant angle, so it serves the angles of any length.  The whole-period kernels (fused, tile) are not used: their
// quadrant and half-period sharing needs L = 2^PHI_WIDTH.
#include "bhw_device.h"

namespace {

// FORM as direct_form: 2 the mad-form rotation on a rolled loop, 1 / 0 the cordic_full chain with the 64- / 32-bit state.
template <int FORM>
__global__ __launch_bounds__(kBlock) void k_direct_len(BhwCordicCfg cfg, BhwWinCfg win, BhwLenPhase lp, uint64_t m0, uint64_t count,
                                                        int32_t *__restrict__ out)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const uint64_t m = bhw_len_mod(m0 + i, lp);                     // the counter wraps modulo L
    int32_t w;
    if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, m));
    else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, m));
    emit(win, out, i, w);
}

// One lane per coefficient from a resident table in format FMT (range_coeff_ph: NT the term-count bound, MODE the rule).  Lanes past
// count gather too (at m = 0) and store nothing: the escape format resolves marked lanes wave-wide.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kBlock) void k_range_len(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, BhwLenPhase lp,
                                                       uint64_t m0, uint64_t count, int32_t *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool in = i < count;
    const uint64_t m = in ? bhw_len_mod(m0 + i, lp) : 0u;
    const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, m));
    if (in) emit(win, out, i, w);
}

} // namespace

int bhwk_len_range(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const int32_t *d_table, const BhwLenPhase &lp,
                   uint64_t n0, uint64_t count, int32_t *d_out)
{
    if (!count) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    const uint64_t m0 = bhw_len_mod(n0, lp);
    const dim3 grid(grid_for(count)), block(kBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) { launch(k_direct_len<D>, grid, block, st, c_in, w, lp, m0, count, d_out); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch(k_range_len<F, NT, M>, grid, block, st, c, w, tab, lp, m0, count, d_out);
        });
}
