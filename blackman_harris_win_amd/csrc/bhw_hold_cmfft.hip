// bhw_hold_cmfft.hip -- window, mixed-radix complex FFT and the max-hold / min-hold traces over the frames in one kernel for
// interleaved I/Q input at n_fft = 2^a 3^b 5^c that is no power of two, odd lengths included (bhw_hold_cmfft_f32_device /
// _from_table; contract: include/bhw.h, plan: BhwHoldCmfftPlan in bhw_plan.h, reasons and measurements: DESIGN.md section 33).
//
// The row function of bhw_stft_cmfft.h, unedited, under the epilogue of bhw_hold.h, as bhw_hold_cfft.hip is the power-of-two kernel
// under it: the power of a bin is the float32 word bhw_stft_cmfft_f32_* writes for it under BHW_CFFT_POWER (mfft_power's expression),
// and the (B, F, n_fft) powers never exist.  The kernels below are k_welch_cmfft_direct / _table of bhw_welch_cmfft.hip with that
// epilogue in place of the binary64 sums; the join is bhwk_hold_join of bhw_hold_cfft.hip.
#include "bhw_stft_cmfft.h"
#include "bhw_hold.h"

namespace {

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_stft_cmfft_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_hold_cmfft_direct(BhwCordicCfg cfg, BhwWinCfg win, CmfftIo a, BhwLenPhase lp, HoldAcc wa)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vbuf = (float *)fft_lds;
    for (uint32_t j = threadIdx.x; j < a.n; j += kFftBlock) {
        const uint32_t k = j - a.col0;                             // unsigned: k < L is the window test
        float v = 0.0f;
        if (k < a.len) {
            int32_t w;
            if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
            else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
            v = fft_coeff(w, a.shift);
        }
        vbuf[j] = v;
    }
    __syncthreads();
    stft_cmfft_rows(a, HoldAccumulate<CmfftIo>(wa));
}

// Coefficient gathered from a resident table in format FMT (as k_stft_cmfft_table).
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_hold_cmfft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, CmfftIo a,
                                                                 BhwLenPhase lp, HoldAcc wa)
{
    float *vbuf = (float *)fft_lds;
    for (uint32_t j0 = 0; j0 < a.n; j0 += kFftBlock) {
        const uint32_t j = j0 + threadIdx.x;
        const uint32_t k = j - a.col0;
        const bool in = j < a.n && k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (j < a.n) vbuf[j] = in ? fft_coeff(w, a.shift) : 0.0f;
    }
    __syncthreads();
    stft_cmfft_rows(a, HoldAccumulate<CmfftIo>(wa));
}

} // namespace

int bhwk_hold_cmfft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwHoldCmfftPlan &hp, const bhw_stft *s,
                        double scale, const float *d_x, float *d_max, float *d_min, void *d_ws, const int32_t *d_table,
                        const BhwLenPhase &lp)
{
    const BhwWelchCmfftPlan &wp = hp.welch;
    const BhwStftCmfftPlan &pl = wp.fft;
    if (!pl.rows) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    const CmfftIo a = cmfft_io(pl, s, d_x, nullptr);
    HoldAcc wa{};
    wa.chunk_ws = (uint2 *)d_ws;
    wa.fpad = wp.fpad;
    wa.chunks = wp.chunks;
    wa.gpr = wp.gpr;
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    const int e = with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_hold_cmfft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp, wa); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_hold_cmfft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp, wa);
        });
    if (e) return e;
    return bhwk_hold_join(l, d_ws, d_max, d_min, s->batch, wp.bins, s->n_fft, wp.chunks, wp.blocks, wp.blocks_grid, wp.join_grid, wp.p_stride,
                          scale, 0u);
}
