// bhw_stft_fft.hip -- window and real FFT in one kernel (bhw_stft_fft_f32_device / _from_table; contract: include/bhw.h, plan:
// BhwStftFftPlan in bhw_plan.h, reasons and measurements: DESIGN.md section 18).  The row function, its helpers and the account of
// what a workgroup does are in bhw_stft_fft.h, shared with bhw_spectrogram.hip; this unit instantiates the epilogue that stores the
// spectrum row.
#include "bhw_stft_fft.h"

namespace {

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_stft_frames_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_stft_fft_direct(BhwCordicCfg cfg, BhwWinCfg win, FftIo a, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vbuf = (float *)fft_lds;
    for (uint32_t j = threadIdx.x; j < a.n_fft; j += kFftBlock) {
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
    stft_fft_rows(a, FftStoreSpectrum{});
}

// Coefficient gathered from a resident table in format FMT; every lane reaches the gather (at k = 0 outside the window) for the
// escape format's wave-wide fix.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_stft_fft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, FftIo a,
                                                               BhwLenPhase lp)
{
    float *vbuf = (float *)fft_lds;
    for (uint32_t j0 = 0; j0 < a.n_fft; j0 += kFftBlock) {
        const uint32_t j = j0 + threadIdx.x;
        const uint32_t k = j - a.col0;
        const bool in = j < a.n_fft && k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (j < a.n_fft) vbuf[j] = in ? fft_coeff(w, a.shift) : 0.0f;
    }
    __syncthreads();
    stft_fft_rows(a, FftStoreSpectrum{});
}

} // namespace

int bhwk_stft_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwStftFftPlan &pl, const bhw_stft *s,
                      const float *d_x, float *d_Y, const int32_t *d_table, const BhwLenPhase &lp)
{
    if (!pl.rows) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    const FftIo a = fft_io(pl, s, d_x, d_Y);
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_stft_fft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_stft_fft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp);
        });
}
