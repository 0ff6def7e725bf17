// bhw_logspec.hip -- window, real FFT, power or filter bank, log and (optionally) a DCT in one kernel, n_fft a power of two
// (bhw_logspec_f32_device / _from_table; contract: include/bhw.h, plan: BhwStftFftPlan in bhw_plan.h, reasons and measurements:
// DESIGN.md section 40).
//
// The forward kernel of bhw_stft_fft.hip with one more epilogue: the row, the passes and the split pass are the one text of
// bhw_stft_fft.h, so the power of a bin and the bank value of a filter are the float32 words bhw_spectrogram_f32_* writes.  What
// follows them -- the log, the log row parked in the slot's dead buffer, the second barrier and the DCT -- is log_row of bhw_logspec.h.
#include "bhw_logspec.h"

namespace {

struct FftStoreLog {
    static constexpr bool kSpectrum = false;
    LogBank fb;
    LogStage ls;
    __device__ __forceinline__ void operator()(const FftIo &a, uint32_t M, uint32_t lpf, bool live, uint64_t b, uint64_t f, uint32_t l,
                                               fft_v2f *src, fft_v2f *tw) const
    {
        log_row(fb, ls, a.Y + b * a.y_bstride + f * a.y_stride, M, lpf, live, l, src, fft_idle_buffer(a, threadIdx.x / lpf), tw);
    }
};

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_stft_fft_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) __attribute__((amdgpu_waves_per_eu(5))) void k_logspec_direct(BhwCordicCfg cfg, BhwWinCfg win, FftIo a, BhwLenPhase lp, LogBank fb,
                                                                                                      LogStage ls)
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
    stft_fft_rows(a, FftStoreLog{fb, ls});
}

// Coefficient gathered from a resident table in format FMT (as k_stft_fft_table).
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) __attribute__((amdgpu_waves_per_eu(5))) void k_logspec_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, FftIo a,
                                                                                                     BhwLenPhase lp, LogBank fb, LogStage ls)
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
    stft_fft_rows(a, FftStoreLog{fb, ls});
}

} // namespace

// pl: the forward plan with y_stride / y_bstride resolved in floats of the output rows (bhwp_logspec_plan)
int bhwk_logspec_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwStftFftPlan &pl, const bhw_stft *s,
                     const bhw_fbank *bank, const bhw_logspec *lg, const float *d_x, float *d_out, const int32_t *d_table, const BhwLenPhase &lp)
{
    if (!pl.rows) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    const FftIo a = fft_io(pl, s, d_x, d_out);
    const LogBank fb = log_bank(bank);
    const LogStage ls = log_stage(lg);
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_logspec_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp, fb, ls); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_logspec_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp, fb, ls);
        });
}
