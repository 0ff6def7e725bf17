// bhw_logspec_mfft.hip -- bhw_logspec.hip for even n_fft = 2^a 3^b 5^c that is no power of two (bhw_logspec_mfft_f32_device /
// _from_table; contract: include/bhw.h, plan: BhwStftMfftPlan in bhw_plan.h, reasons and measurements: DESIGN.md section 40).
//
// The forward kernel of bhw_stft_mfft.hip with the row epilogue of bhw_logspec.h: stft_mfft_rows hands an epilogue with kRows the
// slot's transformed points and its idle buffer at compile time, so the stored forms of MfftStore gain no run-time form.  The power
// of a bin and the bank value of a filter are the float32 words bhw_stft_mfft_f32_* writes under BHW_MFFT_POWER.
#include "bhw_logspec.h"

namespace {

struct MfftStoreLog {
    static constexpr bool kStore = false;
    static constexpr bool kRuns = false;
    static constexpr bool kRows = true;
    LogBank fb;
    LogStage ls;
    __device__ __forceinline__ void operator()(const MfftIo &a, uint32_t lpf, bool live, uint64_t b, uint64_t f, uint32_t l, fft_v2f *src,
                                               fft_v2f *dst, fft_v2f *tw) const
    {
        log_row(fb, ls, a.Y + b * a.y_bstride + f * a.y_stride, a.m, lpf, live, l, src, dst, tw);
    }
};

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_stft_mfft_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_logspec_mfft_direct(BhwCordicCfg cfg, BhwWinCfg win, MfftIo a, BhwLenPhase lp, LogBank fb, LogStage ls)
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
    stft_mfft_rows(a, MfftStoreLog{fb, ls});
}

// Coefficient gathered from a resident table in format FMT; every lane reaches the gather (at k = 0 outside the window) for the
// escape format's wave-wide fix.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_logspec_mfft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, MfftIo a,
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
    stft_mfft_rows(a, MfftStoreLog{fb, ls});
}

} // namespace

// pl: the forward plan with y_stride / y_bstride resolved in floats of the output rows (bhwp_logspec_mfft_plan)
int bhwk_logspec_mfft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwStftMfftPlan &pl, const bhw_stft *s,
                          const bhw_fbank *bank, const bhw_logspec *lg, const float *d_x, float *d_out, const int32_t *d_table,
                          const BhwLenPhase &lp)
{
    if (!pl.rows) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    const MfftIo a = mfft_io(pl, s, d_x, d_out);
    const LogBank fb = log_bank(bank);
    const LogStage ls = log_stage(lg);
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_logspec_mfft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp, fb, ls); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_logspec_mfft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp, fb, ls);
        });
}
