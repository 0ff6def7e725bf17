// bhw_spectrogram.hip -- window, real FFT and power (or filter-bank) rows in one kernel (bhw_spectrogram_f32_device / _from_table;
// contract: include/bhw.h, plan: BhwStftFftPlan in bhw_plan.h, reasons and measurements: DESIGN.md section 20).
//
// The forward kernel of bhw_stft_fft.hip with another epilogue: the row, the passes and the split pass are the one text of
// bhw_stft_fft.h, so (re, im) of a bin are the float32 pair bhw_stft_fft_f32_* writes for it.  After the last pass the Stockham
// buffer that is not `src` is idle; its n_fft floats per slot hold the row's K = M + 1 powers in bank mode.
//   power: lane l of a slot forms the bins k = l, l + lpf, ... <= M and stores fl32((double) re * re + (double) im * im) to the
//          output row: consecutive lanes, consecutive floats.
//   bank:  the same powers go to the idle buffer, one barrier that every lane of the workgroup reaches, then lane l sums the filters
//          m = l, l + lpf, ... one after the other in binary64 in ascending i from +0.0, powers from LDS, first / offset / weight by
//          plain cached global loads (every workgroup reads the same few KiB), and stores consecutive lanes to consecutive columns.
// The bank's arrays are the caller's: offset[m] and offset[m + 1] are clamped to [0, weights] with end >= begin and a band stops at
// bin K, so whatever they hold no read leaves d_weight or the slot's K powers (tests/cpp/san_spectrogram.cpp replays this).
// The mode is a uniform runtime branch: one kernel family with as many instances as the forward kernel has.
#include "bhw_stft_fft.h"

namespace {

struct SpecBank {
    const uint32_t *first, *offset;
    const float *weight;
    uint32_t filters, weights, bank;      // bank 0: power mode, the rest unused
};

// fl32 of the binary64 re^2 + im^2: both squares are exact, the sum rounds once (so a fused multiply-add gives the same value)
__device__ __forceinline__ float spec_power(fft_v2f y)
{
    const double re = (double)y.x, im = (double)y.y;
    return (float)(re * re + im * im);
}

struct FftStorePower {
    static constexpr bool kSpectrum = false;
    SpecBank fb;
    __device__ __forceinline__ void operator()(const FftIo &a, uint32_t M, uint32_t lpf, bool live, uint64_t b, uint64_t f, uint32_t l,
                                               fft_v2f *src, fft_v2f *tw) const
    {
        float *out = a.Y + b * a.y_bstride + f * a.y_stride;
        if (!fb.bank) {
            if (live)
                for (uint32_t k = l; k <= M; k += lpf) out[k] = spec_power(fft_split_bin(src, tw, k, M));
            return;
        }
        float *pw = (float *)fft_idle_buffer(a, threadIdx.x / lpf);      // the slot's K powers (K <= n_fft floats)
        if (live)
            for (uint32_t k = l; k <= M; k += lpf) pw[k] = spec_power(fft_split_bin(src, tw, k, M));
        __syncthreads();                                                // every lane: fb.bank is uniform and this sits outside `live`
        if (live) {
            const uint32_t K = M + 1u, W = fb.weights;
            for (uint32_t m = l; m < fb.filters; m += lpf) {
                uint32_t o0 = fb.offset[m], o1 = fb.offset[m + 1u];
                o0 = o0 < W ? o0 : W;
                o1 = o1 < W ? o1 : W;
                o1 = o1 < o0 ? o0 : o1;
                const uint32_t k0 = fb.first[m];
                uint32_t c = o1 - o0;
                const uint32_t room = k0 < K ? K - k0 : 0u;               // a band stops at bin K
                c = c < room ? c : room;
                double acc = 0.0;
                for (uint32_t i = 0; i < c; ++i) acc = fma((double)pw[k0 + i], (double)fb.weight[o0 + i], acc);
                out[m] = (float)acc;
            }
        }
    }
};

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_stft_fft_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) __attribute__((amdgpu_waves_per_eu(6))) void k_spectrogram_direct(BhwCordicCfg cfg, BhwWinCfg win, FftIo a, BhwLenPhase lp, SpecBank fb)
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
    stft_fft_rows(a, FftStorePower{fb});
}

// Coefficient gathered from a resident table in format FMT (as k_stft_fft_table).
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) __attribute__((amdgpu_waves_per_eu(6))) void k_spectrogram_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, FftIo a,
                                                                  BhwLenPhase lp, SpecBank fb)
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
    stft_fft_rows(a, FftStorePower{fb});
}

} // namespace

// pl: the forward plan with y_stride / y_bstride resolved in floats of the output rows (bhwp_spectrogram_plan)
int bhwk_spectrogram_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwStftFftPlan &pl, const bhw_stft *s,
                         const bhw_fbank *bank, const float *d_x, float *d_P, const int32_t *d_table, const BhwLenPhase &lp)
{
    if (!pl.rows) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    const FftIo a = fft_io(pl, s, d_x, d_P);
    SpecBank fb{};
    if (bank) {
        fb.first = bank->d_first;
        fb.offset = bank->d_offset;
        fb.weight = bank->d_weight;
        fb.filters = bank->filters;
        fb.weights = bank->weights;
        fb.bank = 1u;
    }
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_spectrogram_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp, fb); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_spectrogram_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp, fb);
        });
}
