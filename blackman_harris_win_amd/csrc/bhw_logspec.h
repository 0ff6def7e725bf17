// bhw_logspec.h -- the epilogue of the fused log spectrogram, log-mel spectrogram and MFCC (bhw_logspec_f32_*, bhw_logspec_mfft_f32_*;
// contract: include/bhw.h, reasons and measurements: DESIGN.md section 40): one text for bhw_logspec.hip (under stft_fft_rows of
// bhw_stft_fft.h) and bhw_logspec_mfft.hip (under stft_mfft_rows of bhw_stft_mfft.h).
//
// A slot holds its transformed points in src and has the other Stockham buffer idle; both are M complex64 = n_fft floats.
//   power, no bank: lane l forms the bins k = l, l + lpf, ... <= M and stores g = fl32(mult * log(t)) of the bin's power: no LDS, no
//          barrier.
//   bank:  the powers go to the idle buffer, one barrier that every lane of the workgroup reaches, then lane l sums the filters
//          m = l, l + lpf, ... exactly as bhw_spectrogram.hip does (the same clamps: no read leaves d_weight or the K powers).
//          coeffs == 0: the lane stores g_m in place of the bank value.
//          coeffs > 0:  the lane writes g_m to src viewed as floats (filters <= n_fft of them).  Every fft_split_bin(src, ...) of the
//          slot -- and of every other slot, each on its own src -- precedes the first barrier, so src is dead after it, and the
//          powers in the idle buffer are never overwritten.  A second barrier, reached by every lane (coeffs is a kernel argument),
//          then lane l forms the coefficients j = l, l + lpf, ... < coeffs, a binary64 fma chain over m < filters from +0.0, the
//          matrix by plain cached global loads (consecutive lanes, consecutive floats at each m), and stores consecutive lanes to
//          consecutive columns.  The row function's barrier at the end of the group stands before the next group writes either buffer.
// tests/cpp/san_logspec.cpp replays these steps lane by lane on arrays of the exact sizes.
#pragma once
#include "bhw_stft_mfft.h"

namespace {

struct LogBank {
    const uint32_t *first, *offset;
    const float *weight;
    uint32_t filters, weights, bank;      // bank 0: power rows, the rest unused
};

struct LogStage {
    double floor, mult;
    const float *dct;                     // filters * coeffs floats, [m * coeffs + j]
    uint32_t add, coeffs;                 // add 0: clamp at the floor, 1: add it; coeffs 0: the log rows
};

inline LogBank log_bank(const bhw_fbank *bank)
{
    LogBank fb{};
    if (bank) {
        fb.first = bank->d_first;
        fb.offset = bank->d_offset;
        fb.weight = bank->d_weight;
        fb.filters = bank->filters;
        fb.weights = bank->weights;
        fb.bank = 1u;
    }
    return fb;
}

inline LogStage log_stage(const bhw_logspec *ls)
{
    return LogStage{ls->floor, ls->mult, ls->d_dct, ls->mode == BHW_LOG_ADD ? 1u : 0u, ls->coeffs};
}

// g = fl32(mult * log(t)); a NaN q fails the compare and passes through
__device__ __forceinline__ float log_word(const LogStage &ls, float q)
{
    const double d = (double)q;
    const double t = ls.add ? d + ls.floor : (d < ls.floor ? ls.floor : d);
    return (float)(ls.mult * log(t));
}

// Called by every lane of the workgroup, live or not; out: the row's W floats.
__device__ __forceinline__ void log_row(const LogBank &fb, const LogStage &ls, float *out, uint32_t M, uint32_t lpf, bool live, uint32_t l,
                                        fft_v2f *src, fft_v2f *idle, const fft_v2f *tw)
{
    if (!fb.bank) {
        if (live)
            for (uint32_t k = l; k <= M; k += lpf) out[k] = log_word(ls, mfft_power(fft_split_bin(src, tw, k, M)));
        return;
    }
    float *pw = (float *)idle;                                          // the slot's K powers (K <= n_fft floats)
    if (live)
        for (uint32_t k = l; k <= M; k += lpf) pw[k] = mfft_power(fft_split_bin(src, tw, k, M));
    __syncthreads();                                                    // every lane: fb.bank is uniform and this sits outside `live`
    float *gs = (float *)src;                                           // dead now: the slot's log row under a DCT
    float *to = ls.coeffs ? gs : out;
    if (live) {
        const uint32_t K = M + 1u, W = fb.weights;
        for (uint32_t m = l; m < fb.filters; m += lpf) {
            uint32_t o0 = fb.offset[m], o1 = fb.offset[m + 1u];
            o0 = o0 < W ? o0 : W;
            o1 = o1 < W ? o1 : W;
            o1 = o1 < o0 ? o0 : o1;
            const uint32_t k0 = fb.first[m];
            uint32_t c = o1 - o0;
            const uint32_t room = k0 < K ? K - k0 : 0u;                   // a band stops at bin K
            c = c < room ? c : room;
            double acc = 0.0;
            for (uint32_t i = 0; i < c; ++i) acc = fma((double)pw[k0 + i], (double)fb.weight[o0 + i], acc);
            to[m] = log_word(ls, (float)acc);
        }
    }
    if (!ls.coeffs) return;
    __syncthreads();                                                    // every lane: coeffs is a kernel argument, outside `live`
    if (live) {
        for (uint32_t j = l; j < ls.coeffs; j += lpf) {
            double acc = 0.0;
            for (uint32_t m = 0; m < fb.filters; ++m) acc = fma((double)gs[m], (double)ls.dct[(size_t)m * ls.coeffs + j], acc);
            out[j] = (float)acc;
        }
    }
}

} // namespace
