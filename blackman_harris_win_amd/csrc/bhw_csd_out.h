// bhw_csd_out.h -- the arguments and the output formulas of the Welch cross spectra, one text for bhw_welch_csd.hip (the spectra
// are read from memory) and bhw_csd_fft.hip (the sums come from the fused kernel's workspace): P_xy, P_xx, P_yy, the coherence and H1
// of one (signal, bin) from its ordered binary64 sums (contract: section "Welch cross spectra" of include/bhw.h).
#pragma once
#include "bhw_device.h"

namespace {

typedef float csd_v2f __attribute__((ext_vector_type(2)));

struct CsdArgs {
    const float *X;
    const float *Y;
    float *out[kCsdOutputs];      // d_Pxy, d_Pxx, d_Pyy, d_Cxy, d_H1; read only where the flag is set
    double *ws;
    uint64_t frames, bins, n_fft, blocks, tiles;
    uint64_t x_stride, x_bstride, y_stride, y_bstride, o_stride;
    double scale;
    uint32_t flags;
    uint32_t pad;
};

// The outputs of one (signal, bin) from its sums.  CH == 2: S = {C_re, C_im}; CH == 4: S = {S_xx, S_yy, C_re, C_im}.
template <int CH>
__device__ __forceinline__ void csd_out(const CsdArgs &a, const double *S, uint64_t b, uint64_t k)
{
#pragma clang fp contract(off)                                 // the coherence is written unfused: n + m must stay an add of two rounded squares
    const double sk = bhw_psd_doubled(a.flags & BHW_CSD_ONESIDED ? BHW_PSD_ONESIDED : 0u, k, a.bins, a.n_fft) ? a.scale * 2.0 : a.scale;
    const uint64_t o = b * a.o_stride + k;
    const double cre = S[CH - 2], cim = S[CH - 1];
    if (a.flags & BHW_CSD_PXY) {
        csd_v2f v;
        v.x = (float)(cre * sk);
        v.y = (float)(cim * sk);
        ((csd_v2f *)a.out[0])[o] = v;
    }
    if constexpr (CH == 4) {
        const double sxx = S[0], syy = S[1];
        if (a.flags & BHW_CSD_PXX) a.out[1][o] = (float)(sxx * sk);
        if (a.flags & BHW_CSD_PYY) a.out[2][o] = (float)(syy * sk);
        if (a.flags & BHW_CSD_COHERENCE) {
            const double n = cre * cre, m = cim * cim;
            const double num = n + m, den = sxx * syy;
            a.out[3][o] = (float)(num / den);
        }
        if (a.flags & BHW_CSD_H1) {
            csd_v2f v;
            v.x = (float)(cre / sxx);
            v.y = (float)(cim / sxx);
            ((csd_v2f *)a.out[4])[o] = v;
        }
    }
}

} // namespace
