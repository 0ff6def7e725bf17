// bhw_istft_mfft.hip -- inverse mixed-radix real FFT, window and overlap-add in one kernel, for even n_fft = 2^a 3^b 5^c that is no
// power of two (bhw_istft_mfft_f32_device / _from_table; contract: include/bhw.h, plan: BhwIstftMfftPlan in bhw_plan.h, reasons and
// measurements: DESIGN.md section 24).
//
// The span / halo / ring / flush kernel of bhw_istft_fft.hip with the generic Stockham pass of bhw_stft_mfft.hip inside.  A slot of
// lpf lanes owns one span of a signal's window-start axis w = t + pad - col0 and walks, in ascending f, the frames that reach the
// span's outputs (bhwp_istft_span).  Prologue, once per workgroup: the window coefficients v[0..L) by the direct CORDIC chains or the
// gather over a resident table, and the twiddle table W[k] = exp(+2 pi i k / n_fft), k < M = n_fft / 2, each component the float32
// rounding of a binary64 sincospi; both stay in LDS.  Then, per frame of the slot:
//   1. the pre-split for any M: a lane loads the bins Y[k] and Y[M - k], k = l, l + lpf, ... <= floor(M / 2), each bin once, and forms
//      Z[k] = (Y[k] + conj Y[M - k]) + i (Y[k] - conj Y[M - k]) W[k] and its partner Z[M - k] with W[M - k] = -conj W[k];
//      Z[0] = (Y[0].re + Y[M].re, Y[0].re - Y[M].re): the imaginary parts of bins 0 and M are never read into the arithmetic.  M may
//      be odd: then no bin is its own mirror, and the self-partner test is 2 k == M;
//   2. an inverse Stockham FFT of M points, out of place between two LDS buffers, in the forward's schedule (radix-5 passes, radix-3,
//      radix-4, a last radix-2): butterfly i < M / r reads src[i + q * M / r], multiplies by W at the EXACT index
//      q * k * (n_fft / (r Ns)), k = i mod Ns (indices >= M fold by W[i + M] = -W[i] with a compare), runs the conjugated butterfly
//      and writes dst[(i - k) * r + k + q * Ns].  i mod Ns is the forward's one float multiply.  The result
//      z[i] = (row[2 i], row[2 i + 1]) is n_fft times the row; the row is fl32(z * c), c = (float)(1.0 / (double) n_fft): one
//      float32 multiply, a rounding the power-of-two kernel does not have;
//   3. the ring: position q = c * lpf + l < n_fft belongs to lane l (a lane's last column may be missing: the cols mask).  With
//      base = f * hop, ring position q holds w = base + k, k = q - (base mod n_fft), plus n_fft when negative, which frame f reaches
//      at window index k < L and row column col0 + k.  base mod n_fft is taken once per span and stepped by hop mod n_fft with one
//      conditional subtraction per frame.  S[q] += (double) fl32(row[col0 + k] * c) * (double) v[k], E[q] += (double) v[k]^2, in
//      binary64 registers;
//   4. the flush of bhw_istft_fft.hip: after frame f every w < (f + 1) * hop of the span (after its last frame: every w) is complete;
//      the lane stores fl32(S) or fl32(S / E) (consecutive lanes, consecutive samples) and clears the position.  Outputs no frame
//      reaches are stored as +0.0 directly.
// The fy slots of a workgroup hold different spans (of any signals) and pass the same barriers: every slot makes `trips` rounds,
// idle once its frames are done.  A row's arithmetic does not depend on its slot, span or grid, and an output's sum takes its rows in
// ascending f whatever the spans are: the bits of an output are a function of the window and the rows that reach it.
//
// The text of all this -- ImfftIo, imf_butterfly, imf_pass and istft_mfft_spans -- stands in bhw_istft_mfft.h, a template on the frame
// source that bhw_mask_mfft.hip shares; this unit is its ImfIstftBins instance, steps 1 to 4 as above, and the
// move left the instruction streams of its 48 kernels as they were (profiles/r42_istft_mfft_disasm.txt).
//
// Kept in step by hand: imf_pass restates mfft_pass of bhw_stft_mfft.h around the conjugated butterfly, and the span walk, the ring
// and the flush stand in all four inverse families (bhw_istft_fft.h, bhw_istft_mfft.h, bhw_istft_cfft.hip, bhw_istft_cmfft.hip);
// tests/cpp/san_istft_mfft.cpp replays the header's index arithmetic -- the pre-split pairs, the pass indices and the float i mod Ns,
// the ring's stepped base mod n_fft and the flush bound `end` -- from a copy of its own, since only bhwp_istft_span is shared
// through bhw_plan.h.  An edit of any of these there is an edit of the siblings and of the replay too.  cmul, mfft_twiddle, the radix
// constants and the dynamic LDS array are bhw_stft_mfft.h's and bhw_stft_fft.h's, the Io fill and istft_out bhw_istft.h's.
#include "bhw_istft_mfft.h"

namespace {

// The compiler's own choice of registers: 156 a lane and three workgroups per CU.  Under __launch_bounds__(kFftBlock, 4), which
// bhw_istft_fft.hip holds at 127, the radix-5 butterfly spills 26 registers to scratch, and the library has no scratch.
// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_istft_fft_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_istft_mfft_direct(BhwCordicCfg cfg, BhwWinCfg win, ImfftIo a, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vS = (float *)(fft_lds + (size_t)(2u * a.fy + 1u) * a.m * sizeof(fft_v2f));
    for (uint32_t k = threadIdx.x; k < a.len; k += kFftBlock) {
        int32_t w;
        if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
        else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
        vS[k] = fft_coeff(w, a.shift);
    }
    istft_mfft_spans(a, ImfIstftBins{});
}

// Coefficient gathered from a resident table in format FMT; every lane reaches the gather (at k = 0 past the window) for the escape
// format's wave-wide fix.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_istft_mfft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, ImfftIo a,
                                                                 BhwLenPhase lp)
{
    float *vS = (float *)(fft_lds + (size_t)(2u * a.fy + 1u) * a.m * sizeof(fft_v2f));
    for (uint32_t k0 = 0; k0 < a.len; k0 += kFftBlock) {
        const uint32_t k = k0 + threadIdx.x;
        const bool in = k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (in) vS[k] = fft_coeff(w, a.shift);
    }
    istft_mfft_spans(a, ImfIstftBins{});
}

} // namespace

int bhwk_istft_mfft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwIstftMfftPlan &pl, const bhw_stft *s,
                        const float *d_Y, float *d_x, const int32_t *d_table, const BhwLenPhase &lp)
{
    if (!s->samples) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    ImfftIo a = istft_io<ImfftIo>(pl, s, d_Y, d_x);
    a.n_fft = (uint32_t)s->n_fft;
    a.m = pl.m;
    a.passes = pl.passes;
    for (uint32_t p = 0; p < pl.passes; ++p) a.sched |= (uint32_t)pl.radix[p] << (4u * p);
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_istft_mfft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_istft_mfft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp);
        });
}
