// bhw_istft_fft.hip -- inverse real FFT, window and overlap-add in one kernel (bhw_istft_fft_f32_device / _from_table; contract:
// include/bhw.h, plan: BhwIstftFftPlan in bhw_plan.h, reasons and measurements: DESIGN.md section 19).
//
// The forward kernel (bhw_stft_fft.hip) mirrored.  A slot of lpf lanes owns one span of a signal's window-start axis w = t + pad -
// col0 and walks, in ascending f, the frames that reach the span's outputs (bhwp_istft_span).  Prologue, once per workgroup: the
// window coefficients v[0..L) by the direct CORDIC chains or the gather over a resident table, and the twiddle table
// W[k] = exp(+2 pi i k / n_fft), k < n_fft / 2, each component the float32 rounding of a binary64 sincospi; both stay in LDS.
// Then, per frame of the slot:
//   1. the pre-split: a lane loads the bins Y[k] and Y[M - k], k <= M / 2 (consecutive lanes, consecutive complex64 values), and
//      forms Z[k] = (Y[k] + conj Y[M - k]) + i (Y[k] - conj Y[M - k]) W[k] and its partner Z[M - k]; Z[0] = (Y[0].re + Y[M].re,
//      Y[0].re - Y[M].re): the imaginary parts of bins 0 and M are never read into the arithmetic;
//   2. an inverse Stockham FFT of M points, out of place between two LDS buffers: the forward's passes with the conjugated table
//      and +i in the radix-4 butterfly.  The result z[i] = (row[2 i], row[2 i + 1]) is n_fft times the row;
//   3. the ring: position w mod n_fft belongs to lane (w mod n_fft) mod lpf, cpl positions a lane.  With base = f * hop, ring
//      position q holds w = base + k, k = (q - base) mod n_fft, which frame f reaches at window index k < L and row column col0 + k:
//      S[q] += (double) fl32(row[col0 + k] / n_fft) * (double) v[k], E[q] += (double) v[k]^2, in binary64 registers.  Consecutive
//      lanes read consecutive floats of the row and of v;
//   4. the flush: after frame f every w < (f + 1) * hop of the span (after its last frame: every w) is complete; the lane stores
//      fl32(S) or fl32(S / E) (consecutive lanes, consecutive samples) and clears the position.  Outputs no frame reaches are
//      stored as +0.0 directly.
// The fy slots of a workgroup hold different spans (of any signals) and pass the same barriers: every slot makes `trips` rounds,
// idle once its frames are done.  A row's arithmetic does not depend on its slot, span or grid, and an output's sum takes its rows in
// ascending f whatever the spans are: the bits of an output are a function of the window and the rows that reach it.
//
// The text of all this -- IfftIo and istft_fft_spans -- stands in bhw_istft_fft.h, a template on the frame source, since
// bhw_mask_fft.hip runs the same spans over frames it forms from a signal; this unit instantiates the source
// that reads the bins from memory (IstftBins), and its kernels compiled to the same instruction streams as before the move.
//
// Kept in step by hand: the span walk, the ring and the flush stand in all four inverse families (bhw_istft_fft.h for this unit and
// bhw_mask_fft.hip, bhw_istft_mfft.hip, bhw_istft_cfft.hip, bhw_istft_cmfft.hip), and tests/cpp/san_istft_fft.cpp replays this
// family's index arithmetic -- the pre-split pairs, the pass indices, the ring's (q - base) mod n_fft and the flush bound `end` --
// from a copy of its own (tests/cpp/san_mask_fft.cpp: the ring and the flush again, under the mask's frame source), since only
// bhwp_istft_span is shared through bhw_plan.h.  An edit of any of these in bhw_istft_fft.h is an edit of the siblings and of the
// replays too.  cmul, twiddle and the dynamic LDS array are bhw_stft_fft.h's, the Io fill and istft_out bhw_istft.h's.
#include "bhw_istft_fft.h"

namespace {

// Four workgroups per CU (128 registers a lane): the compiler's own choice is 129 and three.
// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_stft_fft_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock, 4) void k_istft_fft_direct(BhwCordicCfg cfg, BhwWinCfg win, IfftIo a, BhwLenPhase lp)
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
    istft_fft_spans(a, IstftBins{});
}

// Coefficient gathered from a resident table in format FMT; every lane reaches the gather (at k = 0 past the window) for the escape
// format's wave-wide fix.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock, 4) void k_istft_fft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, IfftIo a,
                                                                BhwLenPhase lp)
{
    float *vS = (float *)(fft_lds + (size_t)(2u * a.fy + 1u) * a.m * sizeof(fft_v2f));
    for (uint32_t k0 = 0; k0 < a.len; k0 += kFftBlock) {
        const uint32_t k = k0 + threadIdx.x;
        const bool in = k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (in) vS[k] = fft_coeff(w, a.shift);
    }
    istft_fft_spans(a, IstftBins{});
}

} // namespace

int bhwk_istft_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwIstftFftPlan &pl, const bhw_stft *s,
                       const float *d_Y, float *d_x, const int32_t *d_table, const BhwLenPhase &lp)
{
    if (!s->samples) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    IfftIo a = istft_io<IfftIo>(pl, s, d_Y, d_x);
    a.n_fft = (uint32_t)s->n_fft;
    a.m = pl.m;
    a.radix4 = pl.radix4;
    a.radix2 = pl.radix2;
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_istft_fft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_istft_fft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp);
        });
}
