// bhw_istft_cfft.hip -- inverse complex FFT, window and overlap-add in one kernel for I/Q output (bhw_istft_cfft_f32_device /
// _from_table; contract: include/bhw.h, plan: BhwIstftCfftPlan in bhw_plan.h, reasons and measurements: DESIGN.md section 22).
//
// The spans, the ring and the flush of bhw_istft_fft.hip around the transform of bhw_stft_cfft.hip, conjugated.  A slot of lpf lanes
// owns one span of a signal's window-start axis w = t + pad - col0 and walks, in ascending f, the frames that reach the span's outputs
// (bhwp_istft_span).  Prologue, once per workgroup: the window coefficients v[0..L) by the direct CORDIC chains or the gather over a
// resident table, and the twiddle table W[k] = exp(+2 pi i k / n), k < n / 2, n = n_fft, each component the float32 rounding of a
// binary64 sincospi; both stay in LDS.  Then, per frame of the slot:
//   1. the load: lane l reads the complex bins k = c * lpf + l, c < cpl, with one 8-byte load each (consecutive lanes, consecutive
//      complex64 values), from column k or, under the shift flag, from column (k + n / 2) mod n: every bin is read once, and the
//      shift is a load index, not a pass;
//   2. an inverse Stockham FFT of n points, out of place between two LDS buffers: the forward's passes (bhw_stft_cfft.hip) with the
//      conjugated table and +i in the radix-4 butterfly.  The result z[j] is n_fft times the row;
//   3. the ring: position w mod n belongs to lane (w mod n) mod lpf, cpl positions a lane.  With base = f * hop, ring position q
//      holds w = base + k, k = (q - base) mod n, which frame f reaches at window index k < L and row column col0 + k:
//      S_c[q] += (double) fl32(row[col0 + k].c / n) * (double) v[k] for both parts c, E[q] += (double) v[k]^2, in binary64 registers;
//   4. the flush: after frame f every w < (f + 1) * hop of the span (after its last frame: every w) is complete; the lane stores
//      (fl32(S_0), fl32(S_1)) or (fl32(S_0 / E), fl32(S_1 / E)) -- one 8-byte store where x allows it, else two 4-byte ones -- and
//      clears the position.  Outputs no frame reaches are stored as (+0.0, +0.0) directly.
// The fy slots of a workgroup hold different spans (of any signals) and pass the same barriers: every slot makes `trips` rounds,
// idle once its frames are done.  A row's arithmetic does not depend on its slot, span or grid, and an output's sum takes its rows in
// ascending f whatever the spans are: the bits of an output are a function of the window, the flags and the rows that reach it.
//
// The text of all this -- IcfftIo and istft_cfft_spans -- stands in bhw_istft_cfft.h, a template on the frame source, since
// bhw_mask_cfft.hip runs the same spans over frames it forms from an I/Q signal; this unit instantiates the
// source that reads the bins from memory (IstftCfftBins), and its kernels compiled to the same instruction streams as before the move
// (profiles/r44_istft_iq_disasm.txt).
//
// Kept in step by hand: the span walk, the ring and the flush stand in all four inverse families (bhw_istft_fft.h, bhw_istft_mfft.h,
// bhw_istft_cfft.h for this unit and bhw_mask_cfft.hip, bhw_istft_cmfft.h), and tests/cpp/san_istft_cfft.cpp replays this family's
// index arithmetic -- the load's point index, the pass indices, the ring's (q - base) mod n and the flush bound `end` -- from a copy of
// its own, since only bhwp_istft_span is shared through bhw_plan.h.  An edit of any of these in bhw_istft_cfft.h is an edit of the
// siblings and of the replay too.  cmul, twiddle and the dynamic LDS array are bhw_stft_fft.h's, the Io fill, istft_out and
// istft_store bhw_istft.h's.
#include "bhw_istft_cfft.h"

namespace {

// Three workgroups per CU (137 registers a lane, the compiler's own choice, and the LDS bound at n_fft 2048): asking for four
// (128 registers) spills six registers to scratch.
// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_istft_fft_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_istft_cfft_direct(BhwCordicCfg cfg, BhwWinCfg win, IcfftIo a, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vS = (float *)(fft_lds + ((size_t)2u * a.fy * a.n + a.n / 2u) * sizeof(fft_v2f));
    for (uint32_t k = threadIdx.x; k < a.len; k += kFftBlock) {
        int32_t w;
        if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
        else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
        vS[k] = fft_coeff(w, a.shift);
    }
    istft_cfft_spans(a, IstftCfftBins{});
}

// Coefficient gathered from a resident table in format FMT; every lane reaches the gather (at k = 0 past the window) for the escape
// format's wave-wide fix.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_istft_cfft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, IcfftIo a,
                                                                 BhwLenPhase lp)
{
    float *vS = (float *)(fft_lds + ((size_t)2u * a.fy * a.n + a.n / 2u) * sizeof(fft_v2f));
    for (uint32_t k0 = 0; k0 < a.len; k0 += kFftBlock) {
        const uint32_t k = k0 + threadIdx.x;
        const bool in = k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (in) vS[k] = fft_coeff(w, a.shift);
    }
    istft_cfft_spans(a, IstftCfftBins{});
}

} // namespace

int bhwk_istft_cfft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwIstftCfftPlan &pl, const bhw_stft *s,
                        const float *d_Y, float *d_x, const int32_t *d_table, const BhwLenPhase &lp)
{
    if (!s->samples) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    IcfftIo a = istft_io<IcfftIo>(pl, s, d_Y, d_x);
    a.n = pl.n;
    a.radix4 = pl.radix4;
    a.radix2 = pl.radix2;
    a.binshift = pl.shifted ? 1u : 0u;
    a.vec = iq_vec(d_x, s->batch, pl.x_stride);    // one 8-byte store per complex sample, as the load of bhw_stft_cfft.hip
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_istft_cfft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_istft_cfft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp);
        });
}
