// bhw_istft_cmfft.hip -- inverse mixed-radix complex FFT, window and overlap-add in one kernel for I/Q output, at n_fft = 2^a 3^b 5^c
// that is no power of two, odd lengths included (bhw_istft_cmfft_f32_device / _from_table; contract: include/bhw.h, plan:
// BhwIstftCmfftPlan in bhw_plan.h, reasons and measurements: DESIGN.md section 31).
//
// The spans, the ring and the flush of bhw_istft_cfft.hip around the passes of bhw_stft_cmfft.h.  No pass, butterfly or twiddle code
// is restated: bhw_stft_mfft.h is included and mfft_pass<R> is called exactly as stft_cmfft_rows calls it (M = fold, Q = n / R,
// ts = n / (R Ns)) over the FORWARD table W[k] = exp(-2 pi i k / n).  The inverse comes from swapping the parts,
//     n * IDFT(Y) = swap(DFT(swap(Y))),   swap(a + i b) = b + i a,
// which costs no instruction: the load stores (Y[k].im, Y[k].re) to LDS and the ring reads re = z.y, im = z.x.
//
// A slot of lpf lanes owns one span of a signal's window-start axis w = t + pad - col0 and walks, in ascending f, the frames that
// reach the span's outputs (bhwp_istft_span).  Prologue, once per workgroup: the window coefficients v[0..L) by the direct CORDIC
// chains or the gather over a resident table, and the twiddle table of fold entries (n / 2 for an even n, n for an odd one), each
// component the float32 rounding of a binary64 sincospi; both stay in LDS.  Then, per frame of the slot:
//   1. the load: a lane reads its complex bins k = c * lpf + l < n (the last column may be missing: the cols mask) with one 8-byte
//      load each, from column k or, under the shift flag, from column (k + n / 2) mod n (integer division; a compare and a subtract),
//      and stores the swapped value: every bin is read once, and the shift is a load index, not a pass;
//   2. the plan's schedule (5s, 3s, 4s, a last 2) between two LDS buffers.  The swapped result z[j] is n_fft times the row; the row is
//      fl32(z * c), c = (float)(1.0 / (double) n_fft): one float32 multiply per part, a rounding the power-of-two kernel does not have;
//   3. the ring: position q = c * lpf + l < n belongs to lane l.  With base = f * hop, ring position q holds w = base + k,
//      k = q - (base mod n), plus n when negative, which frame f reaches at window index k < L and row column col0 + k.  base mod n is
//      taken once per span and stepped by hop mod n with one conditional subtraction per frame.
//      S_c[q] += (double) fl32(row[col0 + k].c * c) * (double) v[k] for both parts c, E[q] += (double) v[k]^2, in binary64 registers;
//   4. the flush: after frame f every w < (f + 1) * hop of the span (after its last frame: every w) is complete; the lane stores
//      (fl32(S_0), fl32(S_1)) or (fl32(S_0 / E), fl32(S_1 / E)) -- one 8-byte store where x allows it, else two 4-byte ones -- and
//      clears the position.  Outputs no frame reaches are stored as (+0.0, +0.0) directly.
// The fy slots of a workgroup hold different spans (of any signals) and pass the same barriers: every slot makes `trips` rounds,
// idle once its frames are done.  A row's arithmetic does not depend on its slot, span or grid, and an output's sum takes its rows in
// ascending f whatever the spans are: the bits of an output are a function of the window, the flags and the rows that reach it.
//
// The text of all this -- IcmfftIo and istft_cmfft_spans -- stands in bhw_istft_cmfft.h, a template on the frame source, since
// bhw_mask_cmfft.hip runs the same spans over frames it forms from an I/Q signal; this unit instantiates the
// source that reads the bins from memory (IstftCmfftBins), and its kernels compiled to the same instruction streams as before the
// move (profiles/r44_istft_iq_disasm.txt).
//
// Kept in step by hand: the span walk, the ring and the flush stand in all four inverse families (bhw_istft_fft.h, bhw_istft_mfft.h,
// bhw_istft_cfft.h, bhw_istft_cmfft.h for this unit and bhw_mask_cmfft.hip); tests/cpp/san_istft_cmfft.cpp replays this family's
// index arithmetic -- the load's column, the pass indices, the ring's stepped base mod n and the flush bound `end` -- from a copy of
// its own.  An edit of any of these in bhw_istft_cmfft.h is an edit of the siblings and of the replay too.  The Io fill, istft_out and
// istft_store are bhw_istft.h's.
#include "bhw_istft_cmfft.h"

namespace {

// The compiler's own choice of registers: 152 a lane and three workgroups per CU.  Under __launch_bounds__(kFftBlock, 4) the kernel
// spills 18 registers to scratch, as bhw_istft_cfft.hip and bhw_istft_mfft.hip do, and the library has no scratch.
// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_istft_cfft_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_istft_cmfft_direct(BhwCordicCfg cfg, BhwWinCfg win, IcmfftIo a, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vS = (float *)(fft_lds + icmfft_window_offset(a));
    for (uint32_t k = threadIdx.x; k < a.len; k += kFftBlock) {
        int32_t w;
        if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
        else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
        vS[k] = fft_coeff(w, a.shift);
    }
    istft_cmfft_spans(a, IstftCmfftBins{});
}

// Coefficient gathered from a resident table in format FMT; every lane reaches the gather (at k = 0 past the window) for the escape
// format's wave-wide fix.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_istft_cmfft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, IcmfftIo a,
                                                                  BhwLenPhase lp)
{
    float *vS = (float *)(fft_lds + icmfft_window_offset(a));
    for (uint32_t k0 = 0; k0 < a.len; k0 += kFftBlock) {
        const uint32_t k = k0 + threadIdx.x;
        const bool in = k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (in) vS[k] = fft_coeff(w, a.shift);
    }
    istft_cmfft_spans(a, IstftCmfftBins{});
}

} // namespace

int bhwk_istft_cmfft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwIstftCmfftPlan &pl, const bhw_stft *s,
                         const float *d_Y, float *d_x, const int32_t *d_table, const BhwLenPhase &lp)
{
    if (!s->samples) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    IcmfftIo a = istft_io<IcmfftIo>(pl, s, d_Y, d_x);
    a.n = pl.n;
    a.fold = pl.fold;
    a.passes = pl.passes;
    for (uint32_t p = 0; p < pl.passes; ++p) a.sched |= (uint32_t)pl.radix[p] << (4u * p);
    a.binshift = pl.shifted ? 1u : 0u;
    a.vec = iq_vec(d_x, s->batch, pl.x_stride);    // one 8-byte store per complex sample, as the power-of-two kernel's
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_istft_cmfft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_istft_cmfft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp);
        });
}
