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
// Kept in step by hand: the span walk, the ring and the flush stand in all four inverse units (bhw_istft_fft.hip,
// bhw_istft_mfft.hip, bhw_istft_cfft.hip, this one); tests/cpp/san_istft_cmfft.cpp replays this file's index arithmetic -- the
// load's column, the pass indices, the ring's stepped base mod n and the flush bound `end` -- from a copy of its own.  An edit of
// any of these here is an edit of the siblings and of the replay too.  The Io fill, istft_out and istft_store are bhw_istft.h's.
#include "bhw_istft.h"
#include "bhw_stft_mfft.h"

namespace {

struct IcmfftIo {
    const float *Y;
    float *x;
    uint64_t batch, frames, hop, samples, t0;
    uint64_t x_stride, y_stride, y_bstride;
    uint64_t span, spans, groups, trips;
    uint32_t n, fold, col0, len;
    uint32_t lpf, fy, cpl, passes;
    uint32_t sched;                       // the radix of pass p in bits 4p .. 4p + 3
    uint32_t shift, normalize, binshift, vec;
};

// the float offset of the window coefficients in the dynamic LDS: behind the two buffers and the twiddles
__device__ __forceinline__ size_t icmfft_window_offset(const IcmfftIo &a) { return ((size_t)2u * a.fy * a.n + a.fold) * sizeof(fft_v2f); }

// Everything after the prologue's coefficients: vS (behind the twiddles) holds v[0..L).
__device__ __forceinline__ void istft_cmfft_spans(const IcmfftIo &a)
{
    const uint32_t n = a.n, fold = a.fold, lpf = a.lpf, fy = a.fy, L = a.len;
    fft_v2f *bufA = (fft_v2f *)fft_lds;
    fft_v2f *bufB = bufA + (size_t)fy * n;
    fft_v2f *tw = bufB + (size_t)fy * n;
    const float *vS = (const float *)(tw + fold);
    const uint32_t tid = threadIdx.x;
    const uint32_t slot = tid / lpf, l = tid - slot * lpf;
    for (uint32_t k = tid; k < fold; k += kFftBlock) {                   // the forward table, as stft_cmfft_rows fills it
        double sn, cs;
        sincospi((double)k * 2.0 / (double)n, &sn, &cs);
        tw[k] = fft_v2f{(float)cs, (float)-sn};
    }
    __syncthreads();
    const float scale = (float)(1.0 / (double)n);                        // not a power of two: the multiply rounds
    const uint64_t pool = a.batch * a.spans, hop = a.hop;
    const uint32_t turn = a.binshift ? n >> 1 : 0u;
    const uint32_t hm = (uint32_t)(hop % (uint64_t)n);
    const fft_v2f zero = fft_v2f{0.0f, 0.0f};
    // bit c of cols: the lane has a ring position (and a bin) c (c * lpf + l < n: the last one may be missing)
    uint32_t cols = 0;
#pragma unroll
    for (uint32_t c = 0; c < kCfftMaxCpl; ++c)
        if (c < a.cpl && c * lpf + l < n) cols |= 1u << c;
    double accr[kCfftMaxCpl], acci[kCfftMaxCpl], env[kCfftMaxCpl];
#pragma unroll
    for (uint32_t c = 0; c < kCfftMaxCpl; ++c) accr[c] = acci[c] = env[c] = 0.0;
    for (uint64_t g = blockIdx.x; g < a.groups; g += gridDim.x) {
        const uint64_t sp = g * fy + slot;
        const bool live = sp < pool;
        const uint64_t b = live ? sp / a.spans : 0, s = live ? sp - b * a.spans : 0;
        BhwIstftSpan r = bhwp_istft_span(s, a.span, hop, L, a.t0, a.samples, a.frames);
        if (!live) r.wlo = r.whi = r.f_lo = r.f_hi = 0;
        const float *yb = a.Y + b * a.y_bstride;
        float *xb = a.x + b * a.x_stride;                                // output t = w - t0 (every w formed below is >= wlo >= t0)
        uint64_t cur = r.wlo;                                            // the span's outputs below cur are stored
        uint32_t bm = (uint32_t)((r.f_lo * hop) % (uint64_t)n);          // (f * hop) mod n of the round's frame, stepped below
        for (uint64_t it = 0; it < a.trips; ++it) {
            const uint64_t f = r.f_lo + it;
            const bool act = f < r.f_hi;
            // 1. the load, parts swapped, into the slot's row of buffer A
            fft_v2f *src = bufA + (size_t)slot * n, *dst = bufB + (size_t)slot * n;
            if (act) {
                const fft_v2f *yp = (const fft_v2f *)(yb + f * a.y_stride);
#pragma unroll
                for (uint32_t c = 0; c < kCfftMaxCpl; ++c) {
                    if ((cols >> c) & 1u) {
                        const uint32_t k = c * lpf + l;                  // bin k sits in column k, or (k + n / 2) mod n
                        uint32_t col = k + turn;
                        col = col >= n ? col - n : col;
                        const fft_v2f y = yp[col];
                        src[k] = fft_v2f{y.y, y.x};
                    }
                }
            }
            __syncthreads();
            // 2. the passes (every slot, idle ones on stale data: their result is not read): Ns the product of the radices so far,
            //    rest = n / (Ns * r) after this pass = the twiddle stride n / (r Ns)
            uint32_t Ns = 1, rest = n;
            for (uint32_t p = 0; p < a.passes; ++p) {
                const uint32_t rdx = (a.sched >> (4u * p)) & 15u;
                if (rdx == 5u) {
                    rest /= 5u;
                    mfft_pass<5>(src, dst, tw, fold, n / 5u, Ns, rest, l, lpf);
                } else if (rdx == 3u) {
                    rest /= 3u;
                    mfft_pass<3>(src, dst, tw, fold, n / 3u, Ns, rest, l, lpf);
                } else if (rdx == 4u) {
                    rest >>= 2;
                    mfft_pass<4>(src, dst, tw, fold, n >> 2, Ns, rest, l, lpf);
                } else {
                    rest >>= 1;
                    mfft_pass<2>(src, dst, tw, fold, n >> 1, Ns, rest, l, lpf);
                }
                __syncthreads();
                fft_v2f *sw = src;
                src = dst;
                dst = sw;
                Ns *= rdx;
            }
            // 3. and 4.: the ring
            if (act) {
                const fft_v2f *row = src + a.col0;
                const uint64_t base = f * hop;
                if (cur < base) {                                        // a gap no frame reaches (hop > L, or the span's start)
                    for (uint64_t w = cur + l; w < base; w += lpf) istft_store(xb, w - a.t0, zero, a.vec);
                    cur = base;
                }
                uint64_t end = (f + 1 == r.f_hi || base + hop > r.whi) ? r.whi : base + hop;
                if (end < cur) end = cur;                                // a halo frame whose own hop lies before the span
#pragma unroll
                for (uint32_t c = 0; c < kCfftMaxCpl; ++c) {
                    if ((cols >> c) & 1u) {
                        const uint32_t q = c * lpf + l;
                        const uint32_t k = q >= bm ? q - bm : q + n - bm;
                        const uint64_t w = base + k;
                        if (k < L && w >= cur && w < r.whi) {
                            const double v = (double)vS[k];
                            const fft_v2f z = row[k];                    // swapped: re = z.y, im = z.x
                            accr[c] += (double)(z.y * scale) * v;
                            acci[c] += (double)(z.x * scale) * v;
                            env[c] += v * v;
                            if (w < end) {
                                istft_store(xb, w - a.t0,
                                             fft_v2f{istft_out(accr[c], env[c], a.normalize), istft_out(acci[c], env[c], a.normalize)}, a.vec);
                                accr[c] = acci[c] = env[c] = 0.0;
                            }
                        }
                    }
                }
                const uint64_t reach = base + L;                         // the frame's extent: beyond it up to `end` nothing is summed
                if (reach < end)
                    for (uint64_t w = (reach > cur ? reach : cur) + l; w < end; w += lpf) istft_store(xb, w - a.t0, zero, a.vec);
                cur = end;
            }
            bm += hm;                                                    // ((f + 1) * hop) mod n: both terms are below n
            if (bm >= n) bm -= n;
            __syncthreads();                                             // the next round overwrites both buffers
        }
        if (live)
            for (uint64_t w = cur + l; w < r.whi; w += lpf) istft_store(xb, w - a.t0, zero, a.vec);   // no frame, or past the last one
    }
}

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
    istft_cmfft_spans(a);
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
    istft_cmfft_spans(a);
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
