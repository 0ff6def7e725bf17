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
// Kept in step by hand: the span walk, the ring and the flush stand in all four inverse units (bhw_istft_fft.hip,
// bhw_istft_mfft.hip, this one, bhw_istft_cmfft.hip), and tests/cpp/san_istft_cfft.cpp replays this file's index arithmetic -- the
// load's point index, the pass indices, the ring's (q - base) mod n and the flush bound `end` -- from a copy of its own, since only
// bhwp_istft_span is shared through bhw_plan.h.  An edit of any of these here is an edit of the siblings and of the replay too.
// cmul, twiddle and the dynamic LDS array are bhw_stft_fft.h's, the Io fill, istft_out and istft_store bhw_istft.h's.
#include "bhw_istft.h"

namespace {

struct IcfftIo {
    const float *Y;
    float *x;
    uint64_t batch, frames, hop, samples, t0;
    uint64_t x_stride, y_stride, y_bstride;
    uint64_t span, spans, groups, trips;
    uint32_t n, col0, len;
    uint32_t lpf, fy, cpl, radix4, radix2;
    uint32_t shift, normalize, binshift, vec;
};

// Everything after the prologue's coefficients: vS (behind the twiddles) holds v[0..L).
__device__ __forceinline__ void istft_cfft_spans(const IcfftIo &a)
{
    const uint32_t n = a.n, H = n >> 1, Q = n >> 2, lpf = a.lpf, fy = a.fy, L = a.len;
    fft_v2f *bufA = (fft_v2f *)fft_lds;
    fft_v2f *bufB = bufA + (size_t)fy * n;
    fft_v2f *tw = bufB + (size_t)fy * n;
    const float *vS = (const float *)(tw + H);
    const uint32_t tid = threadIdx.x;
    const uint32_t slot = tid / lpf, l = tid - slot * lpf;
    for (uint32_t k = tid; k < H; k += kFftBlock) {
        double sn, cs;
        sincospi((double)k * 2.0 / (double)n, &sn, &cs);
        tw[k] = fft_v2f{(float)cs, (float)sn};
    }
    __syncthreads();
    const float scale = 1.0f / (float)n;                                 // a power of two: exact
    const uint64_t pool = a.batch * a.spans, hop = a.hop;
    const uint32_t turn = a.binshift ? H : 0u;
    const fft_v2f zero = fft_v2f{0.0f, 0.0f};
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
        for (uint64_t it = 0; it < a.trips; ++it) {
            const uint64_t f = r.f_lo + it;
            const bool act = f < r.f_hi;
            // 1. the load, into the slot's row of buffer A
            fft_v2f *src = bufA + (size_t)slot * n, *dst = bufB + (size_t)slot * n;
            if (act) {
                const fft_v2f *yp = (const fft_v2f *)(yb + f * a.y_stride);
#pragma unroll
                for (uint32_t c = 0; c < kCfftMaxCpl; ++c) {
                    if (c < a.cpl) {
                        const uint32_t k = c * lpf + l;                  // bin k sits in column k, or (k + n / 2) mod n
                        src[k] = yp[(k + turn) & (n - 1u)];
                    }
                }
            }
            __syncthreads();
            // 2. the passes (every slot, idle ones on stale data: their result is not read)
            uint32_t Ns = 1;
            for (uint32_t p = 0; p < a.radix4; ++p) {
                const uint32_t ts = n / (4u * Ns);
                for (uint32_t i = l; i < Q; i += lpf) {
                    const uint32_t k = i & (Ns - 1u);
                    fft_v2f a0 = src[i], a1 = src[i + Q], a2 = src[i + 2u * Q], a3 = src[i + 3u * Q];
                    if (Ns > 1u) {
                        const uint32_t kt = k * ts;
                        a1 = cmul(a1, twiddle(tw, kt, H));
                        a2 = cmul(a2, twiddle(tw, 2u * kt, H));
                        a3 = cmul(a3, twiddle(tw, 3u * kt, H));
                    }
                    const fft_v2f t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3;
                    const fft_v2f t3 = fft_v2f{a3.y - a1.y, a1.x - a3.x};   // +i (a1 - a3)
                    const uint32_t o = ((i - k) << 2) + k;
                    dst[o] = t0 + t2;
                    dst[o + Ns] = t1 + t3;
                    dst[o + 2u * Ns] = t0 - t2;
                    dst[o + 3u * Ns] = t1 - t3;
                }
                __syncthreads();
                fft_v2f *sw = src;
                src = dst;
                dst = sw;
                Ns <<= 2;
            }
            if (a.radix2) {                                              // Ns = n / 2: k = i, twiddle W[i]
                for (uint32_t i = l; i < H; i += lpf) {
                    const fft_v2f a0 = src[i], a1 = cmul(src[i + H], tw[i]);
                    dst[i] = a0 + a1;
                    dst[i + H] = a0 - a1;
                }
                __syncthreads();
                fft_v2f *sw = src;
                src = dst;
                dst = sw;
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
                const uint32_t bm = (uint32_t)(base & (uint64_t)(n - 1u));
#pragma unroll
                for (uint32_t c = 0; c < kCfftMaxCpl; ++c) {
                    if (c < a.cpl) {
                        const uint32_t k = (c * lpf + l - bm) & (n - 1u);
                        const uint64_t w = base + k;
                        if (k < L && w >= cur && w < r.whi) {
                            const double v = (double)vS[k];
                            const fft_v2f z = row[k];
                            accr[c] += (double)(z.x * scale) * v;
                            acci[c] += (double)(z.y * scale) * v;
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
            __syncthreads();                                             // the next round overwrites both buffers
        }
        if (live)
            for (uint64_t w = cur + l; w < r.whi; w += lpf) istft_store(xb, w - a.t0, zero, a.vec);   // no frame, or past the last one
    }
}

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
    istft_cfft_spans(a);
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
    istft_cfft_spans(a);
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
