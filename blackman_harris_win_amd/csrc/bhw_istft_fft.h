// bhw_istft_fft.h -- the span walk, the inverse passes, the ring and the flush shared by the kernels that end in a power-of-two inverse
// real FFT, the window and the overlap-add: bhw_istft_fft.hip (the frames are spectrum rows in memory) and bhw_mask_fft.hip (the
// frames are formed from a signal and a gain row: DESIGN.md section 41).  The function is a template on the frame source -- where the
// pre-split points Z of a frame come from -- and everything after them is one text for both.  The account of what a slot does is in
// bhw_istft_fft.hip.
//
// IstftBins, the source of bhw_istft_fft_f32_*, is a tag: its text (the load of Y[k] and Y[M - k] and the pre-split) stands in the
// function itself under `if constexpr`, where it stood before the function was shared, as FftStoreSpectrum's does in bhw_stft_fft.h
// and for the same reason.  Any other source is an object with
//   kTables        the twiddle tables it wants in LDS behind the Stockham buffers, M entries each: the inverse one, then its own;
//   kMaxCpl        the most columns per lane its n_fft give (the ring positions a lane keeps in registers);
//   tables(tw, k, cs, sn)   called in the table loop for entry k with cos and sin of 2 pi k / n_fft, to fill its own tables at tw + M;
//   frame(a, act, b, f, l, tw, vS, src, dst)   called by every lane of the workgroup for every trip (act: the slot has a frame f of
//                  signal b).  It may use both Stockham buffers of the slot and hold barriers that every lane reaches; it leaves the
//                  pre-split points Z[0..M) in src, swapping src and dst if it must, and the function's barrier follows.
#pragma once
#include "bhw_istft.h"

namespace {

struct IfftIo {
    const float *Y;
    float *x;
    uint64_t batch, frames, hop, samples, t0;
    uint64_t x_stride, y_stride, y_bstride;
    uint64_t span, spans, groups, trips;
    uint32_t n_fft, m, col0, len;
    uint32_t lpf, fy, cpl, radix4, radix2;
    uint32_t shift, normalize;
};

struct IstftBins {
    static constexpr bool kBins = true;
    static constexpr uint32_t kTables = 1;
    static constexpr uint32_t kMaxCpl = kFftMaxCpl;
};

// The pre-split of the bins A = Y[k], B = Y[M - k], 0 < k <= M / 2, with w = W[k] of the inverse table: Z[k], and Z[M - k] where
// k != M / 2, for a source that forms its bins in registers.  (Bin 0 is one line at both users.)  The pre-split text of IstftBins
// below leaves its roundings to the compiler's contraction, and what the compiler makes of that text depends on what stands around
// it: with the bins coming out of a multiply instead of a load it fused other products.  So the roundings k_istft_fft_* were compiled
// with are spelled out here, and nothing is left to contract: of the two products of each part of o = d * w the one by d.x is rounded
// and the one by d.y is fused into it; the adds of e are separate; the partner's o is o's with the sign of its imaginary part turned.
// tests/test_gpu_mask_fft.py holds the two texts to each other word for word.
__device__ __forceinline__ void istft_presplit(fft_v2f *z, uint32_t k, uint32_t M, fft_v2f A, fft_v2f B, fft_v2f w)
{
#pragma clang fp contract(off)
    const float ex = A.x + B.x, ey = A.y - B.y, dx = A.x - B.x, dy = A.y + B.y;
    const float ox = __builtin_fmaf(-dy, w.y, dx * w.x), oy = __builtin_fmaf(dy, w.x, dx * w.y);
    z[k] = fft_v2f{ex - oy, ey + ox};
    if (k != (M >> 1)) z[M - k] = fft_v2f{ex + oy, ox - ey};         // the partner M - k: W[M - k] = -conj W[k]
}

// Everything after the prologue's coefficients: vS (behind the twiddles) holds v[0..L).
template <class Source>
__device__ __forceinline__ void istft_fft_spans(const IfftIo &a, const Source &source)
{
    const uint32_t M = a.m, n = a.n_fft, lpf = a.lpf, fy = a.fy, L = a.len;
    fft_v2f *bufA = (fft_v2f *)fft_lds;
    fft_v2f *bufB = bufA + (size_t)fy * M;
    fft_v2f *tw = bufB + (size_t)fy * M;
    const float *vS = (const float *)(tw + (size_t)Source::kTables * M);
    const uint32_t tid = threadIdx.x;
    const uint32_t slot = tid / lpf, l = tid - slot * lpf;
    for (uint32_t k = tid; k < M; k += kFftBlock) {
        double sn, cs;
        sincospi((double)k * 2.0 / (double)n, &sn, &cs);
        tw[k] = fft_v2f{(float)cs, (float)sn};
        if constexpr (!Source::kBins) source.tables(tw + M, k, cs, sn);
    }
    __syncthreads();
    const float scale = 1.0f / (float)n;                                 // a power of two: exact
    const uint64_t pool = a.batch * a.spans, hop = a.hop;
    const uint32_t H = M >> 1, Q = M >> 2;
    double acc[Source::kMaxCpl], env[Source::kMaxCpl];
#pragma unroll
    for (uint32_t c = 0; c < Source::kMaxCpl; ++c) acc[c] = env[c] = 0.0;
    for (uint64_t g = blockIdx.x; g < a.groups; g += gridDim.x) {
        const uint64_t sp = g * fy + slot;
        const bool live = sp < pool;
        const uint64_t b = live ? sp / a.spans : 0, s = live ? sp - b * a.spans : 0;
        BhwIstftSpan r = bhwp_istft_span(s, a.span, hop, L, a.t0, a.samples, a.frames);
        if (!live) r.wlo = r.whi = r.f_lo = r.f_hi = 0;
        [[maybe_unused]] const float *yb = a.Y + b * a.y_bstride;
        float *xb = a.x + b * a.x_stride;                                // output t = w - t0 (every w formed below is >= wlo >= t0)
        uint64_t cur = r.wlo;                                            // the span's outputs below cur are stored
        for (uint64_t it = 0; it < a.trips; ++it) {
            const uint64_t f = r.f_lo + it;
            const bool act = f < r.f_hi;
            // 1. the pre-split, into the slot's half of buffer A
            fft_v2f *src = bufA + (size_t)slot * M, *dst = bufB + (size_t)slot * M;
            if constexpr (Source::kBins) {
                if (act) {
                    const fft_v2f *yp = (const fft_v2f *)(yb + f * a.y_stride);
                    for (uint32_t k = l; k <= H; k += lpf) {
                        const fft_v2f A = yp[k], B = yp[M - k];
                        if (k == 0u) {
                            src[0] = fft_v2f{A.x + B.x, A.x - B.x};
                        } else {
                            const fft_v2f w = tw[k];
                            const fft_v2f e0 = fft_v2f{A.x + B.x, A.y - B.y}, d0 = fft_v2f{A.x - B.x, A.y + B.y};
                            const fft_v2f o0 = cmul(d0, w);
                            src[k] = fft_v2f{e0.x - o0.y, e0.y + o0.x};
                            if (k != H) {                                    // the partner M - k: W[M - k] = -conj W[k]
                                const fft_v2f e1 = fft_v2f{e0.x, -e0.y}, d1 = fft_v2f{-d0.x, d0.y};
                                const fft_v2f o1 = cmul(d1, fft_v2f{-w.x, w.y});
                                src[M - k] = fft_v2f{e1.x - o1.y, e1.y + o1.x};
                            }
                        }
                    }
                }
            } else {
                source.frame(a, act, b, f, l, tw, vS, src, dst);
            }
            __syncthreads();
            // 2. the passes (every slot, idle ones on stale data: their result is not read)
            uint32_t Ns = 1;
            for (uint32_t p = 0; p < a.radix4; ++p) {
                const uint32_t ts = M / (2u * Ns);                       // n_fft / (4 Ns)
                for (uint32_t i = l; i < Q; i += lpf) {
                    const uint32_t k = i & (Ns - 1u);
                    fft_v2f a0 = src[i], a1 = src[i + Q], a2 = src[i + 2u * Q], a3 = src[i + 3u * Q];
                    if (Ns > 1u) {
                        const uint32_t kt = k * ts;
                        a1 = cmul(a1, twiddle(tw, kt, M));
                        a2 = cmul(a2, twiddle(tw, 2u * kt, M));
                        a3 = cmul(a3, twiddle(tw, 3u * kt, M));
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
            if (a.radix2) {                                              // Ns = M / 2: k = i, twiddle W[2 i]
                for (uint32_t i = l; i < H; i += lpf) {
                    const fft_v2f a0 = src[i], a1 = cmul(src[i + H], tw[2u * i]);
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
                const float *row = (const float *)src + a.col0;
                const uint64_t base = f * hop;
                if (cur < base) {                                        // a gap no frame reaches (hop > L, or the span's start)
                    for (uint64_t w = cur + l; w < base; w += lpf) xb[w - a.t0] = 0.0f;
                    cur = base;
                }
                uint64_t end = (f + 1 == r.f_hi || base + hop > r.whi) ? r.whi : base + hop;
                if (end < cur) end = cur;                                // a halo frame whose own hop lies before the span
                const uint32_t bm = (uint32_t)(base & (uint64_t)(n - 1u));
#pragma unroll
                for (uint32_t c = 0; c < Source::kMaxCpl; ++c) {
                    if (c < a.cpl) {
                        const uint32_t k = (c * lpf + l - bm) & (n - 1u);
                        const uint64_t w = base + k;
                        if (k < L && w >= cur && w < r.whi) {
                            const double v = (double)vS[k];
                            acc[c] += (double)(row[k] * scale) * v;
                            env[c] += v * v;
                            if (w < end) {
                                xb[w - a.t0] = istft_out(acc[c], env[c], a.normalize);
                                acc[c] = env[c] = 0.0;
                            }
                        }
                    }
                }
                const uint64_t reach = base + L;                         // the frame's extent: beyond it up to `end` nothing is summed
                if (reach < end)
                    for (uint64_t w = (reach > cur ? reach : cur) + l; w < end; w += lpf) xb[w - a.t0] = 0.0f;
                cur = end;
            }
            __syncthreads();                                             // the next round overwrites both buffers
        }
        if (live)
            for (uint64_t w = cur + l; w < r.whi; w += lpf) xb[w - a.t0] = 0.0f;   // a span with no frame, or outputs past the last one
    }
}

} // namespace
