// bhw_istft_cfft.h -- the span walk, the inverse passes, the ring and the flush shared by the kernels that end in a power-of-two inverse
// complex FFT, the window and the overlap-add for I/Q output: bhw_istft_cfft.hip (the frames are spectrum rows in memory) and
// bhw_mask_cfft.hip (the frames are formed from an I/Q signal and a gain row: DESIGN.md section 44).  The function is a template on
// the frame source -- where the n bins of a frame come from -- and everything after them is one text for both.  The account of what
// a slot does is in bhw_istft_cfft.hip.
//
// IstftCfftBins, the source of bhw_istft_cfft_f32_*, is a tag: its text (the load of the bins from column k or (k + n / 2) mod n)
// stands in the function itself under `if constexpr`, where it stood before the function was shared, as IstftBins' does in
// bhw_istft_fft.h and for the same reason.  Any other source is an object with
//   kTables        the twiddle tables it wants in LDS behind the Stockham buffers, n / 2 entries each: the inverse one, then its own;
//   tables(tw, k, cs, sn)   called in the table loop for entry k with cos and sin of 2 pi k / n, to fill its own tables at tw + n / 2;
//   frame(a, act, b, f, l, tw, vS, src, dst)   called by every lane of the workgroup for every trip (act: the slot has a frame f of
//                  signal b).  It may use both Stockham buffers of the slot and hold barriers that every lane reaches; it leaves the
//                  bins Y[0..n) in src, swapping src and dst if it must, and the function's barrier follows.
// A lane keeps kCfftMaxCpl ring positions whatever the source is.
#pragma once
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

struct IstftCfftBins {
    static constexpr bool kBins = true;
    static constexpr uint32_t kTables = 1;
};

// Everything after the prologue's coefficients: vS (behind the twiddles) holds v[0..L).
template <class Source>
__device__ __forceinline__ void istft_cfft_spans(const IcfftIo &a, const Source &source)
{
    const uint32_t n = a.n, H = n >> 1, Q = n >> 2, lpf = a.lpf, fy = a.fy, L = a.len;
    fft_v2f *bufA = (fft_v2f *)fft_lds;
    fft_v2f *bufB = bufA + (size_t)fy * n;
    fft_v2f *tw = bufB + (size_t)fy * n;
    const float *vS = (const float *)(tw + (size_t)Source::kTables * H);
    const uint32_t tid = threadIdx.x;
    const uint32_t slot = tid / lpf, l = tid - slot * lpf;
    for (uint32_t k = tid; k < H; k += kFftBlock) {
        double sn, cs;
        sincospi((double)k * 2.0 / (double)n, &sn, &cs);
        tw[k] = fft_v2f{(float)cs, (float)sn};
        if constexpr (!Source::kBins) source.tables(tw + H, k, cs, sn);
    }
    __syncthreads();
    const float scale = 1.0f / (float)n;                                 // a power of two: exact
    const uint64_t pool = a.batch * a.spans, hop = a.hop;
    [[maybe_unused]] const uint32_t turn = a.binshift ? H : 0u;
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
        [[maybe_unused]] const float *yb = a.Y + b * a.y_bstride;
        float *xb = a.x + b * a.x_stride;                                // output t = w - t0 (every w formed below is >= wlo >= t0)
        uint64_t cur = r.wlo;                                            // the span's outputs below cur are stored
        for (uint64_t it = 0; it < a.trips; ++it) {
            const uint64_t f = r.f_lo + it;
            const bool act = f < r.f_hi;
            // 1. the load, into the slot's row of buffer A
            fft_v2f *src = bufA + (size_t)slot * n, *dst = bufB + (size_t)slot * n;
            if constexpr (Source::kBins) {
                if (act) {
                    const fft_v2f *yp = (const fft_v2f *)(yb + f * a.y_stride);
#pragma unroll
                    for (uint32_t c = 0; c < kCfftMaxCpl; ++c) {
                        if (c < a.cpl) {
                            const uint32_t k = c * lpf + l;              // bin k sits in column k, or (k + n / 2) mod n
                            src[k] = yp[(k + turn) & (n - 1u)];
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

} // namespace
