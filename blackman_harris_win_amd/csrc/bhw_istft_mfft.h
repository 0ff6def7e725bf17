// bhw_istft_mfft.h -- the span walk, the inverse passes, the ring and the flush shared by the kernels that end in a mixed-radix inverse
// real FFT, the window and the overlap-add: bhw_istft_mfft.hip (the frames are spectrum rows in memory) and bhw_mask_mfft.hip (the
// frames are formed from a signal and a gain row: DESIGN.md section 42).  The function is a template on the frame source -- where the
// pre-split points Z of a frame come from -- and everything after them is one text for both.  The account of what a slot does is in
// bhw_istft_mfft.hip.
//
// ImfIstftBins, the source of bhw_istft_mfft_f32_*, is a tag: its text (the load of Y[k] and Y[M - k] and the pre-split) stands in
// the function itself under `if constexpr`, where it stood before the function was shared, as IstftBins' does in bhw_istft_fft.h and
// for the same reason.  Any other source is an object with kTables, kMaxCpl, tables() and frame() on the terms bhw_istft_fft.h
// states (a is an ImfftIo here, and the ring keeps Source::kMaxCpl positions per lane).
#pragma once
#include "bhw_istft.h"
#include "bhw_stft_mfft.h"

namespace {

struct ImfftIo {
    const float *Y;
    float *x;
    uint64_t batch, frames, hop, samples, t0;
    uint64_t x_stride, y_stride, y_bstride;
    uint64_t span, spans, groups, trips;
    uint32_t n_fft, m, col0, len;
    uint32_t lpf, fy, cpl, passes;
    uint32_t sched;                       // the radix of pass p in bits 4p .. 4p + 3
    uint32_t shift, normalize;
};

struct ImfIstftBins {
    static constexpr bool kBins = true;
    static constexpr uint32_t kTables = 1;
    static constexpr uint32_t kMaxCpl = kFftMaxCpl;
};

// X[q] = sum over j of a[j] exp(+2 pi i j q / R), in place: the forward's butterflies conjugated
template <uint32_t R>
__device__ __forceinline__ void imf_butterfly(fft_v2f (&a)[R])
{
    if constexpr (R == 2) {
        const fft_v2f a0 = a[0], a1 = a[1];
        a[0] = a0 + a1;
        a[1] = a0 - a1;
    } else if constexpr (R == 3) {
        const fft_v2f t1 = a[1] + a[2], d = a[1] - a[2];
        const fft_v2f t2 = a[0] - 0.5f * t1, t3 = kSin3 * d;
        a[0] = a[0] + t1;
        a[1] = fft_v2f{t2.x - t3.y, t2.y + t3.x};                  // t2 + i t3
        a[2] = fft_v2f{t2.x + t3.y, t2.y - t3.x};                  // t2 - i t3
    } else if constexpr (R == 4) {
        const fft_v2f t0 = a[0] + a[2], t1 = a[0] - a[2], t2 = a[1] + a[3];
        const fft_v2f t3 = fft_v2f{a[3].y - a[1].y, a[1].x - a[3].x};   // +i (a1 - a3)
        a[0] = t0 + t2;
        a[1] = t1 + t3;
        a[2] = t0 - t2;
        a[3] = t1 - t3;
    } else {
        static_assert(R == 5, "radix");
        const fft_v2f b1 = a[1] + a[4], b2 = a[2] + a[3], d1 = a[1] - a[4], d2 = a[2] - a[3];
        const fft_v2f m1 = a[0] + kCos5a * b1 + kCos5b * b2, m2 = a[0] + kCos5b * b1 + kCos5a * b2;
        const fft_v2f n1 = kSin5a * d1 + kSin5b * d2, n2 = kSin5b * d1 - kSin5a * d2;
        a[0] = a[0] + b1 + b2;
        a[1] = fft_v2f{m1.x - n1.y, m1.y + n1.x};                  // m1 + i n1
        a[4] = fft_v2f{m1.x + n1.y, m1.y - n1.x};
        a[2] = fft_v2f{m2.x - n2.y, m2.y + n2.x};                  // m2 + i n2
        a[3] = fft_v2f{m2.x + n2.y, m2.y - n2.x};
    }
}

// One Stockham pass of radix R over the slot's M points: Q = M / R butterflies, sub-transform length Ns, ts = n_fft / (R Ns).
template <uint32_t R>
__device__ __forceinline__ void imf_pass(const fft_v2f *src, fft_v2f *dst, const fft_v2f *tw, uint32_t M, uint32_t Q, uint32_t Ns, uint32_t ts,
                                         uint32_t l, uint32_t lpf)
{
    const float inv = __builtin_amdgcn_rcpf((float)Ns);
    for (uint32_t i = l; i < Q; i += lpf) {
        fft_v2f a[R];
#pragma unroll
        for (uint32_t q = 0; q < R; ++q) a[q] = src[i + q * Q];
        uint32_t k = i;                                                 // the last pass: Ns = Q
        if (Ns < Q) k = i - (uint32_t)(((float)i + 0.5f) * inv) * Ns;   // i mod Ns
        if (Ns > 1u) {
            const uint32_t kt = k * ts;
#pragma unroll
            for (uint32_t q = 1; q < R; ++q) a[q] = cmul(a[q], mfft_twiddle(tw, q * kt, M));
        }
        imf_butterfly<R>(a);
        const uint32_t o = (i - k) * R + k;
#pragma unroll
        for (uint32_t q = 0; q < R; ++q) dst[o + q * Ns] = a[q];
    }
}

// Everything after the prologue's coefficients: vS (behind the twiddles) holds v[0..L).
template <class Source>
__device__ __forceinline__ void istft_mfft_spans(const ImfftIo &a, const Source &source)
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
    const float scale = (float)(1.0 / (double)n);                        // not a power of two: the multiply rounds
    const uint64_t pool = a.batch * a.spans, hop = a.hop;
    const uint32_t H = M >> 1;                                           // floor(M / 2)
    const uint32_t hm = (uint32_t)(hop % (uint64_t)n);
    // bit c of cols: the lane has a ring position c (c * lpf + l < n_fft: the last one may be missing)
    uint32_t cols = 0;
#pragma unroll
    for (uint32_t c = 0; c < Source::kMaxCpl; ++c)
        if (c < a.cpl && c * lpf + l < n) cols |= 1u << c;
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
        uint32_t bm = (uint32_t)((r.f_lo * hop) % (uint64_t)n);          // (f * hop) mod n_fft of the round's frame, stepped below
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
                            if (2u * k != M) {                               // the partner M - k: W[M - k] = -conj W[k]
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
            // 2. the passes (every slot, idle ones on stale data: their result is not read): Ns the product of the radices so far,
            //    rest = M / (Ns * r) after this pass, so n_fft / (r Ns) = 2 * rest
            uint32_t Ns = 1, rest = M;
            for (uint32_t p = 0; p < a.passes; ++p) {
                const uint32_t rdx = (a.sched >> (4u * p)) & 15u;
                if (rdx == 5u) {
                    rest /= 5u;
                    imf_pass<5>(src, dst, tw, M, M / 5u, Ns, 2u * rest, l, lpf);
                } else if (rdx == 3u) {
                    rest /= 3u;
                    imf_pass<3>(src, dst, tw, M, M / 3u, Ns, 2u * rest, l, lpf);
                } else if (rdx == 4u) {
                    rest >>= 2;
                    imf_pass<4>(src, dst, tw, M, M >> 2, Ns, 2u * rest, l, lpf);
                } else {
                    rest >>= 1;
                    imf_pass<2>(src, dst, tw, M, M >> 1, Ns, 2u * rest, l, lpf);
                }
                __syncthreads();
                fft_v2f *sw = src;
                src = dst;
                dst = sw;
                Ns *= rdx;
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
#pragma unroll
                for (uint32_t c = 0; c < Source::kMaxCpl; ++c) {
                    if ((cols >> c) & 1u) {
                        const uint32_t q = c * lpf + l;
                        const uint32_t k = q >= bm ? q - bm : q + n - bm;
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
            bm += hm;                                                    // ((f + 1) * hop) mod n_fft: both terms are below n_fft
            if (bm >= n) bm -= n;
            __syncthreads();                                             // the next round overwrites both buffers
        }
        if (live)
            for (uint64_t w = cur + l; w < r.whi; w += lpf) xb[w - a.t0] = 0.0f;   // a span with no frame, or outputs past the last one
    }
}

} // namespace
