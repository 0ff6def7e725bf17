// bhw_istft_cmfft.h -- the span walk, the passes, the ring and the flush shared by the kernels that end in a mixed-radix inverse
// complex FFT, the window and the overlap-add for I/Q output: bhw_istft_cmfft.hip (the frames are spectrum rows in memory) and
// bhw_mask_cmfft.hip (the frames are formed from an I/Q signal and a gain row: DESIGN.md section 44).  The function is a template on
// the frame source -- where the n bins of a frame come from -- and everything after them is one text for both.  The account of what
// a slot does is in bhw_istft_cmfft.hip.
//
// IstftCmfftBins, the source of bhw_istft_cmfft_f32_*, is a tag: its text (the load of the bins from column k or (k + n / 2) mod n,
// stored with the parts swapped) stands in the function itself under `if constexpr`, where it stood before the function was shared,
// as IstftBins' does in bhw_istft_fft.h and for the same reason.  Any other source is an object with
//   frame(a, act, b, f, l, tw, vS, src, dst)   called by every lane of the workgroup for every trip (act: the slot has a frame f of
//                  signal b).  It may use both Stockham buffers of the slot and hold barriers that every lane reaches; it leaves the
//                  bins Y[0..n), PARTS SWAPPED, in src, swapping src and dst if it must, and the function's barrier follows.
// One twiddle table serves every source: the inverse runs the forward passes over the forward table.
#pragma once
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

struct IstftCmfftBins {
    static constexpr bool kBins = true;
};

// Everything after the prologue's coefficients: vS (behind the twiddles) holds v[0..L).
template <class Source>
__device__ __forceinline__ void istft_cmfft_spans(const IcmfftIo &a, const Source &source)
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
    [[maybe_unused]] const uint32_t turn = a.binshift ? n >> 1 : 0u;
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
        [[maybe_unused]] const float *yb = a.Y + b * a.y_bstride;
        float *xb = a.x + b * a.x_stride;                                // output t = w - t0 (every w formed below is >= wlo >= t0)
        uint64_t cur = r.wlo;                                            // the span's outputs below cur are stored
        uint32_t bm = (uint32_t)((r.f_lo * hop) % (uint64_t)n);          // (f * hop) mod n of the round's frame, stepped below
        for (uint64_t it = 0; it < a.trips; ++it) {
            const uint64_t f = r.f_lo + it;
            const bool act = f < r.f_hi;
            // 1. the load, parts swapped, into the slot's row of buffer A
            fft_v2f *src = bufA + (size_t)slot * n, *dst = bufB + (size_t)slot * n;
            if constexpr (Source::kBins) {
                if (act) {
                    const fft_v2f *yp = (const fft_v2f *)(yb + f * a.y_stride);
#pragma unroll
                    for (uint32_t c = 0; c < kCfftMaxCpl; ++c) {
                        if ((cols >> c) & 1u) {
                            const uint32_t k = c * lpf + l;              // bin k sits in column k, or (k + n / 2) mod n
                            uint32_t col = k + turn;
                            col = col >= n ? col - n : col;
                            const fft_v2f y = yp[col];
                            src[k] = fft_v2f{y.y, y.x};
                        }
                    }
                }
            } else {
                source.frame(a, act, b, f, l, tw, vS, src, dst);
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

} // namespace
