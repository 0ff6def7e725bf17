// bhw_stft_cfft.h -- the body shared by the kernels that form a windowed row of interleaved I/Q samples and transform it in LDS:
// bhw_stft_cfft.hip (stores the spectrum row or its powers) and bhw_welch_cfft.hip (adds the powers over the frames of a run:
// DESIGN.md section 27).  The row function is a template on the epilogue -- what happens to the transformed row -- and everything
// before it is one text for both units.  Moving the body here left the instruction streams of k_stft_cfft_direct<*> and
// k_stft_cfft_table<*> unchanged.  The forward kernels of bhw_stft_fft.h are not touched: cmul, twiddle and
// the launch helper are restated here, as bhw_istft_fft.hip does.
//
// A workgroup owns whole rows of n = n_fft complex points.  Prologue, once per workgroup: the window coefficients v[0..n) (+0.0
// outside the window) by the direct CORDIC chains or the gather over a resident table, staged through LDS so that every lane ends
// with the cpl coefficients of its own columns in registers; and the twiddle table W[k] = exp(-2 pi i k / n), k < n / 2, each
// component the float32 rounding of a binary64 sincospi.  Then, for each group of fy rows the workgroup takes:
//   1. a lane loads the complex samples of its columns c * lpf + lane (consecutive lanes, consecutive complex64 values; one 8-byte
//      load where the base and the signal stride allow it, else two 4-byte ones), with the padding rule of bhw_stft.h; with
//      detrending the raw row goes to LDS, one wave per row sums both channels in the contract's order (64 binary64 partial sums by
//      j mod 64 in ascending j, the butterfly 32 ... 1) and leaves m_c = fl32(S_c / L), two means per slot, in LDS;
//   2. row[j] = (fl32(xr * v), fl32(xi * v)) or (fl32(fl32(xr - m_0) * v), fl32(fl32(xi - m_1) * v)), +0.0 outside the window, goes
//      to LDS as n complex points;
//   3. a Stockham FFT of n points, out of place between two LDS buffers: radix-4 passes (the first without twiddles), one radix-2
//      pass at the end when log2 n is odd.  Butterfly i of a pass at sub-transform length Ns reads z[i + q * n / 4], multiplies by W
//      at q * k * n / (4 Ns), k = i mod Ns, read from the table (never a product of twiddles), and writes (i - k) * 4 + k + q * Ns;
//   4. the epilogue.  CfftStore: lane l writes bins l, l + lpf, ... as complex64 or as fl32(re^2 + im^2) in binary64, to column k
//      or, shifted, to column (k + n / 2) mod n: consecutive lanes, consecutive elements, plain stores.
// A row's arithmetic does not depend on its slot, its group or the grid: the bits of an output row are a function of the row alone.
#pragma once
#include "bhw_device.h"

namespace {

typedef float cfft_v2f __attribute__((ext_vector_type(2)));

struct CfftIo {
    const float *x;
    float *Y;
    uint64_t rows, frames, hop, samples, pad;
    uint64_t x_stride, y_stride, y_bstride;
    uint64_t groups;
    uint32_t n, col0, len;
    uint32_t lpf, fy, cpl, radix4, radix2;
    uint32_t shift, reflect, detrend;
    uint32_t power, binshift, vec;
};

// The Io of a launch from the plan and the descriptor; the Welch and hold plans carry zero y strides and power false.
inline CfftIo cfft_io(const BhwStftCfftPlan &pl, const bhw_stft *s, const float *d_x, float *d_Y)
{
    CfftIo a;
    a.x = d_x;
    a.Y = d_Y;
    a.rows = pl.rows;
    a.frames = s->frames;
    a.hop = s->hop;
    a.samples = s->samples;
    a.pad = s->pad;
    a.x_stride = pl.x_stride;
    a.y_stride = pl.y_stride;
    a.y_bstride = pl.y_bstride;
    a.groups = pl.groups;
    a.n = pl.n;
    a.col0 = (uint32_t)s->col0;
    a.len = (uint32_t)pl.len;
    a.lpf = pl.lpf;
    a.fy = pl.fy;
    a.cpl = pl.cpl;
    a.radix4 = pl.radix4;
    a.radix2 = pl.radix2;
    a.shift = s->shift;
    a.reflect = s->pad_mode == BHW_PAD_REFLECT ? 1u : 0u;
    a.detrend = pl.detrend ? 1u : 0u;
    a.power = pl.power ? 1u : 0u;
    a.binshift = pl.shifted ? 1u : 0u;
    a.vec = iq_vec(d_x, s->batch, pl.x_stride);
    return a;
}

extern __shared__ __attribute__((aligned(16))) unsigned char cfft_lds[];

__device__ __forceinline__ cfft_v2f cmul(cfft_v2f a, cfft_v2f w) { return cfft_v2f{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }

// W at index idx < n (table of h = n / 2 entries, W[idx + h] = -W[idx])
__device__ __forceinline__ cfft_v2f twiddle(const cfft_v2f *tw, uint32_t idx, uint32_t h)
{
    const cfft_v2f w = tw[idx & (h - 1u)];
    return (idx & h) ? cfft_v2f{-w.x, -w.y} : w;
}

// What happens to a transformed row is the epilogue, a template parameter of the row function.  CfftStore, the epilogue of
// bhw_stft_cfft_f32_*, is a tag: its text (consecutive lanes writing consecutive bins of the output row) stands in the row function
// itself under `if constexpr`, where it stood before the function was shared, so that the compiled forward kernels keep their
// registers (the reason bhw_stft_fft.h gives for FftStoreSpectrum).
//
// An epilogue with kRuns true owns RUNS instead of strided groups of the flat row pool (bhw_welch_cfft.hip): the frame axis of every
// signal is padded to epilogue.fpad frames, a run is epilogue.gpr (a power of two) consecutive groups of one signal, workgroup w
// takes the runs w, w + grid, ... and a run's groups in ascending order; a row with f >= frames is not live.  It is called once per
// group by every lane as epilogue(a, g, b, f0, base): the group, its signal, the frame of slot 0 and the transformed points of slot 0
// (slot s at base + s * n).  Such an epilogue may carry state from group to group in `mutable` members, on the terms bhw_stft_fft.h
// states for the real kernel: one object per lane lives for the whole group loop, and the calls of a run's groups come in ascending
// order with nothing of another run between them.
struct CfftStore {
    static constexpr bool kStore = true;
    static constexpr bool kRuns = false;
};

template <class E>
__device__ __forceinline__ uint64_t cfft_first_group(const E &e)
{
    if constexpr (E::kRuns) return (uint64_t)blockIdx.x * e.gpr;
    else                    return blockIdx.x;
}

template <class E>
__device__ __forceinline__ uint64_t cfft_next_group(const E &e, uint64_t g)
{
    if constexpr (E::kRuns) return ((g + 1u) & (e.gpr - 1u)) ? g + 1u : g + 1u + (uint64_t)(gridDim.x - 1u) * e.gpr;
    else                    return g + gridDim.x;
}

// Everything after the prologue's coefficients: vbuf = buffer A viewed as floats holds v[0..n).
template <class Epilogue>
__device__ __forceinline__ void stft_cfft_rows(const CfftIo &a, const Epilogue &epilogue)
{
    const uint32_t n = a.n, H = n >> 1, lpf = a.lpf, fy = a.fy;
    cfft_v2f *bufA = (cfft_v2f *)cfft_lds;
    cfft_v2f *bufB = bufA + (size_t)fy * n;
    cfft_v2f *tw = bufB + (size_t)fy * n;
    float *mean_s = (float *)(tw + H);
    const uint32_t tid = threadIdx.x;
    const uint32_t slot = tid / lpf, l = tid - slot * lpf;
    // the twiddle table
    for (uint32_t k = tid; k < H; k += kFftBlock) {
        double sn, cs;
        sincospi((double)k * 2.0 / (double)n, &sn, &cs);
        tw[k] = cfft_v2f{(float)cs, (float)-sn};
    }
    // the lane's coefficients
    float v[kCfftMaxCpl];
    {
        const float *vbuf = (const float *)bufA;
#pragma unroll
        for (uint32_t c = 0; c < kCfftMaxCpl; ++c) v[c] = c < a.cpl ? vbuf[c * lpf + l] : 0.0f;
    }
    __syncthreads();
    const uint32_t wave = tid >> 6, lane = tid & 63u;
    const uint64_t T = a.samples;
    // bit c of cols: the lane has a column c; of wins: that column is a window column
    uint32_t cols = 0, wins = 0;
#pragma unroll
    for (uint32_t c = 0; c < kCfftMaxCpl; ++c) {
        if (c < a.cpl) {
            cols |= 1u << c;
            if (c * lpf + l - a.col0 < a.len) wins |= 1u << c;        // unsigned: a window column
        }
    }
    cfft_v2f *rowA = bufA + (size_t)slot * n;                          // the slot's row
    for (uint64_t g = cfft_first_group(epilogue); g < a.groups; g = cfft_next_group(epilogue, g)) {
        bool live;
        uint64_t b, f;
        [[maybe_unused]] uint64_t f0 = 0;
        if constexpr (Epilogue::kRuns) {
            const uint64_t r0 = g * fy;                                // fpad is a multiple of fy: a group never crosses a signal
            b = r0 / epilogue.fpad;
            f0 = r0 - b * epilogue.fpad;
            live = f0 + slot < a.frames;
            f = live ? f0 + slot : 0;
        } else {
            const uint64_t r = g * fy + slot;
            live = r < a.rows;
            b = live ? r / a.frames : 0;
            f = live ? r - b * a.frames : 0;
        }
        const float *xb = a.x + b * a.x_stride;
        const uint64_t t0 = f * a.hop + l - a.pad;                     // the (wrapped) time of column l
        asm volatile("" : "+v"(cols), "+v"(wins));
        const uint32_t take = live ? wins : 0u;
        cfft_v2f e[kCfftMaxCpl];
#pragma unroll
        for (uint32_t c = 0; c < kCfftMaxCpl; ++c) {
            e[c] = cfft_v2f{0.0f, 0.0f};
            if ((take >> c) & 1u) {
                uint64_t t = t0 + c * lpf;                             // unsigned: t < T is the whole interior test
                bool zero = false;
                if (t >= T) {
                    const int64_t ts = (int64_t)t;
                    if (a.reflect) t = ts < 0 ? (uint64_t)(-ts) : 2 * (T - 1) - t;
                    else {
                        t = 0;
                        zero = true;
                    }
                }
                const float *px = xb + 2 * t;
                cfft_v2f xv;
                if (a.vec) xv = *(const cfft_v2f *)px;
                else       xv = cfft_v2f{px[0], px[1]};
                e[c] = zero ? cfft_v2f{0.0f, 0.0f} : xv;
            }
        }
        if (a.detrend) {
            // the raw row (col0 0: column j is sample j), then one wave per row and both channels: the order of k_welch_mean
#pragma unroll
            for (uint32_t c = 0; c < kCfftMaxCpl; ++c)
                if ((cols >> c) & 1u) rowA[c * lpf + l] = e[c];
            __syncthreads();
            for (uint32_t s = wave; s < fy; s += kFftBlock / 64u) {
                const cfft_v2f *row = bufA + (size_t)s * n;
                double P0 = 0.0, P1 = 0.0;
                for (uint32_t j = lane; j < a.len; j += 64u) {
                    const cfft_v2f z = row[j];
                    P0 += (double)z.x;
                    P1 += (double)z.y;
                }
#pragma unroll
                for (int sh = 32; sh >= 1; sh >>= 1) {
                    P0 += __shfl_down(P0, sh, 64);
                    P1 += __shfl_down(P1, sh, 64);
                }
                if (lane == 0) {
                    mean_s[2u * s] = (float)(P0 / (double)a.len);
                    mean_s[2u * s + 1u] = (float)(P1 / (double)a.len);
                }
            }
            __syncthreads();
            const float mu0 = mean_s[2u * slot], mu1 = mean_s[2u * slot + 1u];
#pragma unroll
            for (uint32_t c = 0; c < kCfftMaxCpl; ++c)
                if ((cols >> c) & 1u) {
                    const float d0 = e[c].x - mu0, d1 = e[c].y - mu1;
                    rowA[c * lpf + l] = ((take >> c) & 1u) ? cfft_v2f{d0 * v[c], d1 * v[c]} : cfft_v2f{0.0f, 0.0f};
                }
        } else {
#pragma unroll
            for (uint32_t c = 0; c < kCfftMaxCpl; ++c)
                if ((cols >> c) & 1u) rowA[c * lpf + l] = ((take >> c) & 1u) ? cfft_v2f{e[c].x * v[c], e[c].y * v[c]} : cfft_v2f{0.0f, 0.0f};
        }
        __syncthreads();
        // the passes
        cfft_v2f *src = rowA, *dst = bufB + (size_t)slot * n;
        uint32_t Ns = 1;
        const uint32_t Q = n >> 2;
        for (uint32_t p = 0; p < a.radix4; ++p) {
            const uint32_t ts = n / (4u * Ns);
            for (uint32_t i = l; i < Q; i += lpf) {
                const uint32_t k = i & (Ns - 1u);
                cfft_v2f a0 = src[i], a1 = src[i + Q], a2 = src[i + 2u * Q], a3 = src[i + 3u * Q];
                if (Ns > 1u) {
                    const uint32_t kt = k * ts;
                    a1 = cmul(a1, twiddle(tw, kt, H));
                    a2 = cmul(a2, twiddle(tw, 2u * kt, H));
                    a3 = cmul(a3, twiddle(tw, 3u * kt, H));
                }
                const cfft_v2f t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3;
                const cfft_v2f t3 = cfft_v2f{a1.y - a3.y, a3.x - a1.x};   // -i (a1 - a3)
                const uint32_t o = ((i - k) << 2) + k;
                dst[o] = t0 + t2;
                dst[o + Ns] = t1 + t3;
                dst[o + 2u * Ns] = t0 - t2;
                dst[o + 3u * Ns] = t1 - t3;
            }
            __syncthreads();
            cfft_v2f *sw = src;
            src = dst;
            dst = sw;
            Ns <<= 2;
        }
        if (a.radix2) {                                                 // Ns = n / 2: k = i, twiddle W[i]
            for (uint32_t i = l; i < H; i += lpf) {
                const cfft_v2f a0 = src[i], a1 = cmul(src[i + H], tw[i]);
                dst[i] = a0 + a1;
                dst[i + H] = a0 - a1;
            }
            __syncthreads();
            cfft_v2f *sw = src;
            src = dst;
            dst = sw;
        }
        if constexpr (Epilogue::kStore) {
            // the store: bin k to column k, or to (k + n / 2) mod n
            if (live) {
                float *yrow = a.Y + b * a.y_bstride + f * a.y_stride;
                const uint32_t turn = a.binshift ? H : 0u;
                if (a.power) {
                    for (uint32_t k = l; k < n; k += lpf) {
                        const cfft_v2f y = src[k];
                        yrow[(k + turn) & (n - 1u)] = (float)((double)y.x * (double)y.x + (double)y.y * (double)y.y);
                    }
                } else {
                    cfft_v2f *yp = (cfft_v2f *)yrow;
                    for (uint32_t k = l; k < n; k += lpf) yp[(k + turn) & (n - 1u)] = src[k];
                }
            }
        } else {
            epilogue(a, g, b, f0, src - (size_t)slot * n);
        }
        __syncthreads();                                                // the next group overwrites both buffers
    }
}

} // namespace
