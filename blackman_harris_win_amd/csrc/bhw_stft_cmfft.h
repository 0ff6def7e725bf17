// bhw_stft_cmfft.h -- the body of the kernels that form a windowed row of interleaved I/Q samples at n_fft = 2^a 3^b 5^c that is no
// power of two, odd lengths included, and transform it in LDS: bhw_stft_cmfft.hip (stores the spectrum row or its powers; DESIGN.md
// section 30).  The row function is a template on the epilogue -- what happens to the transformed row -- from the start, so that a
// frame-averaging epilogue can be added without touching this text, as bhw_stft_cfft.h and bhw_stft_mfft.h were shared later.
//
// It is the complex loader of bhw_stft_cfft.h in front of the passes of bhw_stft_mfft.h.  Neither header is edited: the passes
// (mfft_pass<R>, mfft_butterfly<R>, mfft_twiddle) are included and called, the loader is restated here with the cols mask of the
// mixed-radix kernel.  A workgroup owns whole rows of n = n_fft complex points.  Prologue, once per workgroup: the window
// coefficients v[0..n) (+0.0 outside the window) staged through LDS into the lane's registers, and the twiddle table
// W[k] = exp(-2 pi i k / n), k < fold, each component the float32 rounding of a binary64 sincospi; fold = n / 2 for an even n
// (W[k + n / 2] = -W[k], the compare of mfft_twiddle) and n for an odd one (no index reaches fold: the compare never fires).  Then,
// for each group of fy rows the workgroup takes:
//   1. a lane loads the complex samples of its columns c * lpf + lane < n (the last column of a lane need not exist), one 8-byte load
//      where the base and the signal stride allow it, else two 4-byte ones, with the padding rule of bhw_stft.h; with detrending the
//      raw row goes to LDS, one wave per row sums both channels in the contract's order and leaves two means per slot in LDS;
//   2. row[j] = (fl32(xr * v), fl32(xi * v)) or (fl32(fl32(xr - m_0) * v), fl32(fl32(xi - m_1) * v)), +0.0 outside the window;
//   3. the plan's schedule (5s, 3s, 4s, a last 2) over the n points, out of place between two LDS buffers: mfft_pass<R> called with
//      M = fold, Q = n / R and ts = n / (R Ns) is the pass of an n-point complex transform;
//   4. the epilogue.  CmfftStore: lane l writes bins l, l + lpf, ... as complex64 or as fl32(re^2 + im^2) in binary64, to column k
//      or, shifted, to column (k + n / 2) mod n (integer division; a compare and a subtract: n is no power of two): consecutive
//      lanes, consecutive elements, plain stores.
// A row's arithmetic does not depend on its slot, its group or the grid: the bits of an output row are a function of the row alone.
#pragma once
#include "bhw_stft_mfft.h"

namespace {

struct CmfftIo {
    const float *x;
    float *Y;
    uint64_t rows, frames, hop, samples, pad;
    uint64_t x_stride, y_stride, y_bstride;
    uint64_t groups;
    uint32_t n, fold, col0, len;
    uint32_t lpf, fy, cpl, passes;
    uint32_t sched;                       // the radix of pass p in bits 4p .. 4p + 3
    uint32_t shift, reflect, detrend;
    uint32_t power, binshift, vec;
};

// The Io of a launch from the plan and the descriptor; the Welch and hold plans carry zero y strides and power false.
inline CmfftIo cmfft_io(const BhwStftCmfftPlan &pl, const bhw_stft *s, const float *d_x, float *d_Y)
{
    CmfftIo a{};
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
    a.fold = pl.fold;
    a.col0 = (uint32_t)s->col0;
    a.len = (uint32_t)pl.len;
    a.lpf = pl.lpf;
    a.fy = pl.fy;
    a.cpl = pl.cpl;
    a.passes = pl.passes;
    for (uint32_t p = 0; p < pl.passes; ++p) a.sched |= (uint32_t)pl.radix[p] << (4u * p);
    a.shift = s->shift;
    a.reflect = s->pad_mode == BHW_PAD_REFLECT ? 1u : 0u;
    a.detrend = pl.detrend ? 1u : 0u;
    a.power = pl.power ? 1u : 0u;
    a.binshift = pl.shifted ? 1u : 0u;
    a.vec = iq_vec(d_x, s->batch, pl.x_stride);
    return a;
}

// What happens to a transformed row is the epilogue, a template parameter of the row function.  CmfftStore, the epilogue of
// bhw_stft_cmfft_f32_*, is a tag: its text stands in the row function itself under `if constexpr`, as in both parents.
//
// An epilogue with kRuns true owns RUNS instead of strided groups of the flat row pool, on the terms bhw_stft_cfft.h states: the
// frame axis of every signal is padded to epilogue.fpad frames, a run is epilogue.gpr (a power of two) consecutive groups of one
// signal, workgroup w takes the runs w, w + grid, ... and a run's groups in ascending order; a row with f >= frames is not live.  It
// is called once per group by every lane as epilogue(a, g, b, f0, base): the group, its signal, the frame of slot 0 and the
// transformed points of slot 0 (slot s at base + s * n).
struct CmfftStore {
    static constexpr bool kStore = true;
    static constexpr bool kRuns = false;
};

// Everything after the prologue's coefficients: vbuf = buffer A viewed as floats holds v[0..n).
template <class Epilogue>
__device__ __forceinline__ void stft_cmfft_rows(const CmfftIo &a, const Epilogue &epilogue)
{
    const uint32_t n = a.n, fold = a.fold, lpf = a.lpf, fy = a.fy;
    fft_v2f *bufA = (fft_v2f *)fft_lds;
    fft_v2f *bufB = bufA + (size_t)fy * n;
    fft_v2f *tw = bufB + (size_t)fy * n;
    float *mean_s = (float *)(tw + fold);
    const uint32_t tid = threadIdx.x;
    const uint32_t slot = tid / lpf, l = tid - slot * lpf;
    // the twiddle table
    for (uint32_t k = tid; k < fold; k += kFftBlock) {
        double sn, cs;
        sincospi((double)k * 2.0 / (double)n, &sn, &cs);
        tw[k] = fft_v2f{(float)cs, (float)-sn};
    }
    // bit c of cols: the lane has a column c (c * lpf + l < n: the last one may be missing); of wins: it is a window column
    uint32_t cols = 0, wins = 0;
#pragma unroll
    for (uint32_t c = 0; c < kCfftMaxCpl; ++c) {
        const uint32_t j = c * lpf + l;
        if (c < a.cpl && j < n) {
            cols |= 1u << c;
            if (j - a.col0 < a.len) wins |= 1u << c;                   // unsigned: a window column
        }
    }
    // the lane's coefficients
    float v[kCfftMaxCpl];
    {
        const float *vbuf = (const float *)bufA;
#pragma unroll
        for (uint32_t c = 0; c < kCfftMaxCpl; ++c) v[c] = ((cols >> c) & 1u) ? vbuf[c * lpf + l] : 0.0f;
    }
    __syncthreads();
    const uint32_t wave = tid >> 6, lane = tid & 63u;
    const uint64_t T = a.samples;
    fft_v2f *rowA = bufA + (size_t)slot * n;                           // the slot's row
    for (uint64_t g = mfft_first_group(epilogue); g < a.groups; g = mfft_next_group(epilogue, g)) {
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
        fft_v2f e[kCfftMaxCpl];
#pragma unroll
        for (uint32_t c = 0; c < kCfftMaxCpl; ++c) {
            e[c] = fft_v2f{0.0f, 0.0f};
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
                fft_v2f xv;
                if (a.vec) xv = *(const fft_v2f *)px;
                else       xv = fft_v2f{px[0], px[1]};
                e[c] = zero ? fft_v2f{0.0f, 0.0f} : xv;
            }
        }
        if (a.detrend) {
            // the raw row (col0 0: column j is sample j), then one wave per row and both channels: the order of k_welch_mean
#pragma unroll
            for (uint32_t c = 0; c < kCfftMaxCpl; ++c)
                if ((cols >> c) & 1u) rowA[c * lpf + l] = e[c];
            __syncthreads();
            for (uint32_t s = wave; s < fy; s += kFftBlock / 64u) {
                const fft_v2f *row = bufA + (size_t)s * n;
                double P0 = 0.0, P1 = 0.0;
                for (uint32_t j = lane; j < a.len; j += 64u) {
                    const fft_v2f z = row[j];
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
                    rowA[c * lpf + l] = ((take >> c) & 1u) ? fft_v2f{d0 * v[c], d1 * v[c]} : fft_v2f{0.0f, 0.0f};
                }
        } else {
#pragma unroll
            for (uint32_t c = 0; c < kCfftMaxCpl; ++c)
                if ((cols >> c) & 1u) rowA[c * lpf + l] = ((take >> c) & 1u) ? fft_v2f{e[c].x * v[c], e[c].y * v[c]} : fft_v2f{0.0f, 0.0f};
        }
        __syncthreads();
        // the passes: Ns the product of the radices so far, rest = n / (Ns * r) after this pass = the twiddle stride n / (r Ns)
        fft_v2f *src = rowA, *dst = bufB + (size_t)slot * n;
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
        if constexpr (Epilogue::kStore) {
            // the store: bin k to column k, or to (k + n / 2) mod n
            if (live) {
                float *yrow = a.Y + b * a.y_bstride + f * a.y_stride;
                const uint32_t turn = a.binshift ? n >> 1 : 0u;
                if (a.power) {
                    for (uint32_t k = l; k < n; k += lpf) {
                        uint32_t col = k + turn;
                        col = col >= n ? col - n : col;
                        yrow[col] = mfft_power(src[k]);
                    }
                } else {
                    fft_v2f *yp = (fft_v2f *)yrow;
                    for (uint32_t k = l; k < n; k += lpf) {
                        uint32_t col = k + turn;
                        col = col >= n ? col - n : col;
                        yp[col] = src[k];
                    }
                }
            }
        } else {
            epilogue(a, g, b, f0, src - (size_t)slot * n);
        }
        __syncthreads();                                                // the next group overwrites both buffers
    }
}

} // namespace
