// bhw_stft_fft.h -- the body shared by the kernels that form a windowed row and transform it in LDS: bhw_stft_fft.hip (stores the
// spectrum row), bhw_spectrogram.hip (stores its powers, or those folded through a filter bank), bhw_welch_fft.hip (adds the
// powers over the frames of a run: DESIGN.md section 26) and bhw_csd_fft.hip (two signals side by side: section 29).  The row
// function is a template on the epilogue -- what happens to the transformed row -- and everything before it is one text for all.  Moving the body
// here left the instruction streams of k_stft_fft_direct<*> and k_stft_fft_table<*> unchanged.
//
// A workgroup owns whole rows.  Prologue, once per workgroup: the window coefficients v[0..n_fft) (+0.0 outside the window) by the
// direct CORDIC chains or the gather over a resident table, staged through LDS so that every lane ends with the cpl coefficients of
// its own columns in registers (the "second lane layout" of section 15: lanes along the row, several columns per lane); and the
// twiddle table W[k] = exp(-2 pi i k / n_fft), k < n_fft / 2, each component the float32 rounding of a binary64 sincospi.
// Then, for each group of fy rows the workgroup takes:
//   1. a lane loads the samples of its columns c * lpf + lane (consecutive lanes, consecutive samples), with the padding rule of
//      bhw_stft.h; with detrending the raw row goes to LDS, one wave per row sums it in the contract's order (64 binary64 partial
//      sums by j mod 64 in ascending j, the butterfly 32 ... 1) and leaves m = fl32(S / L) in LDS;
//   2. row[j] = fl32(x * v) or fl32(fl32(x - m) * v), +0.0 outside the window, goes to LDS as float: the real row IS the sequence of
//      M = n_fft / 2 complex points z[i] = (row[2i], row[2i + 1]);
//   3. a Stockham FFT of M points, out of place between two LDS buffers: radix-4 passes (the first without twiddles), one radix-2
//      pass at the end when log2 M is odd.  Butterfly i of a pass at sub-transform length Ns reads z[i + q * M / 4] -- consecutive
//      lanes, consecutive 8-byte words -- multiplies by W at q * k * n_fft / (4 Ns), k = i mod Ns, read from the table (never a
//      product of twiddles), and writes (i - k) * 4 + k + q * Ns;
//   4. the split pass: Y[k] = E + W[k] * O with E, O the even and odd halves of (Z[k], conj Z[M - k]); bins 0 and M are
//      (Zr + Zi, +0.0) and (Zr - Zi, +0.0).  Consecutive lanes write consecutive complex64 values of the spectrum row.
// A row's arithmetic does not depend on its slot, its group or the grid: the bits of a spectrum row are a function of the row alone.
#pragma once
#include "bhw_device.h"

namespace {

typedef float fft_v2f __attribute__((ext_vector_type(2)));

struct FftIo {
    const float *x;
    float *Y;
    uint64_t rows, frames, hop, samples, pad;
    uint64_t x_stride, y_stride, y_bstride;
    uint64_t groups;
    uint32_t n_fft, m, col0, len;
    uint32_t lpf, fy, cpl, radix4, radix2;
    uint32_t shift, reflect, detrend;
};

// The Io of a launch from the plan and the descriptor; the Welch, hold and csd plans carry zero y strides.
inline FftIo fft_io(const BhwStftFftPlan &pl, const bhw_stft *s, const float *d_x, float *d_Y)
{
    FftIo a;
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
    a.n_fft = (uint32_t)s->n_fft;
    a.m = pl.m;
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
    return a;
}

extern __shared__ __attribute__((aligned(16))) unsigned char fft_lds[];

__device__ __forceinline__ fft_v2f cmul(fft_v2f a, fft_v2f w) { return fft_v2f{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }

// W at index idx < n_fft (table of n_fft / 2 entries, W[idx + n_fft / 2] = -W[idx])
__device__ __forceinline__ fft_v2f twiddle(const fft_v2f *tw, uint32_t idx, uint32_t m)
{
    const fft_v2f w = tw[idx & (m - 1u)];
    return (idx & m) ? fft_v2f{-w.x, -w.y} : w;
}

// Bin k <= M of the split pass over the transformed points Z = src[0..M).
__device__ __forceinline__ fft_v2f fft_split_bin(const fft_v2f *src, const fft_v2f *tw, uint32_t k, uint32_t M)
{
    fft_v2f y;
    if (k == 0u || k == M) {
        const fft_v2f z = src[0];
        y = fft_v2f{k ? z.x - z.y : z.x + z.y, 0.0f};
    } else {
        const fft_v2f A = src[k], B = src[M - k], w = tw[k];
        const fft_v2f E = fft_v2f{0.5f * (A.x + B.x), 0.5f * (A.y - B.y)};
        const fft_v2f O = fft_v2f{0.5f * (A.y + B.y), 0.5f * (B.x - A.x)};
        y = E + cmul(O, w);
    }
    return y;
}

// The slot's Stockham buffer that does not hold the transformed points after the last pass: M complex64 = n_fft floats, idle until
// the barrier that ends the group.  The passes alternate between the buffers from A, so it is B after an even number of them.
__device__ __forceinline__ fft_v2f *fft_idle_buffer(const FftIo &a, uint32_t slot)
{
    fft_v2f *bufA = (fft_v2f *)fft_lds;
    const uint32_t odd = (a.radix4 + a.radix2) & 1u;
    return bufA + ((size_t)(odd ? 0u : a.fy) + slot) * a.m;
}

// What happens to a transformed row is the epilogue, a template parameter of the row function.  FftStoreSpectrum, the epilogue of
// bhw_stft_fft_f32_*, is a tag: its text (the split pass, consecutive lanes writing consecutive complex64 values of the spectrum
// row) stands in the row function itself under `if constexpr`, where it stood before the function was shared, because a call --
// even one inlined at once -- reorders the function's locals and with them the registers of the compiled forward kernels.  Any
// other epilogue is a callable, called by every lane of the workgroup (live or not) with the slot's transformed points in src; it
// may use the slot's idle buffer and may hold barriers that every lane reaches.
struct FftStoreSpectrum {
    static constexpr bool kSpectrum = true;
};

// An epilogue with a member kRuns owns RUNS instead of strided groups of the flat row pool (bhw_welch_fft.hip):
// the frame axis of every signal is padded to epilogue.fpad frames, a run is epilogue.gpr (a power of two) consecutive groups of one
// signal, workgroup w takes the runs w, w + grid, ... and a run's groups in ascending order; a row with f >= frames is not live.  It
// is called once per group by every lane as epilogue(a, M, g, b, f0, base, tw): the group, its signal, the frame of slot 0 and the
// transformed points of slot 0 (slot s at base + s * M).  Such an epilogue MAY CARRY STATE from group to group: the object handed to
// stft_fft_rows lives for the whole group loop, one per lane, and is taken by const reference like every epilogue, so what it carries
// (the sums of a run) stands in `mutable` members; the calls of a run's groups come in ascending order with nothing of another run
// between them.  Every other epilogue keeps the flat pool, under `if constexpr`, and is stateless.
template <class E, class = void>
struct fft_owns_runs : std::false_type {};
template <class E>
struct fft_owns_runs<E, std::void_t<decltype(E::kRuns)>> : std::true_type {};

// An epilogue that owns runs and has a member kPairs as well takes frames of TWO signals side by side (bhw_csd_fft.hip, DESIGN.md
// section 29): of the fy slots of a group the first pairs = fy / 2 carry the frames f0 .. f0 + pairs - 1 of signal b of a.x (signal 0
// under epilogue.bcast: one x is paired with every y) and the others the same frames of signal b of epilogue.y, both at b *
// a.x_stride.  fpad and gpr count frame PAIRS: group g begins at pair g * pairs of the padded axis.  The epilogue's call is the run
// owner's; slot s of x is at base + s * M, of y at base + (pairs + s) * M.
template <class E, class = void>
struct fft_has_pairs : std::false_type {};
template <class E>
struct fft_has_pairs<E, std::void_t<decltype(E::kPairs)>> : std::true_type {};

template <class E>
__device__ __forceinline__ uint64_t fft_first_group(const E &e)
{
    if constexpr (fft_owns_runs<E>::value) return (uint64_t)blockIdx.x * e.gpr;
    else                                   return blockIdx.x;
}

template <class E>
__device__ __forceinline__ uint64_t fft_next_group(const E &e, uint64_t g)
{
    if constexpr (fft_owns_runs<E>::value) return ((g + 1u) & (e.gpr - 1u)) ? g + 1u : g + 1u + (uint64_t)(gridDim.x - 1u) * e.gpr;
    else                                   return g + gridDim.x;
}

// Everything after the prologue's coefficients: vbuf = buffer A viewed as floats holds v[0..n_fft).
template <class Epilogue>
__device__ __forceinline__ void stft_fft_rows(const FftIo &a, const Epilogue &epilogue)
{
    const uint32_t M = a.m, n = a.n_fft, lpf = a.lpf, fy = a.fy;
    fft_v2f *bufA = (fft_v2f *)fft_lds;
    fft_v2f *bufB = bufA + (size_t)fy * M;
    fft_v2f *tw = bufB + (size_t)fy * M;
    float *mean_s = (float *)(tw + M);
    const uint32_t tid = threadIdx.x;
    const uint32_t slot = tid / lpf, l = tid - slot * lpf;
    // the twiddle table
    for (uint32_t k = tid; k < M; k += kFftBlock) {
        double sn, cs;
        sincospi((double)k * 2.0 / (double)n, &sn, &cs);
        tw[k] = fft_v2f{(float)cs, (float)-sn};
    }
    // the lane's coefficients
    float v[kFftMaxCpl];
    {
        const float *vbuf = (const float *)bufA;
#pragma unroll
        for (uint32_t c = 0; c < kFftMaxCpl; ++c) v[c] = c < a.cpl ? vbuf[c * lpf + l] : 0.0f;
    }
    __syncthreads();
    const uint32_t wave = tid >> 6, lane = tid & 63u;
    const uint64_t T = a.samples;
    // bit c of cols: the lane has a column c; of wins: that column is a window column.  Kept in vector registers and made opaque
    // once per group, so that the sixteen tests are two instructions each instead of sixteen lane masks held in scalar registers
    // across the group loop.
    uint32_t cols = 0, wins = 0;
#pragma unroll
    for (uint32_t c = 0; c < kFftMaxCpl; ++c) {
        if (c < a.cpl) {
            cols |= 1u << c;
            if (c * lpf + l - a.col0 < a.len) wins |= 1u << c;      // unsigned: a window column
        }
    }
    float *rowA = (float *)bufA + (size_t)slot * n;               // the slot's row as floats = its M complex points
    for (uint64_t g = fft_first_group(epilogue); g < a.groups; g = fft_next_group(epilogue, g)) {
        bool live;
        uint64_t b, f;
        [[maybe_unused]] uint64_t f0 = 0;
        [[maybe_unused]] bool second = false;
        if constexpr (fft_has_pairs<Epilogue>::value) {
            const uint32_t pairs = fy >> 1;
            const uint64_t r0 = g * pairs;                               // fpad is a multiple of pairs: a group never crosses a signal
            b = r0 / epilogue.fpad;
            f0 = r0 - b * epilogue.fpad;
            second = slot >= pairs;
            const uint32_t fs = second ? slot - pairs : slot;
            live = f0 + fs < a.frames;
            f = live ? f0 + fs : 0;
        } else if constexpr (fft_owns_runs<Epilogue>::value) {
            const uint64_t r0 = g * fy;                                  // fpad is a multiple of fy: a group never crosses a signal
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
        const float *xb;
        if constexpr (fft_has_pairs<Epilogue>::value) xb = second ? epilogue.y + b * a.x_stride : a.x + (epilogue.bcast ? 0u : b) * a.x_stride;
        else                                          xb = a.x + b * a.x_stride;
        const uint64_t t0 = f * a.hop + l - a.pad;                     // the (wrapped) time of column l
        asm volatile("" : "+v"(cols), "+v"(wins));
        const uint32_t take = live ? wins : 0u;
        float e[kFftMaxCpl];
#pragma unroll
        for (uint32_t c = 0; c < kFftMaxCpl; ++c) {
            e[c] = 0.0f;
            {
                if ((take >> c) & 1u) {
                    uint64_t t = t0 + c * lpf;                         // unsigned: t < T is the whole interior test
                    bool zero = false;
                    if (t >= T) {
                        const int64_t ts = (int64_t)t;
                        if (a.reflect) t = ts < 0 ? (uint64_t)(-ts) : 2 * (T - 1) - t;
                        else {
                            t = 0;
                            zero = true;
                        }
                    }
                    const float xv = xb[t];
                    e[c] = zero ? 0.0f : xv;
                }
            }
        }
        if (a.detrend) {
            // the raw row (col0 0: column j is sample j), then one wave per row: the order of k_welch_mean
#pragma unroll
            for (uint32_t c = 0; c < kFftMaxCpl; ++c)
                if ((cols >> c) & 1u) rowA[c * lpf + l] = e[c];
            __syncthreads();
            for (uint32_t s = wave; s < fy; s += kFftBlock / 64u) {
                const float *row = (const float *)bufA + (size_t)s * n;
                double P = 0.0;
                for (uint32_t j = lane; j < a.len; j += 64u) P += (double)row[j];
#pragma unroll
                for (int sh = 32; sh >= 1; sh >>= 1) P += __shfl_down(P, sh, 64);
                if (lane == 0) mean_s[s] = (float)(P / (double)a.len);
            }
            __syncthreads();
            const float mu = mean_s[slot];
#pragma unroll
            for (uint32_t c = 0; c < kFftMaxCpl; ++c)
                if ((cols >> c) & 1u) {
                    const float d = e[c] - mu;
                    rowA[c * lpf + l] = ((take >> c) & 1u) ? d * v[c] : 0.0f;
                }
        } else {
#pragma unroll
            for (uint32_t c = 0; c < kFftMaxCpl; ++c)
                if ((cols >> c) & 1u) rowA[c * lpf + l] = ((take >> c) & 1u) ? e[c] * v[c] : 0.0f;
        }
        __syncthreads();
        // the passes
        fft_v2f *src = bufA + (size_t)slot * M, *dst = bufB + (size_t)slot * M;
        uint32_t Ns = 1;
        const uint32_t Q = M >> 2;
        for (uint32_t p = 0; p < a.radix4; ++p) {
            const uint32_t ts = M / (2u * Ns);                         // n_fft / (4 Ns)
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
                const fft_v2f t3 = fft_v2f{a1.y - a3.y, a3.x - a1.x};   // -i (a1 - a3)
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
        if (a.radix2) {                                                 // Ns = M / 2: k = i, twiddle W_M^i = W[2 i]
            const uint32_t H = M >> 1;
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
        // the split pass and the store
        if constexpr (Epilogue::kSpectrum) {
            if (live) {
                fft_v2f *yp = (fft_v2f *)(a.Y + b * a.y_bstride + f * a.y_stride);
                for (uint32_t k = l; k <= M; k += lpf) {
                    fft_v2f y;
                    if (k == 0u || k == M) {
                        const fft_v2f z = src[0];
                        y = fft_v2f{k ? z.x - z.y : z.x + z.y, 0.0f};
                    } else {
                        const fft_v2f A = src[k], B = src[M - k], w = tw[k];
                        const fft_v2f E = fft_v2f{0.5f * (A.x + B.x), 0.5f * (A.y - B.y)};
                        const fft_v2f O = fft_v2f{0.5f * (A.y + B.y), 0.5f * (B.x - A.x)};
                        y = E + cmul(O, w);
                    }
                    yp[k] = y;
                }
            }
        } else if constexpr (fft_owns_runs<Epilogue>::value) {
            epilogue(a, M, g, b, f0, src - (size_t)slot * M, tw);
        } else {
            epilogue(a, M, lpf, live, b, f, l, src, tw);
        }
        __syncthreads();                                                // the next group overwrites both buffers
    }
}

} // namespace
