// bhw_stft_fft.hip -- window and real FFT in one kernel (bhw_stft_fft_f32_device / _from_table; contract: include/bhw.h, plan:
// BhwStftFftPlan in bhw_plan.h, reasons and measurements: DESIGN.md section 18).
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

extern __shared__ __attribute__((aligned(16))) unsigned char fft_lds[];

__device__ __forceinline__ float fft_coeff(int32_t w, uint32_t shift) { return ldexpf((float)w, -(int)shift); }

__device__ __forceinline__ fft_v2f cmul(fft_v2f a, fft_v2f w) { return fft_v2f{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }

// W at index idx < n_fft (table of n_fft / 2 entries, W[idx + n_fft / 2] = -W[idx])
__device__ __forceinline__ fft_v2f twiddle(const fft_v2f *tw, uint32_t idx, uint32_t m)
{
    const fft_v2f w = tw[idx & (m - 1u)];
    return (idx & m) ? fft_v2f{-w.x, -w.y} : w;
}

// Everything after the prologue's coefficients: vbuf = buffer A viewed as floats holds v[0..n_fft).
__device__ __forceinline__ void stft_fft_rows(const FftIo &a)
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
    for (uint64_t g = blockIdx.x; g < a.groups; g += gridDim.x) {
        const uint64_t r = g * fy + slot;
        const bool live = r < a.rows;
        const uint64_t b = live ? r / a.frames : 0, f = live ? r - b * a.frames : 0;
        const float *xb = a.x + b * a.x_stride;
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
        __syncthreads();                                                // the next group overwrites both buffers
    }
}

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_stft_frames_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_stft_fft_direct(BhwCordicCfg cfg, BhwWinCfg win, FftIo a, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vbuf = (float *)fft_lds;
    for (uint32_t j = threadIdx.x; j < a.n_fft; j += kFftBlock) {
        const uint32_t k = j - a.col0;                             // unsigned: k < L is the window test
        float v = 0.0f;
        if (k < a.len) {
            int32_t w;
            if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
            else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
            v = fft_coeff(w, a.shift);
        }
        vbuf[j] = v;
    }
    __syncthreads();
    stft_fft_rows(a);
}

// Coefficient gathered from a resident table in format FMT; every lane reaches the gather (at k = 0 outside the window) for the
// escape format's wave-wide fix.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_stft_fft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, FftIo a,
                                                               BhwLenPhase lp)
{
    float *vbuf = (float *)fft_lds;
    for (uint32_t j0 = 0; j0 < a.n_fft; j0 += kFftBlock) {
        const uint32_t j = j0 + threadIdx.x;
        const uint32_t k = j - a.col0;
        const bool in = j < a.n_fft && k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (j < a.n_fft) vbuf[j] = in ? fft_coeff(w, a.shift) : 0.0f;
    }
    __syncthreads();
    stft_fft_rows(a);
}

// launch() of bhw_device.h with the plan's dynamic LDS
template <typename... KArgs>
inline void launch_lds(void (*kernel)(KArgs...), dim3 grid, dim3 block, uint32_t lds, hipStream_t st, typename same_type<KArgs>::type... args)
{
    void *ptrs[] = {(void *)&args...};
    const hipError_t e = hipLaunchKernel(reinterpret_cast<const void *>(kernel), grid, block, ptrs, lds, st);
    if (e != hipSuccess && t_launch_err == hipSuccess) t_launch_err = e;
}

} // namespace

int bhwk_stft_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwStftFftPlan &pl, const bhw_stft *s,
                      const float *d_x, float *d_Y, const int32_t *d_table, const BhwLenPhase &lp)
{
    if (!pl.rows) return 0;
    hipStream_t st = (hipStream_t)l.stream;
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
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    if (!d_table) {
        with_int_or_last<2, 1, 0>(direct_form(c_in), [&](auto D) { launch_lds(k_stft_fft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp); });
        return finish(hipSuccess);
    }
    const BhwCordicCfg c = table_layout(c_in);
    int fmt, nt, mode;
    if (!bhwp_range_form(c, w, &fmt, &nt, &mode)) return (int)hipErrorInvalidValue;
    const void *tab = (const void *)d_table;
    with_range_form(fmt, nt, mode, [&](auto F, auto NT, auto M) {
        launch_lds(k_stft_fft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp);
    });
    return finish(hipSuccess);
}
