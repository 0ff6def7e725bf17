// bhw_welch.h -- the loops of Welch's method around the FFT (bhw_welch_f32.hip; contracts: section "Welch's method" of bhw.h).
//
// Segments with a constant detrend take two launches.
//   - k_welch_mean: one wave per row (b, f) of the batch's row pool.  Lane i adds x_j for j = i, i + 64, ... in ascending j into a
//     binary64 partial sum P[i] (four loads in flight, added in order), the wave folds the 64 partial sums by the butterfly
//     s = 32, 16, ..., 1 (P[i] += P[i + s] for i < s), and lane 0 stores m = fl32(P[0] / L) at mean[r * C + c].  The order is the one
//     bhw.h writes down: a function of L alone, whatever the plan of the second launch.
//   - welch_loop: the row loop of bhw_stft.h without its padding path (pad 0, col0 0), with one more load per row -- the row's mean,
//     the same address in every lane of the row, so one cache line per wave -- and a subtraction in front of the multiply:
//     y = fl32(fl32(x - m) * v), two roundings; a subtraction feeding a multiply is nothing a compiler may fuse.
// The averaged periodogram keeps its lanes along the bins, so a wave reads 64 consecutive complex64 values of one row.  The contract's
// sum over a block of BHW_WELCH_BLOCK frames is one ascending chain per bin, which leaves B * blocks * K lanes of parallelism: too few
// loads in flight when one lane walks its own frames (measured).  So four waves load the frames of a pass and
// put re^2 + im^2 (binary64; per element, so order-free) in LDS, and one wave adds the pass in ascending order.  Y is read once, with
// nontemporal loads (the policy of emit() and bhw_ola_f32.h for read-once operands).
#pragma once
#include "bhw_device.h"

namespace {

typedef float welch_v2f __attribute__((ext_vector_type(2)));

struct WelchMeanArgs {
    const float *x;
    float *mean;
    uint64_t rows, frames, hop, x_stride;
    uint32_t len;
    uint32_t vec;             // two channels: 1 = one 8-byte load per pair
};

struct WelchIo {
    const float *x;
    const float *mean;
    float *y;
    uint64_t rows, frames, hop;
    uint64_t x_stride, y_stride, y_bstride;
    uint64_t group, row_blocks, step_b, step_f;
    uint32_t n_fft, len;
    uint32_t kx, fy, shift;
    uint32_t io;              // as StftIo
};

template <int C, bool VEC>
__device__ __forceinline__ void welch_mean_rows(const WelchMeanArgs &a)
{
    constexpr uint32_t U = 4;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t per_wg = kWelchMeanBlock / 64u;
    const uint32_t L = a.len;
    for (uint64_t r = (uint64_t)blockIdx.x * per_wg + wave; r < a.rows; r += (uint64_t)gridDim.x * per_wg) {
        const uint64_t b = r / a.frames, f = r - b * a.frames;
        const float *xp = a.x + b * a.x_stride + f * a.hop * C;
        double P[C];
#pragma unroll
        for (int c = 0; c < C; ++c) P[c] = 0.0;
        for (uint32_t j = lane; j < L; j += 64u * U) {
            float e[U][C];
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) {
                const uint32_t ju = j + 64u * u;
                if (ju < L) {
                    if constexpr (C == 1) {
                        e[u][0] = xp[ju];
                    } else if constexpr (VEC) {
                        const float2 p = *(const float2 *)(xp + (uint64_t)ju * 2u);
                        e[u][0] = p.x;
                        e[u][1] = p.y;
                    } else {
                        e[u][0] = xp[(uint64_t)ju * 2u];
                        e[u][1] = xp[(uint64_t)ju * 2u + 1u];
                    }
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < U; ++u)
                if (j + 64u * u < L) {
#pragma unroll
                    for (int c = 0; c < C; ++c) P[c] += (double)e[u][c];
                }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) P[c] += __shfl_down(P[c], s, 64);   // lanes i < s hold P[i] + P[i + s]; the others are not read again
            if (lane == 0) a.mean[r * C + c] = (float)(P[c] / (double)L);
        }
    }
}

__device__ __forceinline__ void welch_step(const WelchIo &a, uint64_t &b, uint64_t &f)
{
    f += a.step_f;
    b += a.step_b;
    if (f >= a.frames) {
        f -= a.frames;
        ++b;
    }
}

// The rows of this lane: column j < n_fft, `in` = j < L with v its coefficient; the other columns are the zero padding at the end.
template <int C, bool VEC>
__device__ __forceinline__ void welch_loop(const WelchIo &a, uint32_t j, uint32_t ty, bool in, float v)
{
    constexpr int U = 4;
    const uint64_t step = a.fy, span = a.group * a.fy;
    for (uint64_t by = blockIdx.y; by < a.row_blocks; by += gridDim.y) {
        const uint64_t r_beg = by * span + ty;
        const uint64_t r_end0 = (by + 1) * span;
        const uint64_t r_end = r_end0 < a.rows ? r_end0 : a.rows;
        if (r_beg >= r_end) continue;
        uint64_t b = r_beg / a.frames, f = r_beg - b * a.frames;
        for (uint64_t r = r_beg; r < r_end; r += U * step) {
            float e[U][C], m[U][C];
            uint64_t bu[U], fu[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                bu[u] = b;
                fu[u] = f;
                welch_step(a, b, f);
                if (in && r + u * step < r_end) {
                    const uint64_t xi = bu[u] * a.x_stride + (fu[u] * a.hop + j) * C;
                    const uint64_t mi = (r + u * step) * C;                 // row r of the pool is (bu, fu)
                    if constexpr (C == 1) {
                        e[u][0] = a.x[xi];
                    } else if constexpr (VEC) {
                        const float2 p = *(const float2 *)(a.x + xi);
                        e[u][0] = p.x;
                        e[u][1] = p.y;
                    } else {
                        e[u][0] = a.x[xi];
                        e[u][1] = a.x[xi + 1];
                    }
#pragma unroll
                    for (int c = 0; c < C; ++c) m[u][c] = a.mean[mi + c];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (r + u * step < r_end) {
                    float o[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const float d = in ? e[u][c] - m[u][c] : 0.0f;
                        o[c] = in ? d * v : 0.0f;
                    }
                    float *yp = a.y + bu[u] * a.y_bstride + fu[u] * a.y_stride + (uint64_t)j * C;
                    if constexpr (C == 1) {
                        yp[0] = o[0];
                    } else if constexpr (VEC) {
                        *(float2 *)yp = make_float2(o[0], o[1]);
                    } else {
                        yp[0] = o[0];
                        yp[1] = o[1];
                    }
                }
            }
        }
    }
}

__device__ __forceinline__ void welch_apply(const WelchIo &a, uint32_t j, uint32_t ty, bool in, float v)
{
    if (a.io == 0)      welch_loop<1, false>(a, j, ty, in, v);
    else if (a.io == 1) welch_loop<2, false>(a, j, ty, in, v);
    else                welch_loop<2, true>(a, j, ty, in, v);
}

struct PsdArgs {
    const float *Y;
    float *P;
    double *ws;
    uint64_t frames, bins, n_fft, blocks, tiles;
    uint64_t y_stride, y_bstride, p_stride;
    double scale;
    uint32_t flags;
    uint32_t pad;
};

__device__ __forceinline__ float psd_out(const PsdArgs &a, double A, uint64_t k)
{
    const double sk = bhw_psd_doubled(a.flags, k, a.bins, a.n_fft) ? a.scale * 2.0 : a.scale;
    return (float)(A * sk);
}

} // namespace
