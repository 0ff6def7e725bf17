// bhw_stft.h -- the row loop of the batched, centred STFT framing (bhw_stft_f32.hip; contract: bhw_stft_frames_f32_* in bhw.h).
//
// A lane holds column j of the frame row (lanes along the row, kx of them per workgroup row, fy rows side by side).  Inside the
// window (col0 <= j < col0 + L) it holds v[j - col0]; outside it holds nothing and only writes +0.0.  The rows (b, f) of the whole
// batch are one pool, r = b * frames + f: the lane applies its coefficient to G rows of its row block, which may belong to several
// signals, and steps (b, f) by (step_b, step_f) with one compare instead of dividing.
//   - Four rows' loads are issued before their stores; two channels move as one 8-byte access when the bases and every stride allow
//     it (io 2), else as two 4-byte ones.  x takes default-policy loads: it is read up to ceil(n_fft / hop) times.
//   - Padding: t = f * hop + j - pad, taken as unsigned, is inside the signal when t < T -- one compare per element.  Only where it
//     fails (the first and last ceil(pad / hop) + 1 frames of a signal) the reflect map runs, or the constant mode loads index 0 and
//     multiplies +0.0 instead (so a negative coefficient gives -0.0, as torch's F.pad followed by the multiply does).
#pragma once
#include "bhw_device.h"

namespace {

struct StftIo {
    const float *x;
    float *y;
    uint64_t rows;            // B * frames
    uint64_t frames, hop, samples, pad;
    uint64_t x_stride, y_stride, y_bstride;
    uint64_t group;           // G
    uint64_t row_blocks;      // ceil(rows / (fy * G)); blocks past gridDim.y by a grid-stride loop
    uint64_t step_b, step_f;  // fy = step_b * frames + step_f
    uint32_t n_fft, col0, len;
    uint32_t kx, fy, shift;
    uint32_t io;              // 0: one channel; 1: two channels, 4-byte accesses; 2: two channels, one 8-byte access
    uint32_t reflect;         // 1: BHW_PAD_REFLECT, 0: BHW_PAD_CONSTANT
};

// the row after (b, f) by fy rows of the pool
__device__ __forceinline__ void stft_step(const StftIo &a, uint64_t &b, uint64_t &f)
{
    f += a.step_f;
    b += a.step_b;
    if (f >= a.frames) {
        f -= a.frames;
        ++b;
    }
}

// The rows of this lane.  C = channels, VEC: one 8-byte access; in: j is a window column (v its coefficient), else +0.0 is written.
template <int C, bool VEC>
__device__ __forceinline__ void stft_loop(const StftIo &a, uint32_t j, uint32_t ty, bool in, float v)
{
    constexpr int U = 4;
    const uint64_t step = a.fy, span = a.group * a.fy;
    const uint64_t T = a.samples;
    for (uint64_t by = blockIdx.y; by < a.row_blocks; by += gridDim.y) {
        const uint64_t r_beg = by * span + ty;
        const uint64_t r_end0 = (by + 1) * span;
        const uint64_t r_end = r_end0 < a.rows ? r_end0 : a.rows;
        if (r_beg >= r_end) continue;
        uint64_t b = r_beg / a.frames, f = r_beg - b * a.frames;
        for (uint64_t r = r_beg; r < r_end; r += U * step) {
            float e[U][C];
            uint64_t bu[U], fu[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                bu[u] = b;
                fu[u] = f;
                stft_step(a, b, f);
                if (in && r + u * step < r_end) {
                    uint64_t t = fu[u] * a.hop + j - a.pad;            // unsigned: t < T is the whole interior test
                    bool zero = false;
                    if (t >= T) {                                      // padding
                        const int64_t ts = (int64_t)t;
                        if (a.reflect) t = ts < 0 ? (uint64_t)(-ts) : 2 * (T - 1) - t;
                        else {
                            t = 0;
                            zero = true;
                        }
                    }
                    const uint64_t xi = bu[u] * a.x_stride + t * C;
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
                    if (zero) {
#pragma unroll
                        for (int c = 0; c < C; ++c) e[u][c] = 0.0f;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (r + u * step < r_end) {
                    float o[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) o[c] = in ? e[u][c] * v : 0.0f;
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

__device__ __forceinline__ void stft_apply(const StftIo &a, uint32_t j, uint32_t ty, bool in, float v)
{
    if (a.io == 0)      stft_loop<1, false>(a, j, ty, in, v);
    else if (a.io == 1) stft_loop<2, false>(a, j, ty, in, v);
    else                stft_loop<2, true>(a, j, ty, in, v);
}

} // namespace
