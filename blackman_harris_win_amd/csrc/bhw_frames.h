// bhw_frames.h -- the frame loop of the overlapped-frame apply, shared by its int32 (bhw_frames.hip) and float32 (bhw_frames_f32.hip)
// kernels: a lane holds coefficient k of the window and applies it to G frames of one signal.
//   - The frame loop issues four frames' loads before their stores; two channels move as one 8-byte access when both bases and the
//     stride allow it (io 2), else as two 4-byte ones.
//   - x takes default-policy loads: it is read up to ceil(N / hop) times (once per frame that covers it), and the nontemporal load
//     of the single-use emit() would push it past the caches.
#pragma once
#include "bhw_device.h"

namespace {

// The launch arguments of a frames kernel whose samples are of type E (int32_t or float).
template <typename E>
struct FramesIo {
    const E *x;
    E *y;
    uint64_t frames, hop, y_stride;
    uint64_t group;      // G: frame rows of one workgroup
    uint32_t kx;         // lanes along k (a power of two)
    uint32_t fy;         // frame rows side by side in a workgroup: kFramesBlock / kx
    uint32_t shift;
    uint32_t io;         // 0: one channel; 1: two channels, 4-byte accesses; 2: two channels, one 8-byte access
};

// One windowed sample.  int32: low32((x * w) >> shift), the arithmetic of bhw_apply_device.  float: x * v, one IEEE binary32
// multiply (v = fl32(w) * 2^-shift is formed once per lane by the kernel).
__device__ __forceinline__ int32_t apply1(int32_t x, int32_t w, uint32_t shift) { return (int32_t)(((int64_t)x * (int64_t)w) >> shift); }
__device__ __forceinline__ float apply1(float x, float v, uint32_t) { return x * v; }

template <typename E> struct FramesPair;
template <> struct FramesPair<int32_t> { using type = int2; };
template <> struct FramesPair<float> { using type = float2; };
__device__ __forceinline__ int2 frames_pair(int32_t a, int32_t b) { return make_int2(a, b); }
__device__ __forceinline__ float2 frames_pair(float a, float b) { return make_float2(a, b); }

// The frames of this lane: rows [blockIdx.y * G, +G) of fy frames, frame f = row * fy + ty.  C = channels, VEC: one 8-byte access.
template <int C, bool VEC, typename E>
__device__ __forceinline__ void frames_loop(const FramesIo<E> &a, uint32_t k, uint32_t ty, E w)
{
    using P = typename FramesPair<E>::type;
    constexpr int U = 4;
    const uint64_t f_end0 = ((uint64_t)blockIdx.y + 1) * a.group * a.fy;
    const uint64_t f_end = f_end0 < a.frames ? f_end0 : a.frames;
    const uint64_t step = a.fy;
    for (uint64_t f = (uint64_t)blockIdx.y * a.group * a.fy + ty; f < f_end; f += U * step) {
        E v[U][C];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t fu = f + u * step;
            if (fu < f_end) {
                const uint64_t xi = (fu * a.hop + k) * C;
                if constexpr (C == 1) {
                    v[u][0] = a.x[xi];
                } else if constexpr (VEC) {
                    const P p = *(const P *)(a.x + xi);
                    v[u][0] = p.x;
                    v[u][1] = p.y;
                } else {
                    v[u][0] = a.x[xi];
                    v[u][1] = a.x[xi + 1];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t fu = f + u * step;
            if (fu < f_end) {
                E *yp = a.y + fu * a.y_stride + (uint64_t)k * C;
                if constexpr (C == 1) {
                    yp[0] = apply1(v[u][0], w, a.shift);
                } else if constexpr (VEC) {
                    *(P *)yp = frames_pair(apply1(v[u][0], w, a.shift), apply1(v[u][1], w, a.shift));
                } else {
                    yp[0] = apply1(v[u][0], w, a.shift);
                    yp[1] = apply1(v[u][1], w, a.shift);
                }
            }
        }
    }
}

template <typename E>
__device__ __forceinline__ void frames_apply(const FramesIo<E> &a, uint32_t k, uint32_t ty, E w)
{
    if (a.io == 0)      frames_loop<1, false>(a, k, ty, w);
    else if (a.io == 1) frames_loop<2, false>(a, k, ty, w);
    else                frames_loop<2, true>(a, k, ty, w);
}

} // namespace
