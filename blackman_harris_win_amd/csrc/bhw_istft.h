// bhw_istft.h -- what the four fused inverse units (bhw_istft_fft.hip, bhw_istft_mfft.hip, bhw_istft_cfft.hip, bhw_istft_cmfft.hip)
// share beyond bhw_stft_fft.h's fft_v2f, cmul and twiddle: the launch-side fill of their Io structs and the device helpers of the
// flush.  The span walk, the ring and the flush themselves are each unit's own text.
#pragma once
#include "bhw_stft_fft.h"

namespace {

// The fields every inverse Io has under one name, from the plan (any BhwIstftRuns with lpf, fy and cpl) and the descriptor; the rest
// value-initialised, for the launcher to set: m / n / fold, the radix fields or sched, binshift, vec.  Each Io keeps its own layout:
// it is a kernel argument.
template <typename Io, typename Plan>
inline Io istft_io(const Plan &pl, const bhw_stft *s, const float *d_Y, float *d_x)
{
    Io a{};
    a.Y = d_Y;
    a.x = d_x;
    a.batch = s->batch;
    a.frames = s->frames;
    a.hop = pl.hop;
    a.samples = s->samples;
    a.t0 = pl.t0;
    a.x_stride = pl.x_stride;
    a.y_stride = pl.y_stride;
    a.y_bstride = pl.y_bstride;
    a.span = pl.span;
    a.spans = pl.spans;
    a.groups = pl.groups;
    a.trips = pl.trips;
    a.col0 = (uint32_t)s->col0;
    a.len = (uint32_t)pl.len;
    a.lpf = pl.lpf;
    a.fy = pl.fy;
    a.cpl = pl.cpl;
    a.shift = s->shift;
    a.normalize = pl.normalize ? 1u : 0u;
    return a;
}

// a flushed output: the sum, or the sum over the window envelope (+0.0 where the envelope is not positive)
__device__ __forceinline__ float istft_out(double s, double e, uint32_t normalize)
{
    if (!normalize) return (float)s;
    return e > 0.0 ? (float)(s / e) : 0.0f;
}

// the complex sample at float offset 2 * t of a signal: one 8-byte store on the 8-byte grid, else two 4-byte ones
__device__ __forceinline__ void istft_store(float *xb, uint64_t t, fft_v2f z, uint32_t vec)
{
    float *px = xb + 2 * t;
    if (vec) *(fft_v2f *)px = z;
    else {
        px[0] = z.x;
        px[1] = z.y;
    }
}

} // namespace
