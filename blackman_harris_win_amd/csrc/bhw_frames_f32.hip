// bhw_frames_f32.hip -- overlapped-frame apply with float32 samples (bhw_apply_frames_f32_device / bhw_apply_frames_f32_from_table):
// the STFT front end whose output a float FFT takes directly
//
// The kernels of bhw_frames.hip with float32 x and y.  A lane computes the int32 coefficient w[k] exactly as there -- by the direct
// CORDIC chains (direct_coeff / direct_coeff_mad, or their _ph forms over the length-L phase map) or by the gather over a resident
// table (range_coeff / range_coeff_ph) -- turns it once into v = fl32(w) * 2^-shift (v_cvt_f32_i32, then an exact v_ldexp_f32: a
// nonzero |w| >= 1 scaled by 2^-62 at most stays normal) and applies it to its G frames with the shared frame loop (bhw_frames.h):
//     y[f * y_stride + k * C + c] = fl32(x[(f * hop + k) * C + c] * v)      (one IEEE binary32 multiply, denormals kept)
// Same workgroup, grid, load policy and I/Q access forms as the int32 kernels; the bytes moved are the same.  No per-frame route.
#include "bhw_frames.h"

namespace {

struct FramesArgsF32 : FramesIo<float> {};

__device__ __forceinline__ float coeff_f32(int32_t w, uint32_t shift) { return ldexpf((float)w, -(int)shift); }

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_frames_direct).
template <int FORM>
__global__ __launch_bounds__(kFramesBlock) void k_frames_f32_direct(BhwCordicCfg cfg, BhwWinCfg win, FramesArgsF32 a)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    const uint32_t k = blockIdx.x * a.kx + (threadIdx.x & (a.kx - 1u));        // < N: grid.x * kx = N
    int32_t w;
    if constexpr (FORM == 2) w = direct_coeff_mad(cfg, win, lut_s, k);
    else                     w = direct_coeff<T>(cfg, win, lut_s, k);
    frames_apply(a, k, threadIdx.x / a.kx, coeff_f32(w, a.shift));
}

// Coefficient gathered from a resident table in format FMT (range_coeff); every lane reaches the gather.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFramesBlock) void k_frames_f32_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, FramesArgsF32 a)
{
    const uint32_t k = blockIdx.x * a.kx + (threadIdx.x & (a.kx - 1u));
    frames_apply(a, k, threadIdx.x / a.kx, coeff_f32(range_coeff<FMT, NT, MODE>(cfg, win, table, k), a.shift));
}

// Windows of any length L: the lanes past L apply nothing (the table form still gathers, at k = 0, for the escape format's
// wave-wide fix).
template <int FORM>
__global__ __launch_bounds__(kFramesBlock) void k_frames_f32_direct_len(BhwCordicCfg cfg, BhwWinCfg win, FramesArgsF32 a, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    const uint32_t k = blockIdx.x * a.kx + (threadIdx.x & (a.kx - 1u));
    if (k >= lp.len) return;
    int32_t w;
    if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
    else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
    frames_apply(a, k, threadIdx.x / a.kx, coeff_f32(w, a.shift));
}

template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFramesBlock) void k_frames_f32_table_len(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table,
                                                                        FramesArgsF32 a, BhwLenPhase lp)
{
    const uint32_t k = blockIdx.x * a.kx + (threadIdx.x & (a.kx - 1u));
    const bool in = k < lp.len;
    const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
    if (in) frames_apply(a, k, threadIdx.x / a.kx, coeff_f32(w, a.shift));
}

} // namespace

int bhwk_frames_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwFramesPlan &pl, const bhw_frames *f,
                    const float *d_x, float *d_y, const int32_t *d_table, const BhwLenPhase *lp)
{
    if (!f->frames) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    FramesArgsF32 a;
    a.x = d_x;
    a.y = d_y;
    a.frames = f->frames;
    a.hop = f->hop;
    a.y_stride = pl.y_stride;
    a.group = pl.group;
    a.kx = pl.kx;
    a.fy = pl.fy;
    a.shift = f->shift;
    a.io = pair_io(f->channels, d_x, d_y, pl.y_stride);
    const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y), block(kFramesBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) { launch_phase(k_frames_f32_direct_len<D>, k_frames_f32_direct<D>, lp, grid, block, st, c_in, w, a); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_phase(k_frames_f32_table_len<F, NT, M>, k_frames_f32_table<F, NT, M>, lp, grid, block, st, c, w, tab, a);
        });
}
