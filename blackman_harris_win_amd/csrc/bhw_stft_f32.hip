// bhw_stft_f32.hip -- batched, centred STFT framing with float32 samples (bhw_stft_frames_f32_device / _from_table): the framing of
// torch.stft (center, pad_mode, a window of win_length centred in an n_fft row) for B signals in one launch.
//
// Lanes run along the n_fft columns of a frame row (the row loop and its padding path: bhw_stft.h).  A lane inside the window computes
// w[j - col0] once -- by the direct CORDIC chains (direct_coeff_ph / direct_coeff_mad_ph) or the gather over a resident table
// (range_coeff_ph), always at the angles of the length-L phase map, which gives the power-of-two window bit for bit at L = 2^phi_width
// -- turns it into v = fl32(w) * 2^-shift as the *_f32 calls do, and applies it to G rows of the batch's row pool:
//     y[b * y_bstride + f * y_stride + j * C + c] = fl32(X_b(f * hop + j - pad, c) * v)       (one IEEE binary32 multiply)
// Lanes outside the window write +0.0 and compute nothing; they are the zero columns an FFT of n_fft needs.
#include "bhw_stft.h"

namespace {

__device__ __forceinline__ float stft_coeff(int32_t w, uint32_t shift) { return ldexpf((float)w, -(int)shift); }

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_frames_direct).
template <int FORM>
__global__ __launch_bounds__(kFramesBlock) void k_stft_frames_direct(BhwCordicCfg cfg, BhwWinCfg win, StftIo a, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    const uint32_t j = blockIdx.x * a.kx + (threadIdx.x & (a.kx - 1u));
    if (j >= a.n_fft) return;
    const uint32_t k = j - a.col0;                                 // unsigned: k < L is the window test
    const bool in = k < a.len;
    float v = 0.0f;
    if (in) {
        int32_t w;
        if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
        else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
        v = stft_coeff(w, a.shift);
    }
    stft_apply(a, j, threadIdx.x / a.kx, in, v);
}

// Coefficient gathered from a resident table in format FMT; every lane reaches the gather (at k = 0 outside the window) for the
// escape format's wave-wide fix.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFramesBlock) void k_stft_frames_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, StftIo a,
                                                                     BhwLenPhase lp)
{
    const uint32_t j = blockIdx.x * a.kx + (threadIdx.x & (a.kx - 1u));
    const uint32_t k = j - a.col0;
    const bool in = j < a.n_fft && k < a.len;
    const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
    if (j >= a.n_fft) return;
    stft_apply(a, j, threadIdx.x / a.kx, in, stft_coeff(w, a.shift));
}

} // namespace

int bhwk_stft_frames_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwStftPlan &pl, const bhw_stft *s,
                         const float *d_x, float *d_y, const int32_t *d_table, const BhwLenPhase &lp)
{
    if (!pl.rows) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    StftIo a;
    a.x = d_x;
    a.y = d_y;
    a.rows = pl.rows;
    a.frames = s->frames;
    a.hop = s->hop;
    a.samples = s->samples;
    a.pad = s->pad;
    a.x_stride = pl.x_stride;
    a.y_stride = pl.y_stride;
    a.y_bstride = pl.y_bstride;
    a.group = pl.group;
    a.row_blocks = pl.row_blocks;
    a.step_b = pl.step_b;
    a.step_f = pl.step_f;
    a.n_fft = (uint32_t)s->n_fft;
    a.col0 = (uint32_t)s->col0;
    a.len = (uint32_t)pl.len;
    a.kx = pl.kx;
    a.fy = pl.fy;
    a.shift = s->shift;
    a.reflect = s->pad_mode == BHW_PAD_REFLECT ? 1u : 0u;
    // the 8-byte pair access needs every signal and row start 8-byte aligned: both bases and all three strides even
    a.io = pair_io(s->channels, d_x, d_y, pl.y_stride);
    if (a.io == 2 && (pl.x_stride % 2 || pl.y_bstride % 2)) a.io = 1;
    const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y), block(kFramesBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) { launch(k_stft_frames_direct<D>, grid, block, st, c_in, w, a, lp); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch(k_stft_frames_table<F, NT, M>, grid, block, st, c, w, tab, a, lp);
        });
}
