// bhw_welch_f32.hip -- Welch's method around the FFT: the detrended, windowed, end-padded segments (bhw_welch_frames_f32_device /
// _from_table with BHW_WELCH_DETREND_CONSTANT; flags 0 is the stft frames kernel itself) and the averaged periodogram
// (bhw_welch_psd_f32).  The loops and the reasons for their shape: bhw_welch.h.
#include "bhw_welch.h"

namespace {

__device__ __forceinline__ float welch_coeff(int32_t w, uint32_t shift) { return ldexpf((float)w, -(int)shift); }

// The means of the rows: MODE 0 one channel; 1 two channels, 4-byte loads; 2 two channels, one 8-byte load.
template <int MODE>
__global__ __launch_bounds__(kWelchMeanBlock) void k_welch_mean(WelchMeanArgs a)
{
    if constexpr (MODE == 0)      welch_mean_rows<1, false>(a);
    else if constexpr (MODE == 1) welch_mean_rows<2, false>(a);
    else                          welch_mean_rows<2, true>(a);
}

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_stft_frames_direct).
template <int FORM>
__global__ __launch_bounds__(kFramesBlock) void k_welch_frames_direct(BhwCordicCfg cfg, BhwWinCfg win, WelchIo a, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    const uint32_t j = blockIdx.x * a.kx + (threadIdx.x & (a.kx - 1u));
    if (j >= a.n_fft) return;
    const bool in = j < a.len;
    float v = 0.0f;
    if (in) {
        int32_t w;
        if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, j));
        else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, j));
        v = welch_coeff(w, a.shift);
    }
    welch_apply(a, j, threadIdx.x / a.kx, in, v);
}

// Coefficient gathered from a resident table in format FMT; every lane reaches the gather (at k = 0 outside the window) for the
// escape format's wave-wide fix.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFramesBlock) void k_welch_frames_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, WelchIo a,
                                                                      BhwLenPhase lp)
{
    const uint32_t j = blockIdx.x * a.kx + (threadIdx.x & (a.kx - 1u));
    const bool in = j < a.n_fft && j < a.len;
    const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? j : 0u));
    if (j >= a.n_fft) return;
    welch_apply(a, j, threadIdx.x / a.kx, in, welch_coeff(w, a.shift));
}

// One workgroup per (signal, frame block, bin tile): kPsdLanes lanes along the bins, kPsdWaves waves side by side over the frames.  A
// pass covers kPsdWaves * U frames: wave w loads frames p0 + w * U + u, all U loads in flight, and writes q = re^2 + im^2 (binary64,
// order-free: it is per element) to LDS row w * U + u.  U is the plan's: 16 where the grid is small and the passes are what is waited
// for, 8 where it is large and more resident workgroups (fewer registers, half the LDS) stream better.  Wave 0 then adds the rows of the pass
// in ascending order into the lane's A, which it carries from pass to pass: the contract's plain ascending sum over the block, with the
// loads of four waves behind it instead of one lane's.  The next pass's loads are issued before wave 0 sums, so they fly meanwhile.
// Rows past the block's end are loaded clamped to its last row (no branch around a load) and never added.
// PARTIAL: the block sum goes to the workspace; else (one block) P is written.
template <bool PARTIAL, int UNROLL>
__global__ __launch_bounds__(kPsdLanes * kPsdWaves) void k_welch_psd(PsdArgs a)
{
    constexpr uint32_t U = UNROLL, kPsdPass = kPsdWaves * U;
    __shared__ double q_s[kPsdPass][kPsdLanes];
    const uint32_t lane = threadIdx.x & (kPsdLanes - 1u), wave = threadIdx.x / kPsdLanes;
    const uint64_t unit = blockIdx.x;
    const uint64_t tile = unit % a.tiles, rest = unit / a.tiles;
    const uint64_t blk = rest % a.blocks, b = rest / a.blocks;
    const uint64_t k = tile * kPsdLanes + lane;
    const bool active = k < a.bins;
    const uint64_t f0 = blk * BHW_WELCH_BLOCK;
    const uint64_t f1 = f0 + BHW_WELCH_BLOCK < a.frames ? f0 + BHW_WELCH_BLOCK : a.frames;
    const welch_v2f *yp = (const welch_v2f *)a.Y + b * a.y_bstride + (active ? k : a.bins - 1u);   // an idle lane reads the last bin
    welch_v2f e[U];
    auto load_pass = [&](uint64_t p0) {
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint64_t fr = p0 + wave * U + u;
            e[u] = __builtin_nontemporal_load(yp + (fr < f1 ? fr : f1 - 1u) * a.y_stride);
        }
    };
    double A = 0.0;
    load_pass(f0);
    for (uint64_t p0 = f0; p0 < f1; p0 += kPsdPass) {
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const double re = (double)e[u].x, im = (double)e[u].y;
            q_s[wave * U + u][lane] = __builtin_fma(re, re, im * im);             // im * im is exact: one rounding, as the contract's q_f
        }
        __syncthreads();
        if (p0 + kPsdPass < f1) load_pass(p0 + kPsdPass);
        if (wave == 0) {
            const uint32_t n = f1 - p0 < kPsdPass ? (uint32_t)(f1 - p0) : kPsdPass;
            if (n == kPsdPass) {
#pragma unroll
                for (uint32_t i = 0; i < kPsdPass; ++i) A += q_s[i][lane];
            } else {
                for (uint32_t i = 0; i < n; ++i) A += q_s[i][lane];
            }
        }
        __syncthreads();
    }
    if (wave != 0 || !active) return;
    if constexpr (PARTIAL) a.ws[(b * a.blocks + blk) * a.bins + k] = A;
    else                   a.P[b * a.p_stride + k] = psd_out(a, A, k);
}

// The block sums of one (signal, bin) in ascending block order.
__global__ __launch_bounds__(256) void k_welch_psd_join(PsdArgs a, uint64_t batch)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= batch * a.bins) return;
    const uint64_t b = i / a.bins, k = i - b * a.bins;
    const double *wp = a.ws + b * a.blocks * a.bins + k;
    double A = 0.0;
    constexpr uint32_t U = 16;                                     // block sums in flight; past the last block the last one is loaded, not added
    for (uint64_t blk = 0; blk < a.blocks; blk += U) {
        double v[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) v[u] = wp[(blk + u < a.blocks ? blk + u : a.blocks - 1u) * a.bins];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
            if (blk + u < a.blocks) A += v[u];
    }
    a.P[b * a.p_stride + k] = psd_out(a, A, k);
}

} // namespace

int bhwk_welch_frames_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwWelchPlan &wp, const bhw_stft *s,
                          const float *d_x, float *d_y, float *d_mean, const int32_t *d_table, const BhwLenPhase &lp)
{
    const BhwStftPlan &pl = wp.frames;
    if (!pl.rows) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    WelchIo a;
    a.x = d_x;
    a.mean = d_mean;
    a.y = d_y;
    a.rows = pl.rows;
    a.frames = s->frames;
    a.hop = s->hop;
    a.x_stride = pl.x_stride;
    a.y_stride = pl.y_stride;
    a.y_bstride = pl.y_bstride;
    a.group = pl.group;
    a.row_blocks = pl.row_blocks;
    a.step_b = pl.step_b;
    a.step_f = pl.step_f;
    a.n_fft = (uint32_t)s->n_fft;
    a.len = (uint32_t)pl.len;
    a.kx = pl.kx;
    a.fy = pl.fy;
    a.shift = s->shift;
    a.io = pair_io(s->channels, d_x, d_y, pl.y_stride);
    if (a.io == 2 && (pl.x_stride % 2 || pl.y_bstride % 2)) a.io = 1;
    WelchMeanArgs m;
    m.x = d_x;
    m.mean = d_mean;
    m.rows = pl.rows;
    m.frames = s->frames;
    m.hop = s->hop;
    m.x_stride = pl.x_stride;
    m.len = (uint32_t)pl.len;
    m.vec = (s->channels == 2 && (uintptr_t)d_x % 8 == 0 && pl.x_stride % 2 == 0) ? 1u : 0u;
    const int mode = s->channels == 1 ? 0 : m.vec ? 2 : 1;
    with_int_or_last<0, 1, 2>(mode, [&](auto M) { launch(k_welch_mean<M>, dim3((unsigned)wp.mean_grid), dim3(kWelchMeanBlock), st, m); });
    const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y), block(kFramesBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) { launch(k_welch_frames_direct<D>, grid, block, st, c_in, w, a, lp); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch(k_welch_frames_table<F, NT, M>, grid, block, st, c, w, tab, a, lp);
        });
}

int bhwk_welch_psd_f32(const BhwLaunch &l, const BhwPsdPlan &pl, const bhw_psd *d, const float *d_Y, float *d_P, double *d_ws)
{
    hipStream_t st = (hipStream_t)l.stream;
    PsdArgs a;
    a.Y = d_Y;
    a.P = d_P;
    a.ws = d_ws;
    a.frames = d->frames;
    a.bins = d->bins;
    a.n_fft = d->n_fft;
    a.blocks = pl.blocks;
    a.tiles = pl.tiles;
    a.y_stride = pl.y_stride;
    a.y_bstride = pl.y_bstride;
    a.p_stride = pl.p_stride;
    a.scale = d->scale;
    a.flags = d->flags;
    a.pad = 0;
    const dim3 grid((unsigned)pl.grid), block(kPsdLanes * kPsdWaves);
    if (pl.blocks == 1) {
        with_int_or_last<16, 8>((int)pl.unroll, [&](auto U) { launch(k_welch_psd<false, U>, grid, block, st, a); });
    } else {
        with_int_or_last<16, 8>((int)pl.unroll, [&](auto U) { launch(k_welch_psd<true, U>, grid, block, st, a); });
        launch(k_welch_psd_join, dim3((unsigned)pl.join_grid), dim3(256), st, a, (uint64_t)d->batch);
    }
    return finish(hipSuccess);
}
