// bhw_welch_csd.hip -- Welch cross spectra behind the FFT (bhw_welch_csd_f32; contract: section "Welch cross spectra" of bhw.h): X and
// Y are read once, and P_xy, P_xx, P_yy, the coherence and the H1 transfer function all come from the same ordered binary64 sums.
//
// The grid is the periodogram's (bhw_welch.h): one workgroup per (signal of Y, frame block, bin tile), kPsdLanes lanes along the bins so
// that a wave reads 64 consecutive complex64 values of a row, kPsdWaves waves over the frames of a pass.  What differs is two operands
// and CH ordered chains per bin instead of one.  Wave w loads U frames of X and U of Y (2 U 8-byte nontemporal loads in flight) and puts
// their CH binary64 terms -- per element, so order-free -- in LDS; then wave c < CH adds chain c of the pass in ascending order into the
// lane's sum, which it carries from pass to pass.  So the four ordered sums run side by side on four waves, each as long as the
// periodogram's one.  The terms, not the raw pairs, are staged: every wave then converts and multiplies a quarter of the rows, and the
// adding waves do one LDS read and one add per row.  A pass fills 32 KiB of LDS whatever CH is (U = 4 frames a wave for four chains, 8 for
// two), so four workgroups fit a CU.  Rows past the block's end are loaded clamped to its last row and never added.
#include "bhw_csd_out.h"

namespace {

// PARTIAL: the block sums go to the workspace; else (one block) the outputs are written.
template <int CH, bool PARTIAL>
__global__ __launch_bounds__(kPsdLanes * kPsdWaves) void k_welch_csd(CsdArgs a)
{
    constexpr uint32_t U = kCsdPassBytes / (kPsdWaves * kPsdLanes * CH * 8u), kPass = kPsdWaves * U;
    static_assert(CH == 2 || CH == 4, "two chains (P_xy alone) or four");
    static_assert(CH <= (int)kPsdWaves && kPass * CH * kPsdLanes * 8u == kCsdPassBytes && BHW_WELCH_BLOCK % kPass == 0, "pass");
    __shared__ double t_s[CH][kPass][kPsdLanes];
    const uint32_t lane = threadIdx.x & (kPsdLanes - 1u), wave = threadIdx.x / kPsdLanes;
    const uint64_t unit = blockIdx.x;
    const uint64_t tile = unit % a.tiles, rest = unit / a.tiles;
    const uint64_t blk = rest % a.blocks, b = rest / a.blocks;
    const uint64_t k = tile * kPsdLanes + lane;
    const bool active = k < a.bins;
    const uint64_t f0 = blk * BHW_WELCH_BLOCK;
    const uint64_t f1 = f0 + BHW_WELCH_BLOCK < a.frames ? f0 + BHW_WELCH_BLOCK : a.frames;
    const uint64_t kk = active ? k : a.bins - 1u;                                        // an idle lane reads the last bin
    const csd_v2f *xp = (const csd_v2f *)a.X + b * a.x_bstride + kk;                     // x_bstride 0: X is broadcast
    const csd_v2f *yp = (const csd_v2f *)a.Y + b * a.y_bstride + kk;
    csd_v2f ex[U], ey[U];
    auto load_pass = [&](uint64_t p0) {
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint64_t fr = p0 + wave * U + u, fc = fr < f1 ? fr : f1 - 1u;
            ex[u] = __builtin_nontemporal_load(xp + fc * a.x_stride);
            ey[u] = __builtin_nontemporal_load(yp + fc * a.y_stride);
        }
    };
    double A = 0.0;
    load_pass(f0);
    for (uint64_t p0 = f0; p0 < f1; p0 += kPass) {
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const double xr = (double)ex[u].x, xi = (double)ex[u].y, yr = (double)ey[u].x, yi = (double)ey[u].y;
            const uint32_t row = wave * U + u;
            // every product is exact in binary64: each term is one rounding, fused or not
            if constexpr (CH == 4) {
                t_s[0][row][lane] = __builtin_fma(xr, xr, xi * xi);
                t_s[1][row][lane] = __builtin_fma(yr, yr, yi * yi);
            }
            t_s[CH - 2][row][lane] = __builtin_fma(xr, yr, xi * yi);
            t_s[CH - 1][row][lane] = __builtin_fma(xr, yi, -(xi * yr));
        }
        __syncthreads();
        if (p0 + kPass < f1) load_pass(p0 + kPass);
        if (wave < (uint32_t)CH) {
            const uint32_t n = f1 - p0 < kPass ? (uint32_t)(f1 - p0) : kPass;
            if (n == kPass) {
#pragma unroll
                for (uint32_t i = 0; i < kPass; ++i) A += t_s[wave][i][lane];
            } else {
                for (uint32_t i = 0; i < n; ++i) A += t_s[wave][i][lane];
            }
        }
        __syncthreads();
    }
    if constexpr (PARTIAL) {
        if (wave < (uint32_t)CH && active) a.ws[((b * a.blocks + blk) * CH + wave) * a.bins + k] = A;
    } else {
        if (wave < (uint32_t)CH) t_s[wave][0][lane] = A;                                 // the last pass has been read: its rows are free
        __syncthreads();
        if (wave != 0 || !active) return;
        double S[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) S[c] = t_s[c][0][lane];
        csd_out<CH>(a, S, b, k);
    }
}

// The block sums of one (signal, bin), each chain in ascending block order; then the outputs.
template <int CH>
__global__ __launch_bounds__(256) void k_welch_csd_join(CsdArgs a, uint64_t batch)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= batch * a.bins) return;
    const uint64_t b = i / a.bins, k = i - b * a.bins;
    const double *wp = a.ws + b * a.blocks * CH * a.bins + k;
    double S[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) S[c] = 0.0;
    constexpr uint32_t U = 4;                                      // blocks in flight per chain; past the last block the last one is loaded, not added
    for (uint64_t blk = 0; blk < a.blocks; blk += U) {
        double v[U][CH];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < CH; ++c) v[u][c] = wp[((blk + u < a.blocks ? blk + u : a.blocks - 1u) * CH + c) * a.bins];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
            if (blk + u < a.blocks) {
#pragma unroll
                for (int c = 0; c < CH; ++c) S[c] += v[u][c];
            }
    }
    csd_out<CH>(a, S, b, k);
}

} // namespace

int bhwk_welch_csd_f32(const BhwLaunch &l, const BhwCsdPlan &pl, const bhw_csd *d, const float *d_X, const float *d_Y, float *const *outs,
                       double *d_ws)
{
    hipStream_t st = (hipStream_t)l.stream;
    CsdArgs a;
    a.X = d_X;
    a.Y = d_Y;
    for (uint32_t i = 0; i < kCsdOutputs; ++i) a.out[i] = outs[i];
    a.ws = d_ws;
    a.frames = d->frames;
    a.bins = d->bins;
    a.n_fft = d->n_fft;
    a.blocks = pl.blocks;
    a.tiles = pl.tiles;
    a.x_stride = pl.x_stride;
    a.x_bstride = pl.x_bstride;
    a.y_stride = pl.y_stride;
    a.y_bstride = pl.y_bstride;
    a.o_stride = pl.o_stride;
    a.scale = d->scale;
    a.flags = d->flags;
    a.pad = 0;
    const dim3 grid((unsigned)pl.grid), block(kPsdLanes * kPsdWaves);
    with_int_or_last<2, 4>((int)pl.chains, [&](auto CH) {
        if (pl.blocks == 1) {
            launch(k_welch_csd<CH, false>, grid, block, st, a);
        } else {
            launch(k_welch_csd<CH, true>, grid, block, st, a);
            launch(k_welch_csd_join<CH>, dim3((unsigned)pl.join_grid), dim3(256), st, a, (uint64_t)d->batch);
        }
    });
    return finish(hipSuccess);
}
