// bhw_csd_fft.hip -- window, real FFT of two signals and the four frame averages of the Welch cross spectra in one kernel
// (bhw_csd_fft_f32_device / _from_table; contract: include/bhw.h, plan: BhwCsdFftPlan in bhw_plan.h, reasons and measurements:
// DESIGN.md section 29).
//
// The forward kernel of bhw_stft_fft.hip with an epilogue that owns runs of frame PAIRS: of the fy slots of a group the first pairs =
// fy / 2 hold the frames f0 .. f0 + pairs - 1 of x and the others the same frames of y; the row, the passes and the split expression
// are the one text of bhw_stft_fft.h, so (xr, xi) and (yr, yi) of a bin are the float32 pairs bhw_stft_fft_f32_* writes for it, and
// neither spectrum exists.  A run is max(16, pairs) consecutive frames of one pair of signals on the frame axis padded to whole
// chunks of BHW_WELCH_FFT_CHUNK = 16 frames; a workgroup takes the runs w, w + grid, ... and a run's groups in ascending order.  After
// the last pass of a group a lane forms the split bin of ITS bin for the x slot and the y slot of one frame after the other, in
// ascending frame order, and adds the four terms of bhw_welch_csd_f32 (xx, yy, re, im: one rounding each) into four binary64 sums:
//   pairs >= 16 (n_fft <= 64): the group holds pairs / 16 whole chunks; lane i < (pairs / 16) * K owns (chunk i / K, bin i % K), sums
//       the chunk's live frames from +0.0 and stores the four chunk sums.  Nothing is carried between groups.
//   pairs < 16 (n_fft >= 128): lane t owns the bins t, t + 256, ... < M and lane 0 bin M as well where M >= 256 (kCsdFftMaxAcc = 5
//       bins of four sums at n_fft 2048), adds the group's live frames to its sums, carries them over the 16 / pairs groups of the run
//       and stores them at its end.
// A frame >= F is skipped (its rows were formed as zeros and loaded nothing), and a chunk that begins at or past F is never stored, so
// every chunk sum [(b * chunks + c) * 4 K + chain * K + k] is written exactly once and none outside the workspace
// (tests/cpp/san_csd_fft.cpp replays this).  The stores are plain.  The chain is part of the bin axis, so with several blocks the
// chunk sums of a block are added by k_welch_fft_join<true, false> of bhw_welch_fft.hip over 4 K bins; k_csd_fft_out adds the last
// level (the chunks of the one block, or the blocks) in ascending order from +0.0 and applies the output formulas of
// bhw_welch_csd_f32 (bhw_csd_out.h).  No float atomics.
#include "bhw_stft_fft.h"
#include "bhw_csd_out.h"

namespace {

struct CsdFftAcc {
    const float *y;            // the second operand: signal b at b * FftIo::x_stride
    double *chunk_ws;          // [(b * chunks + c) * 4 K + chain * K + k]
    uint64_t fpad, chunks;     // frames of a signal padded to whole runs; ceil(F / 16)
    uint32_t gpr;              // groups per run: max(1, 16 / pairs), pairs = fy / 2
    uint32_t bcast;            // 1: a.x holds one signal, paired with every signal of y
};

// the four terms of one (bin, frame), added to S = {S_xx, S_yy, C_re, C_im}: the expressions of k_welch_csd
__device__ __forceinline__ void csd_fft_add(double *S, fft_v2f x, fft_v2f y)
{
    const double xr = (double)x.x, xi = (double)x.y, yr = (double)y.x, yi = (double)y.y;
    // every product is exact in binary64: each term is one rounding, fused or not
    S[0] += __builtin_fma(xr, xr, xi * xi);
    S[1] += __builtin_fma(yr, yr, yi * yi);
    S[2] += __builtin_fma(xr, yr, xi * yi);
    S[3] += __builtin_fma(xr, yi, -(xi * yr));
}

// One object per lane lives for the whole group loop of stft_fft_rows; the sums of a run stay in its mutable members from one
// group's call to the next (bhw_stft_fft.h: an epilogue which owns runs may do this).
struct FftCrossAccumulate {
    static constexpr bool kSpectrum = false;
    static constexpr bool kRuns = true;
    static constexpr bool kPairs = true;
    const float *y;
    double *chunk_ws;
    uint64_t fpad, chunks;
    uint32_t gpr, bcast;
    mutable double acc[kCsdFftMaxAcc - 1u][kCsdFftChains];     // the bins tid + 256 i below M (every bin when M < 256)
    mutable double acc_m[kCsdFftChains];                       // lane 0: bin M of a row with M >= 256

    __device__ __forceinline__ explicit FftCrossAccumulate(const CsdFftAcc &w)
        : y(w.y), chunk_ws(w.chunk_ws), fpad(w.fpad), chunks(w.chunks), gpr(w.gpr), bcast(w.bcast)
    {
#pragma unroll
        for (uint32_t c = 0; c < kCsdFftChains; ++c) {
#pragma unroll
            for (uint32_t i = 0; i < kCsdFftMaxAcc - 1u; ++i) acc[i][c] = 0.0;
            acc_m[c] = 0.0;
        }
    }

    // g: the group; b, f0: its pair of signals and the frame of slot 0; base: the transformed points of slot 0
    __device__ __forceinline__ void operator()(const FftIo &a, uint32_t M, uint64_t g, uint64_t b, uint64_t f0, const fft_v2f *base,
                                               const fft_v2f *tw) const
    {
        const uint32_t K = M + 1u, tid = threadIdx.x, pairs = a.fy >> 1;
        const uint64_t F = a.frames;
        const fft_v2f *xs = base, *ys = base + (size_t)pairs * M;
        if (pairs >= BHW_WELCH_FFT_CHUNK) {
            const uint32_t units = (pairs / BHW_WELCH_FFT_CHUNK) * K;
            for (uint32_t i = tid; i < units; i += kFftBlock) {
                const uint32_t c = i / K, k = i - c * K;
                const uint64_t fc = f0 + (uint64_t)c * BHW_WELCH_FFT_CHUNK;
                if (fc >= F) continue;                                  // a chunk of the padding: it has no place in the workspace
                const uint32_t n = F - fc < BHW_WELCH_FFT_CHUNK ? (uint32_t)(F - fc) : BHW_WELCH_FFT_CHUNK;
                const size_t s0 = (size_t)c * BHW_WELCH_FFT_CHUNK * M;
                double S[kCsdFftChains] = {0.0, 0.0, 0.0, 0.0};
                for (uint32_t s = 0; s < n; ++s)
                    csd_fft_add(S, fft_split_bin(xs + s0 + (size_t)s * M, tw, k, M), fft_split_bin(ys + s0 + (size_t)s * M, tw, k, M));
                double *out = chunk_ws + (b * chunks + fc / BHW_WELCH_FFT_CHUNK) * (kCsdFftChains * (uint64_t)K) + k;
#pragma unroll
                for (uint32_t ch = 0; ch < kCsdFftChains; ++ch) out[(size_t)ch * K] = S[ch];
            }
            return;
        }
        const uint32_t n = f0 >= F ? 0u : F - f0 < pairs ? (uint32_t)(F - f0) : pairs;   // the live frames are the first n
        const bool last = ((g + 1u) & (gpr - 1u)) == 0u;                // the run's last group (uniform)
        // the run's chunk, f0 / 16 in each of its groups: the run began at a multiple of 16 below fpad, and fpad - F < 16, so it exists
        double *out = chunk_ws + (b * chunks + f0 / BHW_WELCH_FFT_CHUNK) * (kCsdFftChains * (uint64_t)K);
        // From n_fft 512 on K = 256 j + 1: lane 0 adds bin M aside, as FftAccumulate of bhw_welch_fft.hip does.
        const bool wide = M >= kFftBlock;
#pragma unroll
        for (uint32_t i = 0; i < kCsdFftMaxAcc - 1u; ++i) {
            const uint32_t k = tid + i * kFftBlock;
            if (wide ? k < M : k <= M) {
                for (uint32_t s = 0; s < n; ++s)
                    csd_fft_add(acc[i], fft_split_bin(xs + (size_t)s * M, tw, k, M), fft_split_bin(ys + (size_t)s * M, tw, k, M));
                if (last) {
#pragma unroll
                    for (uint32_t ch = 0; ch < kCsdFftChains; ++ch) {
                        out[(size_t)ch * K + k] = acc[i][ch];
                        acc[i][ch] = 0.0;
                    }
                }
            }
        }
        if (wide && tid == 0u) {
            for (uint32_t s = 0; s < n; ++s)
                csd_fft_add(acc_m, fft_split_bin(xs + (size_t)s * M, tw, M, M), fft_split_bin(ys + (size_t)s * M, tw, M, M));
            if (last) {
#pragma unroll
                for (uint32_t ch = 0; ch < kCsdFftChains; ++ch) {
                    out[(size_t)ch * K + M] = acc_m[ch];
                    acc_m[ch] = 0.0;
                }
            }
        }
    }
};

// Three waves per SIMD: the 20 binary64 sums on top of the row function's registers need 162 VGPRs; under this hint every instance
// compiles without scratch, and four waves would spill.
#define BHW_CSD_FFT_WAVES __attribute__((amdgpu_waves_per_eu(3, 3)))

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_stft_fft_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) BHW_CSD_FFT_WAVES void k_csd_fft_direct(BhwCordicCfg cfg, BhwWinCfg win, FftIo a, BhwLenPhase lp, CsdFftAcc wa)
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
    stft_fft_rows(a, FftCrossAccumulate(wa));
}

// Coefficient gathered from a resident table in format FMT (as k_stft_fft_table).
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) BHW_CSD_FFT_WAVES void k_csd_fft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, FftIo a,
                                                              BhwLenPhase lp, CsdFftAcc wa)
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
    stft_fft_rows(a, FftCrossAccumulate(wa));
}

// The last level of the join: the n_in sums of each chain of one (signal, bin) -- the chunks of the one block, or the blocks --
// [(b * n_in + i) * 4 K + chain * K + k], added in ascending order from +0.0, four at a time in flight; then the outputs.
__global__ __launch_bounds__(256) void k_csd_fft_out(CsdArgs a, uint64_t batch, uint64_t n_in)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= batch * a.bins) return;
    const uint64_t b = i / a.bins, k = i - b * a.bins;
    const uint64_t row = kCsdFftChains * a.bins;
    const double *wp = a.ws + b * n_in * row + k;
    double S[kCsdFftChains];
#pragma unroll
    for (uint32_t c = 0; c < kCsdFftChains; ++c) S[c] = 0.0;
    constexpr uint32_t U = 4;                                      // past the last sum the last one is loaded again and not added
    for (uint64_t j = 0; j < n_in; j += U) {
        double v[U][kCsdFftChains];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
#pragma unroll
            for (uint32_t c = 0; c < kCsdFftChains; ++c) v[u][c] = wp[(j + u < n_in ? j + u : n_in - 1u) * row + c * a.bins];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
            if (j + u < n_in) {
#pragma unroll
                for (uint32_t c = 0; c < kCsdFftChains; ++c) S[c] += v[u][c];
            }
    }
    csd_out<4>(a, S, b, k);
}

} // namespace

int bhwk_csd_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwCsdFftPlan &cp, const bhw_stft *s,
                     double scale, const float *d_x, const float *d_y, float *const *outs, double *d_ws, const int32_t *d_table,
                     const BhwLenPhase &lp)
{
    const BhwStftFftPlan &pl = cp.fft;
    if (!pl.rows) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    const FftIo a = fft_io(pl, s, d_x, nullptr);
    CsdFftAcc wa{};
    wa.y = d_y;
    wa.chunk_ws = d_ws;
    wa.fpad = cp.fpad;
    wa.chunks = cp.chunks;
    wa.gpr = cp.gpr;
    wa.bcast = (cp.flags & BHW_CSD_BROADCAST_X) ? 1u : 0u;
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    int e = with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_csd_fft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp, wa); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_csd_fft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp, wa);
        });
    if (e) return e;
    const uint64_t row = kCsdFftChains * cp.bins;
    if (cp.blocks > 1) {
        e = bhwk_welch_join_blocks(l, d_ws, s->batch, row, cp.chunks, cp.blocks, cp.blocks_grid);
        if (e) return e;
    }
    CsdArgs o{};
    for (uint32_t i = 0; i < kCsdOutputs; ++i) o.out[i] = outs[i];
    o.ws = cp.blocks > 1 ? d_ws + s->batch * cp.chunks * row : d_ws;    // the block sums follow the chunk sums
    o.frames = s->frames;
    o.bins = cp.bins;
    o.n_fft = s->n_fft;
    o.o_stride = cp.o_stride;
    o.scale = scale;
    o.flags = cp.flags;
    launch(k_csd_fft_out, dim3((unsigned)cp.out_grid), dim3(256), st, o, (uint64_t)s->batch, cp.blocks > 1 ? cp.blocks : cp.chunks);
    return finish(hipSuccess);
}
