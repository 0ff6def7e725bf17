// bhw_welch_fft.hip -- window, real FFT and the frame average in one kernel (bhw_welch_fft_f32_device / _from_table; contract:
// include/bhw.h, plan: BhwWelchFftPlan in bhw_plan.h, reasons and measurements: DESIGN.md section 26).
//
// The forward kernel of bhw_stft_fft.hip with an epilogue that owns runs: the row, the passes and the split expression are the one
// text of bhw_stft_fft.h, so (re, im) of a bin are the float32 pair bhw_stft_fft_f32_* writes for it, and the spectrum never exists.
// A run is max(16, fy) consecutive frames of one signal on the frame axis padded to whole chunks of BHW_WELCH_FFT_CHUNK = 16 frames;
// a workgroup takes the runs w, w + grid, ... and a run's groups of fy rows in ascending order.  After the last pass of a group the
// transformed points of every slot are in LDS behind the pass's barrier, and a lane forms the split bin of ITS bin for one slot after
// the other, in ascending frame order, adding q = (double) re * re + (double) im * im into binary64:
//   fy >= 16 (n_fft <= 128): the group holds fy / 16 whole chunks; lane i < (fy / 16) * K owns (chunk i / K, bin i % K), sums the
//       chunk's live slots from +0.0 and stores the chunk sum.  Nothing is carried between groups.
//   fy < 16 (n_fft >= 256): lane t owns the bins t, t + 256, ... < M and lane 0 bin M as well (kWelchFftMaxAcc = 9 at n_fft 4096,
//       two on lane 0 at 512; at n_fft 256 lane t <= 128 owns bin t), adds the group's live slots to its accumulators, carries
//       them over the 16 / fy groups of the run and stores them at its end.
// A slot whose frame is >= F is skipped (its row was formed as zeros and loaded nothing), and a chunk that begins at or past F is
// never stored, so every chunk sum [(b * chunks + c) * K + k] is written exactly once and none outside the workspace
// (tests/cpp/san_welch_fft.cpp replays this).  The stores are plain; two small kernels join them in the contract's order:
// k_welch_fft_join<true, *> adds the chunk sums of a block of BHW_WELCH_BLOCK frames, sixteen loads in flight, and writes the block
// sum -- or P when there is one block --, k_welch_fft_join<false, true> adds the block sums sixteen at a time and writes P.  No float
// atomics.
#include "bhw_stft_fft.h"

namespace {

struct WelchFftAcc {
    double *chunk_ws;          // [(b * chunks + c) * K + k]
    uint64_t fpad, chunks;     // frames of a signal padded to whole runs; ceil(F / 16)
    uint32_t gpr;              // groups per run: max(1, 16 / fy)
    uint32_t pad;
};

__device__ __forceinline__ double welch_fft_q(fft_v2f y)
{
    const double re = (double)y.x, im = (double)y.y;
    return __builtin_fma(re, re, im * im);                              // im * im is exact: one rounding, the contract's q_f
}

// The epilogue carries state: one object per lane lives for the whole group loop of stft_fft_rows, and the sums of a run stay in its
// mutable members from one group's call to the next (the row function takes every epilogue by const reference; bhw_stft_fft.h says
// that an epilogue which owns runs may do this).
struct FftAccumulate {
    static constexpr bool kSpectrum = false;
    static constexpr bool kRuns = true;
    double *chunk_ws;
    uint64_t fpad, chunks;
    uint32_t gpr;
    mutable double acc[kWelchFftMaxAcc - 1u];      // the bins tid + 256 i below M (every bin when M < 256)
    mutable double acc_m;                          // lane 0: bin M of a row with M >= 256

    __device__ __forceinline__ explicit FftAccumulate(const WelchFftAcc &w) : chunk_ws(w.chunk_ws), fpad(w.fpad), chunks(w.chunks), gpr(w.gpr)
    {
#pragma unroll
        for (uint32_t i = 0; i < kWelchFftMaxAcc - 1u; ++i) acc[i] = 0.0;
        acc_m = 0.0;
    }

    // g: the group; b, f0: its signal and the frame of slot 0; base: the transformed points of slot 0
    __device__ __forceinline__ void operator()(const FftIo &a, uint32_t M, uint64_t g, uint64_t b, uint64_t f0, const fft_v2f *base,
                                               const fft_v2f *tw) const
    {
        const uint32_t K = M + 1u, fy = a.fy, tid = threadIdx.x;
        const uint64_t F = a.frames;
        if (fy >= BHW_WELCH_FFT_CHUNK) {
            const uint32_t pairs = (fy / BHW_WELCH_FFT_CHUNK) * K;
            for (uint32_t i = tid; i < pairs; i += kFftBlock) {
                const uint32_t c = i / K, k = i - c * K;
                const uint64_t fc = f0 + (uint64_t)c * BHW_WELCH_FFT_CHUNK;
                if (fc >= F) continue;                                  // a chunk of the padding: it has no place in the workspace
                const uint32_t n = F - fc < BHW_WELCH_FFT_CHUNK ? (uint32_t)(F - fc) : BHW_WELCH_FFT_CHUNK;
                const fft_v2f *src = base + (size_t)c * BHW_WELCH_FFT_CHUNK * M;
                double A = 0.0;
                for (uint32_t s = 0; s < n; ++s) A += welch_fft_q(fft_split_bin(src + (size_t)s * M, tw, k, M));
                chunk_ws[(b * chunks + fc / BHW_WELCH_FFT_CHUNK) * K + k] = A;
            }
            return;
        }
        const uint32_t n = f0 >= F ? 0u : F - f0 < fy ? (uint32_t)(F - f0) : fy;     // the live slots are the first n
        const bool last = ((g + 1u) & (gpr - 1u)) == 0u;                // the run's last group (uniform)
        // the run's chunk, f0 / 16 in each of its groups: the run began at a multiple of 16 below fpad, and fpad - F < 16, so it exists
        double *out = chunk_ws + (b * chunks + f0 / BHW_WELCH_FFT_CHUNK) * K;
        // From n_fft 512 on K = 256 j + 1: bin M alone would cost every lane of wave 0 one more trip for lane 0's sake.  It is
        // (Zr - Zi, +0.0) of the word bin 0 reads, so lane 0 adds it aside, by the same expression (fft_split_bin at k = M).
        const bool wide = M >= kFftBlock;
#pragma unroll
        for (uint32_t i = 0; i < kWelchFftMaxAcc - 1u; ++i) {
            const uint32_t k = tid + i * kFftBlock;
            if (wide ? k < M : k <= M) {
                double A = acc[i];
                for (uint32_t s = 0; s < n; ++s) A += welch_fft_q(fft_split_bin(base + (size_t)s * M, tw, k, M));
                if (last) {
                    out[k] = A;
                    A = 0.0;
                }
                acc[i] = A;
            }
        }
        if (wide && tid == 0u) {
            double A = acc_m;
            for (uint32_t s = 0; s < n; ++s) A += welch_fft_q(fft_split_bin(base + (size_t)s * M, tw, M, M));
            if (last) {
                out[M] = A;
                A = 0.0;
            }
            acc_m = A;
        }
    }
};

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_stft_fft_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_welch_fft_direct(BhwCordicCfg cfg, BhwWinCfg win, FftIo a, BhwLenPhase lp, WelchFftAcc wa)
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
    stft_fft_rows(a, FftAccumulate(wa));
}

// Coefficient gathered from a resident table in format FMT (as k_stft_fft_table).
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_welch_fft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, FftIo a,
                                                                BhwLenPhase lp, WelchFftAcc wa)
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
    stft_fft_rows(a, FftAccumulate(wa));
}

struct WelchFftJoin {
    const double *in;          // the sums to add: [(b * n_in + i) * K + k]
    double *out;               // stage 1 with several blocks: [(b * n_out + o) * K + k]
    float *P;
    uint64_t batch, bins, n_fft, n_in, n_out, p_stride;
    double scale;
    uint32_t flags, pad;
};

// Sixteen sums of one (signal, bin) per trip, all loads in flight, added in ascending order; past the last one the last is loaded
// again and not added.  GROUPED: output o adds the inputs 16 o .. 16 o + 15 (the chunks of a block) from +0.0; else every input, the
// lane's sum carried from trip to trip (the blocks of a signal).  FINAL: the sum is A of the contract and P is written.
template <bool GROUPED, bool FINAL>
__global__ __launch_bounds__(256) void k_welch_fft_join(WelchFftJoin a)
{
    constexpr uint32_t U = BHW_WELCH_BLOCK / BHW_WELCH_FFT_CHUNK;      // 16
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.batch * a.n_out * a.bins) return;
    const uint64_t k = i % a.bins, rest = i / a.bins;
    const uint64_t o = rest % a.n_out, b = rest / a.n_out;
    const double *wp = a.in + b * a.n_in * a.bins + k;
    const uint64_t i0 = GROUPED ? o * U : 0, i1 = GROUPED ? (i0 + U < a.n_in ? i0 + U : a.n_in) : a.n_in;
    double A = 0.0;
    for (uint64_t j = i0; j < i1; j += U) {
        double v[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) v[u] = wp[(j + u < i1 ? j + u : i1 - 1u) * a.bins];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
            if (j + u < i1) A += v[u];
    }
    if constexpr (FINAL) {
        const double sk = bhw_psd_doubled(a.flags, k, a.bins, a.n_fft) ? a.scale * 2.0 : a.scale;
        a.P[b * a.p_stride + k] = (float)(A * sk);
    } else {
        a.out[(b * a.n_out + o) * a.bins + k] = A;
    }
}

} // namespace

int bhwk_welch_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwWelchFftPlan &wp, const bhw_stft *s,
                       double scale, uint32_t psd_flags, const float *d_x, float *d_P, double *d_ws, const int32_t *d_table,
                       const BhwLenPhase &lp)
{
    const BhwStftFftPlan &pl = wp.fft;
    if (!pl.rows) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    const FftIo a = fft_io(pl, s, d_x, nullptr);
    WelchFftAcc wa{};
    wa.chunk_ws = d_ws;
    wa.fpad = wp.fpad;
    wa.chunks = wp.chunks;
    wa.gpr = wp.gpr;
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    const int e = with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_welch_fft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp, wa); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_welch_fft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp, wa);
        });
    if (e) return e;
    return bhwk_welch_join(l, d_ws, d_P, s->batch, wp.bins, s->n_fft, wp.chunks, wp.blocks, wp.blocks_grid, wp.join_grid, wp.p_stride, scale,
                           psd_flags);
}

// The join of the chunk sums at d_ws (the block sums follow them), for this unit and bhw_welch_cfft.hip: bhw_internal.h.
int bhwk_welch_join(const BhwLaunch &l, double *d_ws, float *d_P, uint64_t batch, uint64_t bins, uint64_t n_fft, uint64_t chunks,
                    uint64_t blocks, uint64_t blocks_grid, uint64_t join_grid, uint64_t p_stride, double scale, uint32_t psd_flags)
{
    hipStream_t st = (hipStream_t)l.stream;
    WelchFftJoin j{};
    j.in = d_ws;
    j.out = d_ws + batch * chunks * bins;                               // the block sums follow the chunk sums
    j.P = d_P;
    j.batch = batch;
    j.bins = bins;
    j.n_fft = n_fft;
    j.n_in = chunks;
    j.n_out = blocks;
    j.p_stride = p_stride;
    j.scale = scale;
    j.flags = psd_flags;
    const dim3 g1((unsigned)blocks_grid), g2((unsigned)join_grid);
    if (blocks == 1) {
        launch(k_welch_fft_join<true, true>, g1, dim3(256), st, j);
    } else {
        launch(k_welch_fft_join<true, false>, g1, dim3(256), st, j);
        j.in = j.out;
        j.n_in = blocks;
        j.n_out = 1;
        launch(k_welch_fft_join<false, true>, g2, dim3(256), st, j);
    }
    return finish(hipSuccess);
}

int bhwk_welch_join_blocks(const BhwLaunch &l, double *d_ws, uint64_t batch, uint64_t bins, uint64_t chunks, uint64_t blocks,
                           uint64_t blocks_grid)
{
    WelchFftJoin j{};
    j.in = d_ws;
    j.out = d_ws + batch * chunks * bins;
    j.batch = batch;
    j.bins = bins;
    j.n_in = chunks;
    j.n_out = blocks;
    launch(k_welch_fft_join<true, false>, dim3((unsigned)blocks_grid), dim3(256), (hipStream_t)l.stream, j);
    return finish(hipSuccess);
}
