// bhw_welch_mfft.hip -- window, mixed-radix real FFT and the frame average in one kernel, for even n_fft = 2^a 3^b 5^c that is no power
// of two (bhw_welch_mfft_f32_device / _from_table; contract: include/bhw.h, plan: BhwWelchMfftPlan in bhw_plan.h, reasons and
// measurements: DESIGN.md section 28).
//
// The row function of bhw_stft_mfft.h with an epilogue that owns runs, as bhw_welch_fft.hip is the power-of-two kernel under one: the
// row, the passes and the split expression are the one text of that header and of bhw_stft_fft.h, so (re, im) of a bin are the
// float32 pair bhw_stft_mfft_f32_* writes for it, and the spectrum never exists.  A run is max(16, fy) consecutive frames of one
// signal on the frame axis padded to whole runs; a workgroup takes the runs w, w + grid, ... and a run's groups of fy rows in
// ascending order.  After the last pass of a group the M transformed points of every slot are in LDS behind the pass's barrier, and
// a lane forms the split bin of ITS bin (fft_split_bin, which takes an odd M) for one slot after the other, in ascending frame order,
// adding q = (double) re * re + (double) im * im into binary64:
//   fy >= 16 (n_fft 18 ... 120): the group holds fy / 16 whole chunks; lane i < (fy / 16) * K owns (chunk i / K, bin i % K), sums the
//       chunk's live slots from +0.0 and stores the chunk sum.  Nothing is carried between groups.
//   fy < 16 (n_fft >= 144): lane t owns the bins t, t + 256, ... <= M (kWelchMfftMaxAcc = 8 at n_fft 4050; at 144 lane t <= 72 owns
//       bin t), adds the group's live slots to its accumulators, carries them over the 16 / fy groups of the run and stores them at
//       its end.  Where M is a multiple of 256 (n_fft 1536, 2560, 3072) bin M would be a trip of its own for lane 0's sake: lane 0
//       adds it aside, by the same expression.
// A slot whose frame is >= F is skipped (its row was formed as zeros and loaded nothing), and a chunk that begins at or past F is
// never stored, so every chunk sum [(b * chunks + c) * K + k] is written exactly once and none outside the workspace
// (tests/cpp/san_welch_mfft.cpp replays this).  The stores are plain; the joins are bhwk_welch_join's (the kernels of
// bhw_welch_fft.hip, bins = K, the call's psd_flags).  No float atomics.
#include "bhw_stft_mfft.h"

namespace {

struct WelchMfftAcc {
    double *chunk_ws;          // [(b * chunks + c) * K + k]
    uint64_t fpad, chunks;     // frames of a signal padded to whole runs; ceil(F / 16)
    uint32_t gpr;              // groups per run: max(1, 16 / fy)
    uint32_t pad;
};

__device__ __forceinline__ double welch_mfft_q(fft_v2f y)
{
    const double re = (double)y.x, im = (double)y.y;
    return __builtin_fma(re, re, im * im);                              // im * im is exact: one rounding, the contract's q_f
}

// The epilogue carries state: one object per lane lives for the whole group loop of stft_mfft_rows, and the sums of a run stay in
// its mutable members from one group's call to the next (bhw_stft_mfft.h says that an epilogue which owns runs may do this).
struct MfftAccumulate {
    static constexpr bool kStore = false;
    static constexpr bool kRuns = true;
    double *chunk_ws;
    uint64_t fpad, chunks;
    uint32_t gpr;
    // The bins tid + 256 i.  Where bin M is taken aside M is at most 6 * 256, so the last accumulator is free and holds it on lane 0.
    mutable double acc[kWelchMfftMaxAcc];

    __device__ __forceinline__ explicit MfftAccumulate(const WelchMfftAcc &w) : chunk_ws(w.chunk_ws), fpad(w.fpad), chunks(w.chunks), gpr(w.gpr)
    {
#pragma unroll
        for (uint32_t i = 0; i < kWelchMfftMaxAcc; ++i) acc[i] = 0.0;
    }

    // g: the group; b, f0: its signal and the frame of slot 0; base: the transformed points of slot 0
    __device__ __forceinline__ void operator()(const MfftIo &a, uint64_t g, uint64_t b, uint64_t f0, const fft_v2f *base, const fft_v2f *tw) const
    {
        const uint32_t M = a.m, K = M + 1u, fy = a.fy, tid = threadIdx.x;
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
                for (uint32_t s = 0; s < n; ++s) A += welch_mfft_q(fft_split_bin(src + (size_t)s * M, tw, k, M));
                chunk_ws[(b * chunks + fc / BHW_WELCH_FFT_CHUNK) * K + k] = A;
            }
            return;
        }
        const uint32_t n = f0 >= F ? 0u : F - f0 < fy ? (uint32_t)(F - f0) : fy;     // the live slots are the first n
        const bool last = ((g + 1u) & (gpr - 1u)) == 0u;                // the run's last group (uniform)
        // the run's chunk, f0 / 16 in each of its groups: the run began at a multiple of 16 below fpad, and fpad - F < 16, so it exists
        double *out = chunk_ws + (b * chunks + f0 / BHW_WELCH_FFT_CHUNK) * K;
        // K = 256 j + 1: bin M alone would cost every lane of wave 0 one more trip for lane 0's sake.  It is (Zr - Zi, +0.0) of the
        // word bin 0 reads, so lane 0 adds it aside, by the same expression (fft_split_bin at k = M).
        const bool aside = (M & (kFftBlock - 1u)) == 0u;
#pragma unroll
        for (uint32_t i = 0; i < kWelchMfftMaxAcc; ++i) {
            const uint32_t k = tid + i * kFftBlock;
            if (aside ? k < M : k <= M) {
                double A = acc[i];
                for (uint32_t s = 0; s < n; ++s) A += welch_mfft_q(fft_split_bin(base + (size_t)s * M, tw, k, M));
                if (last) {
                    out[k] = A;
                    A = 0.0;
                }
                acc[i] = A;
            }
        }
        if (aside && tid == 0u) {
            double A = acc[kWelchMfftMaxAcc - 1u];
            for (uint32_t s = 0; s < n; ++s) A += welch_mfft_q(fft_split_bin(base + (size_t)s * M, tw, M, M));
            if (last) {
                out[M] = A;
                A = 0.0;
            }
            acc[kWelchMfftMaxAcc - 1u] = A;
        }
    }
};

// Without a hint the allocator ends at 129 VGPRs, one above the 128 that four waves of a SIMD share; asked for four waves it finds 128
// with no scratch and no spill in every instance (kernel_resources.json; tests/test_abi.py's standing rule holds it there).
#define BHW_WELCH_MFFT_WAVES __attribute__((amdgpu_waves_per_eu(4, 4)))

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_stft_mfft_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) BHW_WELCH_MFFT_WAVES void k_welch_mfft_direct(BhwCordicCfg cfg, BhwWinCfg win, MfftIo a, BhwLenPhase lp, WelchMfftAcc wa)
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
    stft_mfft_rows(a, MfftAccumulate(wa));
}

// Coefficient gathered from a resident table in format FMT (as k_stft_mfft_table).
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) BHW_WELCH_MFFT_WAVES void k_welch_mfft_table(BhwCordicCfg cfg, BhwWinCfg win,
                                                                                      const void *__restrict__ table, MfftIo a, BhwLenPhase lp,
                                                                                      WelchMfftAcc wa)
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
    stft_mfft_rows(a, MfftAccumulate(wa));
}

} // namespace

int bhwk_welch_mfft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwWelchMfftPlan &wp, const bhw_stft *s,
                        double scale, uint32_t psd_flags, const float *d_x, float *d_P, double *d_ws, const int32_t *d_table,
                        const BhwLenPhase &lp)
{
    const BhwStftMfftPlan &pl = wp.fft;
    if (!pl.rows) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    const MfftIo a = mfft_io(pl, s, d_x, nullptr);
    WelchMfftAcc wa{};
    wa.chunk_ws = d_ws;
    wa.fpad = wp.fpad;
    wa.chunks = wp.chunks;
    wa.gpr = wp.gpr;
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    const int e = with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_welch_mfft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp, wa); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_welch_mfft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp, wa);
        });
    if (e) return e;
    return bhwk_welch_join(l, d_ws, d_P, s->batch, wp.bins, s->n_fft, wp.chunks, wp.blocks, wp.blocks_grid, wp.join_grid, wp.p_stride, scale,
                           psd_flags);
}
