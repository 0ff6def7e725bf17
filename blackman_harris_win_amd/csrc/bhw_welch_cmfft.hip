// bhw_welch_cmfft.hip -- window, mixed-radix complex FFT and the frame average in one kernel for interleaved I/Q input at
// n_fft = 2^a 3^b 5^c that is no power of two, odd lengths included (bhw_welch_cmfft_f32_device / _from_table; contract:
// include/bhw.h, plan: BhwWelchCmfftPlan in bhw_plan.h, reasons and measurements: DESIGN.md section 32).
//
// The row function of bhw_stft_cmfft.h with an epilogue that owns runs, as bhw_welch_cfft.hip is the power-of-two kernel under one:
// the row and the passes are the one text of that header, so (re, im) of a bin are the float32 pair bhw_stft_cmfft_f32_* writes for
// it, and the spectrum never exists.  A run is max(16, fy) consecutive frames of one signal on the frame axis padded to whole runs; a
// workgroup takes the runs w, w + grid, ... and a run's groups of fy rows in ascending order.  After the last pass of a group the
// transformed points of every slot are in LDS behind the pass's barrier -- a bin's power is the point itself, there is no split
// expression -- and a lane adds q = (double) re * re + (double) im * im into binary64, one slot after the other in ascending frame
// order:
//   fy >= 16 (n_fft 18 ... 64: fy 32 or 16): the group holds fy / 16 whole chunks; lane i < (fy / 16) * n owns (chunk i / n, bin
//       i % n), sums the chunk's live slots from +0.0 and stores the chunk sum.  Nothing is carried between groups.  n is no power of
//       two: i / n is a division.
//   fy < 16 (n_fft >= 65: fy 8, 4, 2, 1): lane t owns the bins t, t + 256, ... < n (kWelchCmfftMaxAcc = 8 at n_fft 2025; below 256
//       some lanes own none), adds the group's live slots to its accumulators, carries them over the 16 / fy groups of the run and
//       stores them at its end.
// A slot whose frame is >= F is skipped (its row was formed as zeros and loaded nothing), and a chunk that begins at or past F is
// never stored, so every chunk sum [(b * chunks + c) * n + j] is written exactly once and none outside the workspace
// (tests/cpp/san_welch_cmfft.cpp replays this).  Under BHW_CFFT_SHIFT bin k goes to column j = k + n / 2, less n where that reaches
// n (integer division, a compare and a subtract: an odd n follows fftshift) HERE, where the chunk sum is stored, so the joins
// (bhwk_welch_join: the kernels of bhw_welch_fft.hip, bins = n, nothing doubled) see columns only.  The stores are plain; no float
// atomics.
#include "bhw_stft_cmfft.h"

namespace {

struct WelchCmfftAcc {
    double *chunk_ws;          // [(b * chunks + c) * n + j]
    uint64_t fpad, chunks;     // frames of a signal padded to whole runs; ceil(F / 16)
    uint32_t gpr;              // groups per run: max(1, 16 / fy)
    uint32_t pad;
};

__device__ __forceinline__ double welch_cmfft_q(fft_v2f y)
{
    const double re = (double)y.x, im = (double)y.y;
    return __builtin_fma(re, re, im * im);                              // im * im is exact: one rounding, the contract's q_f
}

// bin k's column: k, or shifted (turn = n / 2) k + n / 2 mod n
__device__ __forceinline__ uint32_t welch_cmfft_col(uint32_t k, uint32_t turn, uint32_t n)
{
    const uint32_t j = k + turn;
    return j >= n ? j - n : j;
}

// The epilogue carries state: one object per lane lives for the whole group loop of stft_cmfft_rows, and the sums of a run stay in
// its mutable members from one group's call to the next (bhw_stft_cmfft.h says that an epilogue which owns runs may do this).
struct CmfftAccumulate {
    static constexpr bool kStore = false;
    static constexpr bool kRuns = true;
    double *chunk_ws;
    uint64_t fpad, chunks;
    uint32_t gpr;
    mutable double acc[kWelchCmfftMaxAcc];         // the bins tid + 256 i below n

    __device__ __forceinline__ explicit CmfftAccumulate(const WelchCmfftAcc &w) : chunk_ws(w.chunk_ws), fpad(w.fpad), chunks(w.chunks), gpr(w.gpr)
    {
#pragma unroll
        for (uint32_t i = 0; i < kWelchCmfftMaxAcc; ++i) acc[i] = 0.0;
    }

    // g: the group; b, f0: its signal and the frame of slot 0; base: the transformed points of slot 0
    __device__ __forceinline__ void operator()(const CmfftIo &a, uint64_t g, uint64_t b, uint64_t f0, const fft_v2f *base) const
    {
        const uint32_t n = a.n, fy = a.fy, tid = threadIdx.x;
        const uint32_t turn = a.binshift ? n >> 1 : 0u;
        const uint64_t F = a.frames;
        if (fy >= BHW_WELCH_FFT_CHUNK) {
            const uint32_t pairs = (fy / BHW_WELCH_FFT_CHUNK) * n;
            for (uint32_t i = tid; i < pairs; i += kFftBlock) {
                const uint32_t c = i / n, k = i - c * n;
                const uint64_t fc = f0 + (uint64_t)c * BHW_WELCH_FFT_CHUNK;
                if (fc >= F) continue;                                  // a chunk of the padding: it has no place in the workspace
                const uint32_t m = F - fc < BHW_WELCH_FFT_CHUNK ? (uint32_t)(F - fc) : BHW_WELCH_FFT_CHUNK;
                const fft_v2f *src = base + (size_t)c * BHW_WELCH_FFT_CHUNK * n + k;
                double A = 0.0;
                for (uint32_t s = 0; s < m; ++s) A += welch_cmfft_q(src[(size_t)s * n]);
                chunk_ws[(b * chunks + fc / BHW_WELCH_FFT_CHUNK) * n + welch_cmfft_col(k, turn, n)] = A;
            }
            return;
        }
        const uint32_t m = f0 >= F ? 0u : F - f0 < fy ? (uint32_t)(F - f0) : fy;     // the live slots are the first m
        const bool last = ((g + 1u) & (gpr - 1u)) == 0u;                // the run's last group (uniform)
        // the run's chunk, f0 / 16 in each of its groups: the run began at a multiple of 16 below fpad, and fpad - F < 16, so it exists
        double *out = chunk_ws + (b * chunks + f0 / BHW_WELCH_FFT_CHUNK) * n;
#pragma unroll
        for (uint32_t i = 0; i < kWelchCmfftMaxAcc; ++i) {
            const uint32_t k = tid + i * kFftBlock;
            if (k < n) {
                double A = acc[i];
                for (uint32_t s = 0; s < m; ++s) A += welch_cmfft_q(base[(size_t)s * n + k]);
                if (last) {
                    out[welch_cmfft_col(k, turn, n)] = A;
                    A = 0.0;
                }
                acc[i] = A;
            }
        }
    }
};

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_stft_cmfft_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_welch_cmfft_direct(BhwCordicCfg cfg, BhwWinCfg win, CmfftIo a, BhwLenPhase lp, WelchCmfftAcc wa)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vbuf = (float *)fft_lds;
    for (uint32_t j = threadIdx.x; j < a.n; j += kFftBlock) {
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
    stft_cmfft_rows(a, CmfftAccumulate(wa));
}

// Coefficient gathered from a resident table in format FMT (as k_stft_cmfft_table).
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_welch_cmfft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, CmfftIo a,
                                                                  BhwLenPhase lp, WelchCmfftAcc wa)
{
    float *vbuf = (float *)fft_lds;
    for (uint32_t j0 = 0; j0 < a.n; j0 += kFftBlock) {
        const uint32_t j = j0 + threadIdx.x;
        const uint32_t k = j - a.col0;
        const bool in = j < a.n && k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (j < a.n) vbuf[j] = in ? fft_coeff(w, a.shift) : 0.0f;
    }
    __syncthreads();
    stft_cmfft_rows(a, CmfftAccumulate(wa));
}

} // namespace

int bhwk_welch_cmfft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwWelchCmfftPlan &wp, const bhw_stft *s,
                         double scale, const float *d_x, float *d_P, double *d_ws, const int32_t *d_table, const BhwLenPhase &lp)
{
    const BhwStftCmfftPlan &pl = wp.fft;
    if (!pl.rows) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    const CmfftIo a = cmfft_io(pl, s, d_x, nullptr);
    WelchCmfftAcc wa{};
    wa.chunk_ws = d_ws;
    wa.fpad = wp.fpad;
    wa.chunks = wp.chunks;
    wa.gpr = wp.gpr;
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    const int e = with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_welch_cmfft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp, wa); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_welch_cmfft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp, wa);
        });
    if (e) return e;
    // the chunk sums hold columns: bins = n_fft, nothing doubled
    return bhwk_welch_join(l, d_ws, d_P, s->batch, wp.bins, s->n_fft, wp.chunks, wp.blocks, wp.blocks_grid, wp.join_grid, wp.p_stride,
                           scale, 0u);
}
