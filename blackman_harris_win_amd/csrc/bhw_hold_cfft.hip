// bhw_hold_cfft.hip -- window, complex FFT and the max-hold / min-hold traces over the frames in one kernel for interleaved I/Q input
// (bhw_hold_cfft_f32_device / _from_table; contract: include/bhw.h, plan: BhwHoldCfftPlan in bhw_plan.h, reasons and measurements:
// DESIGN.md section 33), and the join of both hold families (bhwk_hold_join, also launched by bhw_hold_cmfft.hip).
//
// The row function of bhw_stft_cfft.h, unedited, under the epilogue of bhw_hold.h: the row and the passes are the one text of that
// header, so the power of a bin is the float32 word bhw_stft_cfft_f32_* writes for it under BHW_CFFT_POWER, and the (B, F, n_fft)
// powers never exist.  The kernels below are k_welch_cfft_direct / _table of bhw_welch_cfft.hip with that epilogue in place of the
// binary64 sums.
#include "bhw_stft_cfft.h"
#include "bhw_hold.h"

namespace {

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_stft_cfft_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_hold_cfft_direct(BhwCordicCfg cfg, BhwWinCfg win, CfftIo a, BhwLenPhase lp, HoldAcc wa)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vbuf = (float *)cfft_lds;
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
    stft_cfft_rows(a, HoldAccumulate<CfftIo>(wa));
}

// Coefficient gathered from a resident table in format FMT (as k_stft_cfft_table).
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_hold_cfft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, CfftIo a,
                                                                BhwLenPhase lp, HoldAcc wa)
{
    float *vbuf = (float *)cfft_lds;
    for (uint32_t j0 = 0; j0 < a.n; j0 += kFftBlock) {
        const uint32_t j = j0 + threadIdx.x;
        const uint32_t k = j - a.col0;
        const bool in = j < a.n && k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (j < a.n) vbuf[j] = in ? fft_coeff(w, a.shift) : 0.0f;
    }
    __syncthreads();
    stft_cfft_rows(a, HoldAccumulate<CfftIo>(wa));
}

struct HoldJoin {
    const uint2 *in;           // the pairs to reduce: [(b * n_in + i) * bins + j]
    uint2 *out;                // stage 1 with several blocks: [(b * n_out + o) * bins + j]
    float *pmax, *pmin;        // either may be NULL: that trace is not written
    uint64_t batch, bins, n_fft, n_in, n_out, p_stride;
    double scale;
    uint32_t flags, pad;       // bhw_psd's flags: the one-sided doubling of the real-input calls; 0 for I/Q
};

// Sixteen pairs of one (signal, column) per trip, all loads in flight; past the last one the last is loaded again, which changes
// neither a maximum nor a minimum.  GROUPED: output o reduces the inputs 16 o .. 16 o + 15 (the chunks of a block); else every input
// (the blocks of a signal).  FINAL: the traces are written, scaled by k_welch_fft_join's very factor (`scale` alone under flags 0); a
// maximum that is a NaN (its word lies above +inf's) is the minimum too.
template <bool GROUPED, bool FINAL>
__global__ __launch_bounds__(256) void k_hold_join(HoldJoin a)
{
    constexpr uint32_t U = BHW_WELCH_BLOCK / BHW_WELCH_FFT_CHUNK;      // 16
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.batch * a.n_out * a.bins) return;
    const uint64_t j = i % a.bins, rest = i / a.bins;
    const uint64_t o = rest % a.n_out, b = rest / a.n_out;
    const uint2 *wp = a.in + b * a.n_in * a.bins + j;
    const uint64_t i0 = GROUPED ? o * U : 0, i1 = GROUPED ? (i0 + U < a.n_in ? i0 + U : a.n_in) : a.n_in;
    uint32_t H = kHoldWordMax, L = kHoldWordMin;
    for (uint64_t c = i0; c < i1; c += U) {
        uint2 v[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) v[u] = wp[(c + u < i1 ? c + u : i1 - 1u) * a.bins];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            H = v[u].x > H ? v[u].x : H;
            L = v[u].y < L ? v[u].y : L;
        }
    }
    if constexpr (FINAL) {
        if (H > 0x7F800000u) L = H;                                     // some frame's power was a NaN: both traces are
        const double sk = bhw_psd_doubled(a.flags, j, a.bins, a.n_fft) ? a.scale * 2.0 : a.scale;
        if (a.pmax) a.pmax[b * a.p_stride + j] = (float)((double)__uint_as_float(H) * sk);
        if (a.pmin) a.pmin[b * a.p_stride + j] = (float)((double)__uint_as_float(L) * sk);
    } else {
        a.out[(b * a.n_out + o) * a.bins + j] = make_uint2(H, L);
    }
}

} // namespace

int bhwk_hold_cfft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwHoldCfftPlan &hp, const bhw_stft *s,
                       double scale, const float *d_x, float *d_max, float *d_min, void *d_ws, const int32_t *d_table,
                       const BhwLenPhase &lp)
{
    const BhwWelchCfftPlan &wp = hp.welch;
    const BhwStftCfftPlan &pl = wp.fft;
    if (!pl.rows) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    const CfftIo a = cfft_io(pl, s, d_x, nullptr);
    HoldAcc wa{};
    wa.chunk_ws = (uint2 *)d_ws;
    wa.fpad = wp.fpad;
    wa.chunks = wp.chunks;
    wa.gpr = wp.gpr;
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    const int e = with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_hold_cfft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp, wa); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_hold_cfft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp, wa);
        });
    if (e) return e;
    return bhwk_hold_join(l, d_ws, d_max, d_min, s->batch, wp.bins, s->n_fft, wp.chunks, wp.blocks, wp.blocks_grid, wp.join_grid, wp.p_stride,
                          scale, 0u);
}

// The join of the chunk pairs at d_ws (the block pairs follow them), for this unit, bhw_hold_cmfft.hip, bhw_hold_fft.hip and
// bhw_hold_mfft.hip: bhw_internal.h.
int bhwk_hold_join(const BhwLaunch &l, void *d_ws, float *d_max, float *d_min, uint64_t batch, uint64_t bins, uint64_t n_fft,
                   uint64_t chunks, uint64_t blocks, uint64_t blocks_grid, uint64_t join_grid, uint64_t p_stride, double scale,
                   uint32_t psd_flags)
{
    hipStream_t st = (hipStream_t)l.stream;
    HoldJoin j{};
    j.in = (const uint2 *)d_ws;
    j.out = (uint2 *)d_ws + batch * chunks * bins;                      // the block pairs follow the chunk pairs
    j.pmax = d_max;
    j.pmin = d_min;
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
        launch(k_hold_join<true, true>, g1, dim3(256), st, j);
    } else {
        launch(k_hold_join<true, false>, g1, dim3(256), st, j);
        j.in = j.out;
        j.n_in = blocks;
        j.n_out = 1;
        launch(k_hold_join<false, true>, g2, dim3(256), st, j);
    }
    return finish(hipSuccess);
}
