// bhw_frames.hip -- overlapped-frame apply (bhw_apply_frames_device / bhw_apply_frames_from_table): the window over many frames of
// one signal at any hop in one launch, the front end of an STFT or a Welch estimate
//
// Part of the hand-written HIP kernels for gfx950 (MI355X, CDNA4) behind include/bhw.h.  Hot path of the reference: phase
// accumulator -> CORDIC rotation chain (or Taylor LUT) -> weighted N-term cosine sum -> int32 coefficient (SURVEY section 8a
// rows a1-a11), then the multiplier in front of the FFT (int_multNxN_dsp48, src/int_multNxN_dsp48.vhd:102).
//
// Coefficient k is the same in every frame, so a lane computes w[k] once -- by the direct CORDIC chains of k_direct
// (direct_coeff) or by the gather of k_range_combine over a resident table (range_coeff) -- keeps it in a register and applies it to
// a group of G frames:  y[f * y_stride + k * C + c] = low32((x[(f * hop + k) * C + c] * w[k]) >> shift).  The per-coefficient work
// that bounds every other kernel of the library is spread over G frames, and what is left is the x read and the y write.
//   - Workgroup: kFramesBlock lanes, min(N, 256) along k and the rest side by side over frames (windows shorter than 256).
//   - Grid: (N / kx) x (frame groups); bhwp_frames_plan picks G so that about kFramesTargetWg workgroups fill the 256 CUs.
//   - x is read up to ceil(N / hop) times (once per frame that covers it), so it takes default-policy loads, and the frame groups are
//     dispatched in signal order, so the frames that share an x are in flight together.
//   - The frame loop (bhw_frames.h, shared with the float32 kernels of bhw_frames_f32.hip) issues four frames' loads before their
//     stores; two channels move as one 8-byte access when both bases and the stride allow it (FramesArgs.io), else as two 4-byte ones.
#include "bhw_frames.h"

namespace {

// the int32 form of the frame loop's arguments (bhw_frames.h)
struct FramesArgs : FramesIo<int32_t> {};

// Coefficient by the direct CORDIC chains.  FORM 0 / 1: the cordic_full chain of k_direct (T = int32_t, or int64_t where the state
// needs more than 32 bits); FORM 2: the mad-form rotation where it applies (direct_form, the rule bhwk_direct picks k_direct_fast by).
template <int FORM>
__global__ __launch_bounds__(kFramesBlock) void k_frames_direct(BhwCordicCfg cfg, BhwWinCfg win, FramesArgs a)
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
    frames_apply(a, k, threadIdx.x / a.kx, w);
}

// Coefficient gathered from a resident table in format FMT (range_coeff: NT the term-count bound, MODE the rule).  Every lane
// reaches the gather (the escape format resolves marked lanes wave-wide).
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFramesBlock) void k_frames_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, FramesArgs a)
{
    const uint32_t k = blockIdx.x * a.kx + (threadIdx.x & (a.kx - 1u));
    frames_apply(a, k, threadIdx.x / a.kx, range_coeff<FMT, NT, MODE>(cfg, win, table, k));
}

// Windows of any length L (bhw_len.h): the same two sources with coefficient k read at the angles of the length-L phase map.  The
// grid covers ceil(L / kx) * kx lanes along k; the lanes past L apply nothing (the table form still gathers, at k = 0, so that the
// escape format's wave-wide fix is reached by every lane).
template <int FORM>
__global__ __launch_bounds__(kFramesBlock) void k_frames_direct_len(BhwCordicCfg cfg, BhwWinCfg win, FramesArgs a, BhwLenPhase lp)
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
    frames_apply(a, k, threadIdx.x / a.kx, w);
}

template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFramesBlock) void k_frames_table_len(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, FramesArgs a,
                                                                    BhwLenPhase lp)
{
    const uint32_t k = blockIdx.x * a.kx + (threadIdx.x & (a.kx - 1u));
    const bool in = k < lp.len;
    const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
    if (in) frames_apply(a, k, threadIdx.x / a.kx, w);
}

} // namespace

int bhwk_frames(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwFramesPlan &pl, const bhw_frames *f,
                const int32_t *d_x, int32_t *d_y, const int32_t *d_table, const BhwLenPhase *lp)
{
    if (!f->frames) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    FramesArgs a;
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
        c_in, w, d_table, [&](auto D) { launch_phase(k_frames_direct_len<D>, k_frames_direct<D>, lp, grid, block, st, c_in, w, a); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_phase(k_frames_table_len<F, NT, M>, k_frames_table<F, NT, M>, lp, grid, block, st, c, w, tab, a);
        });
}
