// bhw_ola.hip -- weighted overlap-add (bhw_overlap_add_device / bhw_overlap_add_from_table): every frame multiplied by the window
// again and the overlapping frames summed back into one signal in one launch, the synthesis side of an STFT
//
// Part of the hand-written HIP kernels for gfx950 (MI355X, CDNA4) behind include/bhw.h.  The transpose of bhw_frames.hip: there
// each output depends on one coefficient, here output t sums up to ceil(N / hop) products, each with its own coefficient:
//     x[t] = low32((sum over frames f of  y[f * y_stride + (t - f * hop) * C + c] * w[t - f * hop]) >> shift)
// Write t = q * hop + r.  A lane owns one residue r and a block of Q consecutive hops q; for each j it computes w[r + j * hop] once
// -- by the direct CORDIC chains (direct_coeff / direct_coeff_mad) or by the gather over a resident table (range_coeff) -- and adds
// y[(q - j) * y_stride + (r + j * hop) * C + c] * w into Q * C int64 registers, then shifts and stores the Q outputs.  Every element
// of y is read once, every output written once, and the coefficient work per output is (frames reaching it) / Q.
//   - Workgroup: kOlaBlock lanes, rx along the residue (consecutive outputs and frame elements in a wave) and fy = kOlaBlock / rx
//     side by side over rows of Q hops (hops shorter than 256).  Lane s is numbered from t0: it holds the residue of t0 + s.
//   - Grid: ceil(min(hop, count) / rx) x (row blocks); bhwp_ola_plan picks Q so that about kOlaTargetWg workgroups fill the 256
//     CUs; row blocks past kOlaMaxGridY take a grid-stride loop.
//   - The j loop of a lane covers only the frames that exist for its rows (the first and last frames of a call reach fewer
//     outputs); its trip count is the wave's largest, with the other lanes masked, so every lane reaches range_coeff together.
//   - y and x are single-use streams: nontemporal loads and stores (the emit() policy); two channels move as one 8-byte access when
//     both bases and the stride allow it (OlaArgs.io), else as two 4-byte ones.
#include "bhw_ola.h"

namespace {

typedef int ola_v2i __attribute__((ext_vector_type(2)));      // one I/Q pair (the nontemporal builtins take native vectors only)

// the int32 form of the overlap-add arguments (bhw_ola.h)
struct OlaArgs : OlaIo<int32_t> {};

// The outputs of this lane.  C = channels, VEC: one 8-byte access per I/Q pair; coeff(k) gives w[k] for k < N (and is called
// with k = 0 on masked lanes).
template <int C, bool VEC, typename Coeff>
__device__ __forceinline__ void ola_loop(const OlaArgs &a, Coeff coeff)
{
    const uint32_t ty = threadIdx.x / a.rx;
    const uint64_t s = (uint64_t)blockIdx.x * a.rx + (threadIdx.x & (a.rx - 1u));
    const bool lane_ok = s < a.lanes;
    uint64_t r = a.r0 + s;                                         // s < hop: at most one wrap
    int64_t qb = (int64_t)a.q0;
    if (r >= a.hop) {
        r -= a.hop;
        ++qb;
    }
    const int64_t jr = (!lane_ok || r >= a.n) ? 0 : (r < a.rlim ? a.jmax : a.jmax - 1);   // frames reaching this residue: j < jr
    const int64_t frames = (int64_t)a.frames;
    for (uint64_t by = blockIdx.y; by < a.row_blocks; by += gridDim.y) {
        const uint64_t ia = (by * a.fy + ty) * a.q;                // first row (hop index relative to t0) of this lane
        // rows of this lane with an output u = i * hop + s inside [0, count): a prefix of the Q rows (ia < rows keeps ia * hop
        // below count whatever the hop)
        const uint64_t u0 = ia < a.rows ? ia * a.hop + s : a.count;
        uint32_t nrow = 0;
        if (lane_ok && u0 < a.count) {
            const uint64_t left = (a.count - u0 - 1) / a.hop + 1;
            nrow = left < a.q ? (uint32_t)left : a.q;
        }
        // frames that reach these rows: f = qb + i - j in [0, frames), j in [0, jr)
        const int64_t qa = qb + (int64_t)ia;
        const int64_t jlo = qa - frames + 1 > 0 ? qa - frames + 1 : 0;
        const int64_t jhi = (qa + (int64_t)nrow - 1) < jr - 1 ? qa + (int64_t)nrow - 1 : jr - 1;
        const uint32_t trip = (nrow && jhi >= jlo) ? (uint32_t)(jhi - jlo + 1) : 0u;
        const uint32_t trip_w = wave_max(trip);
        int64_t acc[kOlaQMax][C];
#pragma unroll
        for (uint32_t i = 0; i < kOlaQMax; ++i)
#pragma unroll
            for (int c = 0; c < C; ++c) acc[i][c] = 0;
        for (uint32_t n = 0; n < trip_w; ++n) {
            const bool act = n < trip;
            const int64_t j = jlo + (int64_t)n;
            const uint32_t k = act ? (uint32_t)(r + (uint64_t)j * a.hop) : 0u;   // < N on active lanes
            const int64_t w = coeff(k);
            const int64_t f0 = qa - j;                             // frame of row ia
            int32_t v[kOlaQMax][C];
#pragma unroll
            for (uint32_t i = 0; i < kOlaQMax; ++i) {
                const int64_t f = f0 + (int64_t)i;
                const bool ok = act && i < nrow && f >= 0 && f < frames;
                const uint64_t yi = ok ? (uint64_t)f * a.y_stride + (uint64_t)k * C : 0;
                if constexpr (C == 1) {
                    v[i][0] = ok ? __builtin_nontemporal_load(a.y + yi) : 0;
                } else if constexpr (VEC) {
                    ola_v2i pr = {0, 0};
                    if (ok) pr = __builtin_nontemporal_load((const ola_v2i *)(a.y + yi));
                    v[i][0] = pr.x;
                    v[i][1] = pr.y;
                } else {
                    v[i][0] = ok ? __builtin_nontemporal_load(a.y + yi) : 0;
                    v[i][1] = ok ? __builtin_nontemporal_load(a.y + yi + 1) : 0;
                }
            }
#pragma unroll
            for (uint32_t i = 0; i < kOlaQMax; ++i)
#pragma unroll
                for (int c = 0; c < C; ++c) acc[i][c] += (int64_t)v[i][c] * w;   // masked elements are 0; the sum wraps mod 2^64
        }
#pragma unroll
        for (uint32_t i = 0; i < kOlaQMax; ++i) {
            if (i < nrow) {
                int32_t *xp = a.x + (u0 + (uint64_t)i * a.hop) * C;
                if constexpr (C == 1) {
                    __builtin_nontemporal_store((int32_t)(acc[i][0] >> a.shift), xp);
                } else if constexpr (VEC) {
                    __builtin_nontemporal_store(ola_v2i{(int32_t)(acc[i][0] >> a.shift), (int32_t)(acc[i][1] >> a.shift)}, (ola_v2i *)xp);
                } else {
                    __builtin_nontemporal_store((int32_t)(acc[i][0] >> a.shift), xp);
                    __builtin_nontemporal_store((int32_t)(acc[i][1] >> a.shift), xp + 1);
                }
            }
        }
    }
}

// IO (OlaArgs.io) is a template argument of the kernels: with the three access forms in one kernel its registers are those of the
// widest, and the escape format's wave-wide fix no longer stays in registers.
template <int IO, typename Coeff>
__device__ __forceinline__ void ola_io(const OlaArgs &a, Coeff coeff)
{
    ola_loop<IO == 0 ? 1 : 2, IO == 2>(a, coeff);
}

// Coefficient by the direct CORDIC chains, as k_frames_direct: FORM 0 / 1 the cordic_full chain of k_direct (T = int32_t, or int64_t
// where the state needs more than 32 bits), FORM 2 the mad-form rotation where it applies (direct_form).
template <int FORM, int IO>
__global__ __launch_bounds__(kOlaBlock) void k_ola_direct(BhwCordicCfg cfg, BhwWinCfg win, OlaArgs a)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    ola_io<IO>(a, [&](uint32_t k) -> int32_t {
        if constexpr (FORM == 2) return direct_coeff_mad(cfg, win, lut_s, k);
        else                     return direct_coeff<T>(cfg, win, lut_s, k);
    });
}

// Coefficient gathered from a resident table in format FMT (range_coeff: NT the term-count bound, MODE the rule).  Every lane of
// a wave reaches the gather on every trip (the escape format resolves marked lanes wave-wide).
template <int FMT, int NT, int MODE, int IO>
__global__ __launch_bounds__(kOlaBlock) void k_ola_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, OlaArgs a)
{
    ola_io<IO>(a, [&](uint32_t k) -> int32_t { return range_coeff<FMT, NT, MODE>(cfg, win, table, k); });
}

// Windows of any length L (bhw_len.h): the same two sources with coefficient k read at the angles of the length-L phase map (OlaArgs.n
// is L, so the frames that reach a residue and the coefficients a lane takes are those of the length-L window).
template <int FORM, int IO>
__global__ __launch_bounds__(kOlaBlock) void k_ola_direct_len(BhwCordicCfg cfg, BhwWinCfg win, OlaArgs a, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    ola_io<IO>(a, [&](uint32_t k) -> int32_t {
        if constexpr (FORM == 2) return direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
        else                     return direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
    });
}

template <int FMT, int NT, int MODE, int IO>
__global__ __launch_bounds__(kOlaBlock) void k_ola_table_len(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, OlaArgs a,
                                                              BhwLenPhase lp)
{
    ola_io<IO>(a, [&](uint32_t k) -> int32_t { return range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, k)); });
}

} // namespace

int bhwk_ola(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwOlaPlan &pl, const bhw_ola *o,
             const int32_t *d_y, int32_t *d_x, const int32_t *d_table, const BhwLenPhase *lp)
{
    if (!o->count) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    OlaArgs a;
    ola_args(a, pl, o, d_y, d_x);
    const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y), block(kOlaBlock);
    return with_window_source(
        c_in, w, d_table,
        [&](auto D) {
            with_int_or_last<0, 1, 2>(a.io, [&](auto IO) {
                launch_phase(k_ola_direct_len<D, IO>, k_ola_direct<D, IO>, lp, grid, block, st, c_in, w, a);
            });
        },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            with_int_or_last<0, 1, 2>(a.io, [&](auto IO) {
                launch_phase(k_ola_table_len<F, NT, M, IO>, k_ola_table<F, NT, M, IO>, lp, grid, block, st, c, w, tab, a);
            });
        });
}
