// bhw_ola_f32.h -- weighted overlap-add with float32 samples (bhw_overlap_add_f32_device / bhw_overlap_add_f32_from_table), the
// kernels of both translation units: bhw_ola_f32.hip compiles the plain sum, bhw_ola_f32_norm.hip the sum divided by the window
// envelope (BHW_OLA_NORMALIZE), so that the two halves of the instances compile in parallel.
//
// The lane structure of bhw_ola.hip, shared with it through bhw_ola.h: output t = q * hop + r, a lane owns
// one residue r and Q consecutive hops, computes the coefficient w[r + j * hop] once per j -- direct CORDIC chains or the gather over
// a resident table, at the angles of the power-of-two or the length-L phase map -- and turns it into v = fl32(w) * 2^-shift.  With the float32 frame elements y it forms
//     S = sum over the frames f reaching t, in ascending f, of  (double) y * (double) v        (binary64, from +0.0)
//     E = sum over the same frames, in the same order, of  (double) v * (double) v             (NORM only)
// in Q * C (and Q) binary64 registers and stores fl32(S), or fl32(S / E) where E > 0 and +0.0 elsewhere.  Each product is exact in
// binary64 (24 x 24 significand bits), so a fused multiply-add rounds as the separate multiply and add would.
//   - Floating-point addition does not associate, so the order is part of the contract: the j loop runs from the lane's largest j
//     down (frame f = q - j ascends).  Masked elements add (double) 0 * v = +-0, which leaves every sum unchanged: a sum that starts
//     at +0.0 is never -0.0 under round-to-nearest.
//   - The trip count is the wave's largest, with the other lanes masked, so every lane reaches range_coeff together.
//   - y and x keep the nontemporal emit() policy; two channels move as one 8-byte access when both bases and the stride allow it.
//   - A batch of signals (bhw_istft_ola_f32_*) runs in grid z: each workgroup moves y and x once to its signal's rows and outputs
//     (OlaArgsF32's strides); the lane structure does not see the batch, and the one-signal calls run with grid z = 1.
//   - NORM is a template argument, not a run-time branch: the Q extra accumulators of E belong only to the instances that need them,
//     which are compiled for Q <= kOlaQMaxNorm rows (the planner's bound for them) to keep their registers near the plain ones.
#pragma once
#include "bhw_ola.h"

int bhwk_ola_f32_norm(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwOlaPlan &pl, const bhw_ola *o,
                      const float *d_y, float *d_x, const int32_t *d_table, const BhwLenPhase *lp, const BhwOlaBatch &bt);

namespace {

typedef float ola_v2f __attribute__((ext_vector_type(2)));    // one I/Q pair (the nontemporal builtins take native vectors only)

// the float32 form of the overlap-add arguments (bhw_ola.h), with the signals of a batch: the workgroups of grid z = b read the rows
// of signal b from y + b * y_bstride and write its outputs to x + b * x_bstride (a batch beyond kOlaMaxGridZ signals takes several
// launches)
struct OlaArgsF32 : OlaIo<float> {
    uint64_t y_bstride, x_bstride;
};

__device__ __forceinline__ float ola_out(double s, double e)
{
    return e > 0.0 ? (float)(s / e) : 0.0f;
}

// The outputs of this lane.  C = channels, VEC: one 8-byte access per I/Q pair, NORM: divide by the envelope; coeff(k) gives the
// int32 w[k] for k < N (and is called with k = 0 on masked lanes).
template <int C, bool VEC, bool NORM, typename Coeff>
__device__ __forceinline__ void ola_f32_loop(const OlaArgsF32 &a, Coeff coeff)
{
    const uint32_t ty = threadIdx.x / a.rx;
    const OlaLane ln = ola_lane(a);
    const uint64_t r = ln.r;
    const int64_t frames = (int64_t)a.frames;
    constexpr uint32_t QM = NORM ? kOlaQMaxNorm : kOlaQMax;       // rows this instance holds (the plan's Q is at most that)
    const float *ys = a.y + (uint64_t)blockIdx.z * a.y_bstride;     // signal blockIdx.z of the batch
    float *xs = a.x + (uint64_t)blockIdx.z * a.x_bstride;
    for (uint64_t by = blockIdx.y; by < a.row_blocks; by += gridDim.y) {
        const OlaRows rw = ola_rows(a, ln, frames, by, ty);
        const uint64_t u0 = rw.u0;
        const uint32_t nrow = rw.nrow, trip = rw.trip;
        const int64_t qa = rw.qa, jhi = rw.jhi;
        const uint32_t trip_w = wave_max(trip);
        double acc[QM][C];
        double env[NORM ? QM : 1];
#pragma unroll
        for (uint32_t i = 0; i < QM; ++i) {
#pragma unroll
            for (int c = 0; c < C; ++c) acc[i][c] = 0.0;
            if constexpr (NORM) env[i] = 0.0;
        }
        for (uint32_t n = 0; n < trip_w; ++n) {
            const bool act = n < trip;
            const int64_t j = jhi - (int64_t)n;                    // descending j: ascending frames
            const uint32_t k = act ? (uint32_t)(r + (uint64_t)j * a.hop) : 0u;   // < N on active lanes
            const double v = (double)ldexpf((float)coeff(k), -(int)a.shift);
            const int64_t f0 = qa - j;                             // frame of row ia
            float e[QM][C];
            bool okr[QM];
#pragma unroll
            for (uint32_t i = 0; i < QM; ++i) {
                const int64_t f = f0 + (int64_t)i;
                const bool ok = act && i < nrow && f >= 0 && f < frames;
                okr[i] = ok;
                // every lane loads (a masked one the first element of row 0, which a call with count > 0 has) and zeroes what it
                // masked afterwards: a load under the mask would take the conversion into its branch and wait for each load alone
                const uint64_t yi = ok ? (uint64_t)f * a.y_stride + (uint64_t)k * C : 0;
                if constexpr (C == 1) {
                    e[i][0] = __builtin_nontemporal_load(ys + yi);
                } else if constexpr (VEC) {
                    const ola_v2f pr = __builtin_nontemporal_load((const ola_v2f *)(ys + yi));
                    e[i][0] = pr.x;
                    e[i][1] = pr.y;
                } else {
                    e[i][0] = __builtin_nontemporal_load(ys + yi);
                    e[i][1] = __builtin_nontemporal_load(ys + yi + 1);
                }
            }
#pragma unroll
            for (uint32_t i = 0; i < QM; ++i)
#pragma unroll
                for (int c = 0; c < C; ++c) e[i][c] = okr[i] ? e[i][c] : 0.0f;
#pragma unroll
            for (uint32_t i = 0; i < QM; ++i) {
#pragma unroll
                for (int c = 0; c < C; ++c) acc[i][c] += (double)e[i][c] * v;
                if constexpr (NORM) env[i] += okr[i] ? v * v : 0.0;
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < QM; ++i) {
            if (i < nrow) {
                float *xp = xs + (u0 + (uint64_t)i * a.hop) * C;
                float o[C];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    if constexpr (NORM) o[c] = ola_out(acc[i][c], env[i]);
                    else                o[c] = (float)acc[i][c];
                }
                if constexpr (C == 1) {
                    __builtin_nontemporal_store(o[0], xp);
                } else if constexpr (VEC) {
                    __builtin_nontemporal_store(ola_v2f{o[0], o[1]}, (ola_v2f *)xp);
                } else {
                    __builtin_nontemporal_store(o[0], xp);
                    __builtin_nontemporal_store(o[1], xp + 1);
                }
            }
        }
    }
}

template <int IO, bool NORM, typename Coeff>
__device__ __forceinline__ void ola_f32_io(const OlaArgsF32 &a, Coeff coeff)
{
    ola_f32_loop<IO == 0 ? 1 : 2, IO == 2, NORM>(a, coeff);
}

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_ola_direct).
template <int FORM, int IO, bool NORM>
__global__ __launch_bounds__(kOlaBlock) void k_ola_f32_direct(BhwCordicCfg cfg, BhwWinCfg win, OlaArgsF32 a)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    ola_f32_io<IO, NORM>(a, [&](uint32_t k) -> int32_t {
        if constexpr (FORM == 2) return direct_coeff_mad(cfg, win, lut_s, k);
        else                     return direct_coeff<T>(cfg, win, lut_s, k);
    });
}

// Coefficient gathered from a resident table in format FMT (range_coeff); every lane of a wave reaches the gather on every trip.
template <int FMT, int NT, int MODE, int IO, bool NORM>
__global__ __launch_bounds__(kOlaBlock) void k_ola_f32_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, OlaArgsF32 a)
{
    ola_f32_io<IO, NORM>(a, [&](uint32_t k) -> int32_t { return range_coeff<FMT, NT, MODE>(cfg, win, table, k); });
}

// Windows of any length L: the same two sources at the angles of the length-L phase map (OlaArgsF32.n is L).
template <int FORM, int IO, bool NORM>
__global__ __launch_bounds__(kOlaBlock) void k_ola_f32_direct_len(BhwCordicCfg cfg, BhwWinCfg win, OlaArgsF32 a, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    ola_f32_io<IO, NORM>(a, [&](uint32_t k) -> int32_t {
        if constexpr (FORM == 2) return direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
        else                     return direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
    });
}

template <int FMT, int NT, int MODE, int IO, bool NORM>
__global__ __launch_bounds__(kOlaBlock) void k_ola_f32_table_len(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, OlaArgsF32 a,
                                                                  BhwLenPhase lp)
{
    ola_f32_io<IO, NORM>(a, [&](uint32_t k) -> int32_t { return range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, k)); });
}

// The launch of one NORM half (each translation unit instantiates one).
template <bool NORM>
int ola_f32_launch(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwOlaPlan &pl, const bhw_ola *o,
                   const float *d_y, float *d_x, const int32_t *d_table, const BhwLenPhase *lp, const BhwOlaBatch &bt)
{
    if (!o->count || !bt.batch) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    OlaArgsF32 a;
    ola_args(a, pl, o, d_y, d_x);
    a.y_bstride = bt.y_bstride;
    a.x_bstride = bt.x_bstride;
    if (a.io == 2 && bt.batch > 1 && (bt.y_bstride % 2 || bt.x_bstride % 2)) a.io = 1;    // every signal start 8-byte aligned
    // one launch per slab of kOlaMaxGridZ signals, inside the source's callback: the table's form is resolved once
    const dim3 block(kOlaBlock);
    const auto per_slab = [&](auto &&launch_slab) {
        for (uint64_t b0 = 0; b0 < bt.batch; b0 += kOlaMaxGridZ) {
            const uint64_t nb = bt.batch - b0 < kOlaMaxGridZ ? bt.batch - b0 : kOlaMaxGridZ;
            a.y = d_y + b0 * bt.y_bstride;
            a.x = d_x + b0 * bt.x_bstride;
            launch_slab(dim3((unsigned)pl.grid_x, (unsigned)pl.grid_y, (unsigned)nb));
        }
    };
    return with_window_source(
        c_in, w, d_table,
        [&](auto D) {
            with_int_or_last<0, 1, 2>(a.io, [&](auto IO) {
                per_slab([&](dim3 grid) {
                    launch_phase(k_ola_f32_direct_len<D, IO, NORM>, k_ola_f32_direct<D, IO, NORM>, lp, grid, block, st, c_in, w, a);
                });
            });
        },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            with_int_or_last<0, 1, 2>(a.io, [&](auto IO) {
                per_slab([&](dim3 grid) {
                    launch_phase(k_ola_f32_table_len<F, NT, M, IO, NORM>, k_ola_f32_table<F, NT, M, IO, NORM>, lp, grid, block, st, c, w, tab, a);
                });
            });
        });
}

} // namespace
