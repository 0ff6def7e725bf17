// bhw_welch_sums.hip -- the window sums of a spectrum scaling (bhw_window_sums_device / _from_table): s1 = sum u[k] and s2 = sum u[k]^2
// over the window of length L, u = w or (int64) fl32(w), as exact integers, without storing the window.
//
// Lane g of the grid takes k = g, g + lanes, g + 2 * lanes, ... (the same trip count in every lane: the table gather is wave-wide, a
// lane past L gathers k = 0 and adds nothing) and keeps four 64-bit integers: s1, the sums of the low and of the high 32 bits of u^2
// (u^2 <= 2^62; L <= 2^30 keeps either sum below 2^62: no 128-bit arithmetic on the device) and the count.  The wave folds them with
// shuffles, the workgroup through LDS, and lane 0 adds the four results to the output words with 64-bit integer atomics.  Integer
// sums: exact in any order.  The four words are cleared by a memset on the same stream in front of the launch.
#include "bhw_device.h"

namespace {

struct SumsArgs {
    unsigned long long *out;      // { s1, sum lo32(u^2), sum hi32(u^2), count }
    uint64_t len, stride;         // L; lanes of the grid
    uint32_t trips, f32;
};

struct SumsAcc {
    unsigned long long s1 = 0, lo = 0, hi = 0, n = 0;            // s1 in two's complement: wrapping adds are exact mod 2^64
};

__device__ __forceinline__ void sums_add(SumsAcc &acc, int32_t w, bool f32)
{
    const int64_t u = f32 ? (int64_t)(float)w : (int64_t)w;      // |u| <= 2^31
    const uint64_t q = (uint64_t)(u * u);                        // <= 2^62
    acc.s1 += (unsigned long long)u;
    acc.lo += q & 0xFFFFFFFFull;
    acc.hi += q >> 32;
    acc.n += 1;
}

__device__ __forceinline__ void sums_finish(const SumsArgs &a, SumsAcc acc)
{
    __shared__ unsigned long long part[kSumsBlock / 64][4];
    unsigned long long v[4] = {acc.s1, acc.lo, acc.hi, acc.n};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) v[i] += __shfl_down(v[i], s, 64);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) part[wave][i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long t = 0;
#pragma unroll
        for (uint32_t wv = 0; wv < kSumsBlock / 64; ++wv) t += part[wv][threadIdx.x];
        atomicAdd(a.out + threadIdx.x, t);
    }
}

template <int FORM>
__global__ __launch_bounds__(kSumsBlock) void k_window_sums_direct(BhwCordicCfg cfg, BhwWinCfg win, SumsArgs a, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    const uint64_t g = (uint64_t)blockIdx.x * kSumsBlock + threadIdx.x;
    SumsAcc acc;
    for (uint32_t n = 0; n < a.trips; ++n) {
        const uint64_t k = g + (uint64_t)n * a.stride;
        if (k < a.len) {
            int32_t w;
            if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
            else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
            sums_add(acc, w, a.f32 != 0);
        }
    }
    sums_finish(a, acc);
}

template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kSumsBlock) void k_window_sums_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, SumsArgs a,
                                                                   BhwLenPhase lp)
{
    const uint64_t g = (uint64_t)blockIdx.x * kSumsBlock + threadIdx.x;
    SumsAcc acc;
    for (uint32_t n = 0; n < a.trips; ++n) {
        const uint64_t k = g + (uint64_t)n * a.stride;
        const bool in = k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (in) sums_add(acc, w, a.f32 != 0);
    }
    sums_finish(a, acc);
}

} // namespace

int bhwk_window_sums(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwSumsPlan &pl, uint32_t flags,
                     const int32_t *d_table, const BhwLenPhase &lp, uint64_t *d_sums)
{
    hipStream_t st = (hipStream_t)l.stream;
    const hipError_t e = hipMemsetAsync(d_sums, 0, 4 * sizeof(uint64_t), st);          // a memset node under capture
    if (e != hipSuccess) return (int)e;
    SumsArgs a;
    a.out = (unsigned long long *)d_sums;
    a.len = pl.len;
    a.stride = (uint64_t)pl.grid * kSumsBlock;
    a.trips = pl.trips;
    a.f32 = (flags & BHW_SUMS_F32) ? 1u : 0u;
    const dim3 grid(pl.grid), block(kSumsBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) { launch(k_window_sums_direct<D>, grid, block, st, c_in, w, a, lp); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch(k_window_sums_table<F, NT, M>, grid, block, st, c, w, tab, a, lp);
        });
}
