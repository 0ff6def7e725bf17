// bhw_hold.h -- the max-hold / min-hold epilogue of the two fused I/Q row functions: one text for bhw_hold_cfft.hip (under
// stft_cfft_rows of bhw_stft_cfft.h) and bhw_hold_cmfft.hip (under stft_cmfft_rows of bhw_stft_cmfft.h).  Contract: include/bhw.h
// (bhw_hold_cfft_f32_*, bhw_hold_cmfft_f32_*); plans: BhwHoldCfftPlan, BhwHoldCmfftPlan in bhw_plan.h; reasons: DESIGN.md section 33.
// Include it after the row function's header.
//
// The ownership is the Welch epilogues' (bhw_welch_cfft.hip, bhw_welch_cmfft.hip), whole: a run is max(16, fy) consecutive frames of
// one signal, a workgroup takes the runs w, w + grid, ... and a run's groups of fy rows in ascending order.  What differs is the value
// and the reduction.  The value of (b, f, k) is h = fl32((double) re^2 + (double) im^2), the float32 word the forward call stores
// under BHW_CFFT_POWER (the products are exact in binary64, so the expression has one binary64 and one float32 rounding however it
// is contracted).  h is never negative and never -0.0, so the WORDS of two values order as unsigned integers exactly as the values
// do, +inf above every finite one and every NaN (of either sign) above +inf.  A lane therefore keeps two uint32 per bin: the
// unsigned maximum from 0 and the unsigned minimum from all ones, the identities -- not zero: a min-hold that began at 0.0 would
// stay there.  No order of reduction changes a maximum, so there is nothing to pin as the Welch sums pin theirs, and a NaN is
// carried up in the maximum by the integer compare where v_max_f32 would drop it; the output kernel copies it to the minimum.
//   fy >= 16: the group holds fy / 16 whole chunks; lane i < (fy / 16) * n owns (chunk i / n, bin i % n), reduces the chunk's live
//       slots and stores the pair.  Nothing is carried between groups.
//   fy < 16: lane t owns the bins t, t + 256, ... < n (at most kHoldMaxAcc = 8: 16 registers), reduces the group's live slots into
//       its pairs, carries them over the 16 / fy groups of the run and stores them at its end.
// A slot whose frame is >= F is skipped -- its row was formed as zeros, and one such slot would make the minimum 0 -- and a chunk
// that begins at or past F is never stored, so every pair [(b * chunks + c) * n + j] is written exactly once and none outside the
// workspace (tests/cpp/san_hold_iq.cpp replays this).  Under BHW_CFFT_SHIFT bin k goes to column k + n / 2, less n where that
// reaches n, HERE, so the joins see columns only.  The stores are plain; no atomics.
#pragma once

// Registers: the allocator takes what launch_bounds(256) allows (123 registers under stft_cfft_rows, 127 under stft_cmfft_rows,
// occupancy 4, no scratch), as it does for the Welch kernels.  Asked for the forward kernels' occupancy of 5 waves per SIMD with
// amdgpu_waves_per_eu(5) it keeps 96 registers and spills 24 / 36 of them to 100 / 116 bytes of scratch: the eight unrolled pairs and
// their eight bin tests live across the row function's whole group loop.  So there is no hint.

namespace {

typedef float hold_v2f __attribute__((ext_vector_type(2)));         // cfft_v2f and fft_v2f are this type

struct HoldAcc {
    uint2 *chunk_ws;           // [(b * chunks + c) * n + j]: x the maximum's word, y the minimum's
    uint64_t fpad, chunks;     // frames of a signal padded to whole runs; ceil(F / 16)
    uint32_t gpr;              // groups per run: max(1, 16 / fy)
    uint32_t pad;
};

constexpr uint32_t kHoldWordMax = 0u, kHoldWordMin = 0xFFFFFFFFu;   // the identities of the two reductions

__device__ __forceinline__ uint32_t hold_word(hold_v2f y)
{
    const double re = (double)y.x, im = (double)y.y;
    return __float_as_uint((float)(re * re + im * im));
}

__device__ __forceinline__ uint32_t hold_col(uint32_t k, uint32_t turn, uint32_t n)
{
    const uint32_t j = k + turn;
    return j >= n ? j - n : j;
}

// Io: CfftIo or CmfftIo (n, fy, binshift and frames are read).  The epilogue carries state as the Welch epilogues do: one object per
// lane lives for the whole group loop of the row function.
template <class Io>
struct HoldAccumulate {
    static constexpr bool kStore = false;
    static constexpr bool kRuns = true;
    uint2 *chunk_ws;
    uint64_t fpad, chunks;
    uint32_t gpr;
    mutable uint32_t hi[kHoldMaxAcc], lo[kHoldMaxAcc];              // the bins tid + 256 i below n

    __device__ __forceinline__ explicit HoldAccumulate(const HoldAcc &w) : chunk_ws(w.chunk_ws), fpad(w.fpad), chunks(w.chunks), gpr(w.gpr)
    {
#pragma unroll
        for (uint32_t i = 0; i < kHoldMaxAcc; ++i) {
            hi[i] = kHoldWordMax;
            lo[i] = kHoldWordMin;
        }
    }

    // g: the group; b, f0: its signal and the frame of slot 0; base: the transformed points of slot 0
    __device__ __forceinline__ void operator()(const Io &a, uint64_t g, uint64_t b, uint64_t f0, const hold_v2f *base) const
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
                const hold_v2f *src = base + (size_t)c * BHW_WELCH_FFT_CHUNK * n + k;
                uint32_t H = kHoldWordMax, L = kHoldWordMin;
                for (uint32_t s = 0; s < m; ++s) {                      // the live slots only: m >= 1
                    const uint32_t h = hold_word(src[(size_t)s * n]);
                    H = h > H ? h : H;
                    L = h < L ? h : L;
                }
                chunk_ws[(b * chunks + fc / BHW_WELCH_FFT_CHUNK) * n + hold_col(k, turn, n)] = make_uint2(H, L);
            }
            return;
        }
        const uint32_t m = f0 >= F ? 0u : F - f0 < fy ? (uint32_t)(F - f0) : fy;     // the live slots are the first m
        const bool last = ((g + 1u) & (gpr - 1u)) == 0u;                // the run's last group (uniform)
        // the run's chunk, f0 / 16 in each of its groups: the run began at a multiple of 16 below fpad, and fpad - F < 16, so it exists
        // and its first frame is live
        uint2 *out = chunk_ws + (b * chunks + f0 / BHW_WELCH_FFT_CHUNK) * n;
#pragma unroll
        for (uint32_t i = 0; i < kHoldMaxAcc; ++i) {
            const uint32_t k = tid + i * kFftBlock;
            if (k < n) {
                uint32_t H = hi[i], L = lo[i];
                for (uint32_t s = 0; s < m; ++s) {
                    const uint32_t h = hold_word(base[(size_t)s * n + k]);
                    H = h > H ? h : H;
                    L = h < L ? h : L;
                }
                if (last) {
                    out[hold_col(k, turn, n)] = make_uint2(H, L);
                    H = kHoldWordMax;
                    L = kHoldWordMin;
                }
                hi[i] = H;
                lo[i] = L;
            }
        }
    }
};

} // namespace
