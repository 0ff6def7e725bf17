// bhw_hold_real.h -- the max-hold / min-hold epilogue of the two fused real-input row functions: one text for bhw_hold_fft.hip (under
// stft_fft_rows of bhw_stft_fft.h) and bhw_hold_mfft.hip (under stft_mfft_rows of bhw_stft_mfft.h).  Contract: include/bhw.h
// (bhw_hold_fft_f32_*, bhw_hold_mfft_f32_*); plans: BhwHoldFftPlan, BhwHoldMfftPlan in bhw_plan.h; reasons: DESIGN.md section 34.
// Include it after the row function's header.  The words, their identities and HoldAcc are bhw_hold.h's, whose text is not touched.
//
// The ownership is the real Welch epilogues' (FftAccumulate of bhw_welch_fft.hip, MfftAccumulate of bhw_welch_mfft.hip), whole: a run
// is max(16, fy) consecutive frames of one signal, a workgroup takes the runs w, w + grid, ... and a run's groups of fy rows in
// ascending order.  The value of (b, f, k), k <= M = n_fft / 2, is h = hold_word(fft_split_bin(...)): the float32 word the forward
// call stores for the bin's power (bhw_spectrogram_f32_*, bhw_stft_mfft_f32_* under BHW_MFFT_POWER), never negative and never -0.0,
// so the words order as the values do and a NaN lies above +inf (bhw_hold.h).  A lane keeps two uint32 per bin, the unsigned maximum
// from 0 and the unsigned minimum from all ones.
//   fy >= 16: the group holds fy / 16 whole chunks; lane i < (fy / 16) * K owns (chunk i / K, bin i % K), reduces the chunk's live
//       slots and stores the pair.  Nothing is carried between groups.
//   fy < 16: lane t owns the bins t, t + 256, ... and carries their pairs over the 16 / fy groups of the run, stores them at its end
//       and resets them to the identities.  Bin M is taken aside on lane 0 where the Welch sibling takes it aside: M >= 256 under
//       stft_fft_rows (POW2: NACC = 9 pairs, the ninth is lane 0's), M a multiple of 256 under stft_mfft_rows (NACC = 8: M is at
//       most 6 * 256 there, so the last pair is free and holds it).
// A slot whose frame is >= F is never read -- its row was formed as zeros, and one such slot would make the minimum 0 -- and a chunk
// that begins at or past F is never stored, so every pair [(b * chunks + c) * K + k] is written exactly once and none outside the
// workspace (tests/cpp/san_hold_real.cpp replays this).  The stores are plain; no atomics.
#pragma once
#include "bhw_hold.h"

namespace {

template <uint32_t NACC, bool POW2>
struct HoldRealAccumulate {
    static constexpr bool kSpectrum = false;                        // read by stft_fft_rows
    static constexpr bool kStore = false;                           // read by stft_mfft_rows
    static constexpr bool kRuns = true;
    uint2 *chunk_ws;
    uint64_t fpad, chunks;
    uint32_t gpr;
    mutable uint32_t hi[NACC], lo[NACC];                            // the bins tid + 256 i; [NACC - 1] is bin M on lane 0 where it is aside

    __device__ __forceinline__ explicit HoldRealAccumulate(const HoldAcc &w) : chunk_ws(w.chunk_ws), fpad(w.fpad), chunks(w.chunks), gpr(w.gpr)
    {
#pragma unroll
        for (uint32_t i = 0; i < NACC; ++i) {
            hi[i] = kHoldWordMax;
            lo[i] = kHoldWordMin;
        }
    }

    // stft_fft_rows' call
    __device__ __forceinline__ void operator()(const FftIo &a, uint32_t M, uint64_t g, uint64_t b, uint64_t f0, const fft_v2f *base,
                                               const fft_v2f *tw) const
    {
        reduce(a.fy, a.frames, M, g, b, f0, base, tw);
    }

    // stft_mfft_rows' call
    template <class Io>
    __device__ __forceinline__ void operator()(const Io &a, uint64_t g, uint64_t b, uint64_t f0, const fft_v2f *base, const fft_v2f *tw) const
    {
        reduce(a.fy, a.frames, a.m, g, b, f0, base, tw);
    }

    // g: the group; b, f0: its signal and the frame of slot 0; base: the transformed points of slot 0
    __device__ __forceinline__ void reduce(uint32_t fy, uint64_t F, uint32_t M, uint64_t g, uint64_t b, uint64_t f0, const fft_v2f *base,
                                           const fft_v2f *tw) const
    {
        const uint32_t K = M + 1u, tid = threadIdx.x;
        if (fy >= BHW_WELCH_FFT_CHUNK) {
            const uint32_t pairs = (fy / BHW_WELCH_FFT_CHUNK) * K;
            for (uint32_t i = tid; i < pairs; i += kFftBlock) {
                const uint32_t c = i / K, k = i - c * K;
                const uint64_t fc = f0 + (uint64_t)c * BHW_WELCH_FFT_CHUNK;
                if (fc >= F) continue;                                  // a chunk of the padding: it has no place in the workspace
                const uint32_t m = F - fc < BHW_WELCH_FFT_CHUNK ? (uint32_t)(F - fc) : BHW_WELCH_FFT_CHUNK;
                const fft_v2f *src = base + (size_t)c * BHW_WELCH_FFT_CHUNK * M;
                uint32_t H = kHoldWordMax, L = kHoldWordMin;
                for (uint32_t s = 0; s < m; ++s) {                      // the live slots only: m >= 1
                    const uint32_t h = hold_word(fft_split_bin(src + (size_t)s * M, tw, k, M));
                    H = h > H ? h : H;
                    L = h < L ? h : L;
                }
                chunk_ws[(b * chunks + fc / BHW_WELCH_FFT_CHUNK) * K + k] = make_uint2(H, L);
            }
            return;
        }
        const uint32_t m = f0 >= F ? 0u : F - f0 < fy ? (uint32_t)(F - f0) : fy;     // the live slots are the first m
        const bool last = ((g + 1u) & (gpr - 1u)) == 0u;                // the run's last group (uniform)
        // the run's chunk, f0 / 16 in each of its groups: the run began at a multiple of 16 below fpad, and fpad - F < 16, so it exists
        // and its first frame is live
        uint2 *out = chunk_ws + (b * chunks + f0 / BHW_WELCH_FFT_CHUNK) * K;
        // K = 256 j + 1: bin M alone would cost every lane of wave 0 one more trip for lane 0's sake, so lane 0 reduces it aside, by
        // the same expression (fft_split_bin at k = M), exactly where the Welch sibling does
        const bool aside = POW2 ? M >= kFftBlock : (M & (kFftBlock - 1u)) == 0u;
#pragma unroll
        for (uint32_t i = 0; i < (POW2 ? NACC - 1u : NACC); ++i) {
            const uint32_t k = tid + i * kFftBlock;
            if (aside ? k < M : k <= M) {
                uint32_t H = hi[i], L = lo[i];
                for (uint32_t s = 0; s < m; ++s) {
                    const uint32_t h = hold_word(fft_split_bin(base + (size_t)s * M, tw, k, M));
                    H = h > H ? h : H;
                    L = h < L ? h : L;
                }
                if (last) {
                    out[k] = make_uint2(H, L);
                    H = kHoldWordMax;
                    L = kHoldWordMin;
                }
                hi[i] = H;
                lo[i] = L;
            }
        }
        if (aside && tid == 0u) {
            uint32_t H = hi[NACC - 1u], L = lo[NACC - 1u];
            for (uint32_t s = 0; s < m; ++s) {
                const uint32_t h = hold_word(fft_split_bin(base + (size_t)s * M, tw, M, M));
                H = h > H ? h : H;
                L = h < L ? h : L;
            }
            if (last) {
                out[M] = make_uint2(H, L);
                H = kHoldWordMax;
                L = kHoldWordMin;
            }
            hi[NACC - 1u] = H;
            lo[NACC - 1u] = L;
        }
    }
};

} // namespace
