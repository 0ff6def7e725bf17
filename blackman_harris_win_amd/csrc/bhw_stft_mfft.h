// bhw_stft_mfft.h -- the body shared by the kernels that form a windowed real row of an even n_fft = 2^a 3^b 5^c that is no power of
// two and transform it in LDS: bhw_stft_mfft.hip (stores the spectrum row, its powers or their fold through a filter bank) and
// bhw_welch_mfft.hip (adds the powers over the frames of a run: DESIGN.md section 28).  The row function is a template on the
// epilogue -- what happens to the transformed row -- and everything before it is one text for both units.  Moving the body here left
// the instruction streams of k_stft_mfft_direct<*> and k_stft_mfft_table<*> unchanged.
//
// The workgroup of bhw_stft_fft.h -- 256 lanes own whole rows, the window through LDS into the lane's registers, the twiddle table
// W[k] = exp(-2 pi i k / n_fft), k < n_fft / 2, by binary64 sincospi, the row loaded, detrended and windowed by the same steps -- with
// three differences:
//   - a lane's last column need not exist: cpl = ceil(n_fft / lpf), and c * lpf + l < n_fft is the column test behind the cols mask;
//   - the passes are a generic Stockham pass of radix r in {5, 3, 4, 2} at sub-transform length Ns over M = n_fft / 2 complex points:
//     butterfly i < M / r reads src[i + q * M / r] (consecutive lanes, consecutive 8-byte words), multiplies by W at the EXACT index
//     q * k * (n_fft / (r Ns)), k = i mod Ns (r Ns divides M; indices >= n_fft / 2 fold by W[i + n_fft / 2] = -W[i] with a compare),
//     and writes dst[(i - k) * r + k + q * Ns].  A lane loops i = l, l + lpf, ...: a pass may leave lanes idle or take two trips.
//     i mod Ns is one float multiply: floor((i + 0.5) * (1 / Ns)) is the quotient for every i, Ns < 2^11 (the distance of
//     (i + 0.5) / Ns from an integer is at least 0.5 / Ns, the float error below 2^-10.9 / Ns; tests/cpp/san_stft_mfft.cpp replays it);
//   - the epilogue.  MfftStore: the output form is a uniform runtime branch after ONE evaluation of the split pass (fft_split_bin's
//     arithmetic; M may be odd): the spectrum pair, its power fl32((double) re^2 + (double) im^2), or the powers kept in the slot's
//     idle Stockham buffer and folded through the bank exactly as bhw_spectrogram.hip does, every lane reaching the barrier in between.
// A row's arithmetic does not depend on its slot, its group or the grid.
#pragma once
#include "bhw_stft_fft.h"

namespace {

struct MfftIo {
    const float *x;
    float *Y;
    uint64_t rows, frames, hop, samples, pad;
    uint64_t x_stride, y_stride, y_bstride;
    uint64_t groups;
    uint32_t n_fft, m, col0, len;
    uint32_t lpf, fy, cpl, passes;
    uint32_t sched;                       // the radix of pass p in bits 4p .. 4p + 3
    uint32_t shift, reflect, detrend;
    uint32_t form;                        // BHWP_MFFT_SPECTRUM, _POWER, _BANK
    const uint32_t *first, *offset;       // the bank (form BHWP_MFFT_BANK)
    const float *weight;
    uint32_t filters, weights;
};

// The Io of a launch from the plan and the descriptor, without a bank (bhwk_stft_mfft_f32 adds it); the Welch and hold plans
// carry zero y strides and form BHWP_MFFT_SPECTRUM.
inline MfftIo mfft_io(const BhwStftMfftPlan &pl, const bhw_stft *s, const float *d_x, float *d_Y)
{
    MfftIo a{};
    a.x = d_x;
    a.Y = d_Y;
    a.rows = pl.rows;
    a.frames = s->frames;
    a.hop = s->hop;
    a.samples = s->samples;
    a.pad = s->pad;
    a.x_stride = pl.x_stride;
    a.y_stride = pl.y_stride;
    a.y_bstride = pl.y_bstride;
    a.groups = pl.groups;
    a.n_fft = (uint32_t)s->n_fft;
    a.m = pl.m;
    a.col0 = (uint32_t)s->col0;
    a.len = (uint32_t)pl.len;
    a.lpf = pl.lpf;
    a.fy = pl.fy;
    a.cpl = pl.cpl;
    a.passes = pl.passes;
    for (uint32_t p = 0; p < pl.passes; ++p) a.sched |= (uint32_t)pl.radix[p] << (4u * p);
    a.shift = s->shift;
    a.reflect = s->pad_mode == BHW_PAD_REFLECT ? 1u : 0u;
    a.detrend = pl.detrend ? 1u : 0u;
    a.form = pl.form;
    return a;
}

// W at index idx < n_fft (table of M = n_fft / 2 entries, W[idx + M] = -W[idx]); M is no power of two: a compare, not a mask
__device__ __forceinline__ fft_v2f mfft_twiddle(const fft_v2f *tw, uint32_t idx, uint32_t M)
{
    const bool hi = idx >= M;
    const fft_v2f w = tw[hi ? idx - M : idx];
    return hi ? fft_v2f{-w.x, -w.y} : w;
}

// float32 roundings of binary64 values
constexpr float kSin3 = (float)0.86602540378443864676;      // sin(2 pi / 3)
constexpr float kCos5a = (float)0.30901699437494742410;     // cos(2 pi / 5)
constexpr float kCos5b = (float)-0.80901699437494742410;    // cos(4 pi / 5)
constexpr float kSin5a = (float)0.95105651629515357212;     // sin(2 pi / 5)
constexpr float kSin5b = (float)0.58778525229247312917;     // sin(4 pi / 5)

// X[q] = sum over j of a[j] exp(-2 pi i j q / R), in place
template <uint32_t R>
__device__ __forceinline__ void mfft_butterfly(fft_v2f (&a)[R])
{
    if constexpr (R == 2) {
        const fft_v2f a0 = a[0], a1 = a[1];
        a[0] = a0 + a1;
        a[1] = a0 - a1;
    } else if constexpr (R == 3) {
        const fft_v2f t1 = a[1] + a[2], d = a[1] - a[2];
        const fft_v2f t2 = a[0] - 0.5f * t1, t3 = kSin3 * d;
        a[0] = a[0] + t1;
        a[1] = fft_v2f{t2.x + t3.y, t2.y - t3.x};                  // t2 - i t3
        a[2] = fft_v2f{t2.x - t3.y, t2.y + t3.x};                  // t2 + i t3
    } else if constexpr (R == 4) {
        const fft_v2f t0 = a[0] + a[2], t1 = a[0] - a[2], t2 = a[1] + a[3];
        const fft_v2f t3 = fft_v2f{a[1].y - a[3].y, a[3].x - a[1].x};   // -i (a1 - a3)
        a[0] = t0 + t2;
        a[1] = t1 + t3;
        a[2] = t0 - t2;
        a[3] = t1 - t3;
    } else {
        static_assert(R == 5, "radix");
        const fft_v2f b1 = a[1] + a[4], b2 = a[2] + a[3], d1 = a[1] - a[4], d2 = a[2] - a[3];
        const fft_v2f m1 = a[0] + kCos5a * b1 + kCos5b * b2, m2 = a[0] + kCos5b * b1 + kCos5a * b2;
        const fft_v2f n1 = kSin5a * d1 + kSin5b * d2, n2 = kSin5b * d1 - kSin5a * d2;
        a[0] = a[0] + b1 + b2;
        a[1] = fft_v2f{m1.x + n1.y, m1.y - n1.x};                  // m1 - i n1
        a[4] = fft_v2f{m1.x - n1.y, m1.y + n1.x};
        a[2] = fft_v2f{m2.x + n2.y, m2.y - n2.x};                  // m2 - i n2
        a[3] = fft_v2f{m2.x - n2.y, m2.y + n2.x};
    }
}

// One Stockham pass of radix R over the slot's M points: Q = M / R butterflies, sub-transform length Ns, ts = n_fft / (R Ns).
template <uint32_t R>
__device__ __forceinline__ void mfft_pass(const fft_v2f *src, fft_v2f *dst, const fft_v2f *tw, uint32_t M, uint32_t Q, uint32_t Ns, uint32_t ts,
                                          uint32_t l, uint32_t lpf)
{
    const float inv = __builtin_amdgcn_rcpf((float)Ns);
    for (uint32_t i = l; i < Q; i += lpf) {
        fft_v2f a[R];
#pragma unroll
        for (uint32_t q = 0; q < R; ++q) a[q] = src[i + q * Q];
        uint32_t k = i;                                                 // the last pass: Ns = Q
        if (Ns < Q) k = i - (uint32_t)(((float)i + 0.5f) * inv) * Ns;   // i mod Ns
        if (Ns > 1u) {
            const uint32_t kt = k * ts;
#pragma unroll
            for (uint32_t q = 1; q < R; ++q) a[q] = cmul(a[q], mfft_twiddle(tw, q * kt, M));
        }
        mfft_butterfly<R>(a);
        const uint32_t o = (i - k) * R + k;
#pragma unroll
        for (uint32_t q = 0; q < R; ++q) dst[o + q * Ns] = a[q];
    }
}

// fl32 of the binary64 re^2 + im^2: both squares are exact, the sum rounds once
__device__ __forceinline__ float mfft_power(fft_v2f y)
{
    const double re = (double)y.x, im = (double)y.y;
    return (float)(re * re + im * im);
}

// What happens to a transformed row is the epilogue, a template parameter of the row function.  MfftStore, the epilogue of
// bhw_stft_mfft_f32_*, is a tag: its text (the split pass once and the three output forms) stands in the row function itself under
// `if constexpr`, where it stood before the function was shared, so that the compiled forward kernels keep their instructions (the
// reason bhw_stft_fft.h gives for FftStoreSpectrum).
//
// An epilogue with kRuns true owns RUNS instead of strided groups of the flat row pool (bhw_welch_mfft.hip): the frame axis of every
// signal is padded to epilogue.fpad frames, a run is epilogue.gpr (a power of two) consecutive groups of one signal, workgroup w
// takes the runs w, w + grid, ... and a run's groups in ascending order; a row with f >= frames is not live: it loads nothing and
// its row is zeros.  It is called once per group by every lane, after the last pass's barrier, as epilogue(a, g, b, f0, base, tw):
// the group, its signal, the frame of slot 0, the transformed points of slot 0 (slot s at base + s * M) and the twiddle table.  Such
// an epilogue may carry state from group to group in `mutable` members, on the terms bhw_stft_fft.h states: one object per lane
// lives for the whole group loop, and the calls of a run's groups come in ascending order with nothing of another run between them.
//
// An epilogue with a member kRows (kStore and kRuns false) keeps the flat pool and takes each transformed row itself
// (bhw_logspec_mfft.hip): it is called by every lane of the workgroup, live or not, after the last pass's barrier, as
// epilogue(a, lpf, live, b, f, l, src, dst, tw): the slot's transformed points in src, its idle buffer dst.  It is stateless and may
// hold barriers that every lane reaches.
struct MfftStore {
    static constexpr bool kStore = true;
    static constexpr bool kRuns = false;
};

template <class E, class = void>
struct mfft_takes_rows : std::false_type {};
template <class E>
struct mfft_takes_rows<E, std::void_t<decltype(E::kRows)>> : std::true_type {};

template <class E>
__device__ __forceinline__ uint64_t mfft_first_group(const E &e)
{
    if constexpr (E::kRuns) return (uint64_t)blockIdx.x * e.gpr;
    else                    return blockIdx.x;
}

template <class E>
__device__ __forceinline__ uint64_t mfft_next_group(const E &e, uint64_t g)
{
    if constexpr (E::kRuns) return ((g + 1u) & (e.gpr - 1u)) ? g + 1u : g + 1u + (uint64_t)(gridDim.x - 1u) * e.gpr;
    else                    return g + gridDim.x;
}

// Everything after the prologue's coefficients: vbuf = buffer A viewed as floats holds v[0..n_fft).
template <class Epilogue>
__device__ __forceinline__ void stft_mfft_rows(const MfftIo &a, const Epilogue &epilogue)
{
    const uint32_t M = a.m, n = a.n_fft, lpf = a.lpf, fy = a.fy;
    fft_v2f *bufA = (fft_v2f *)fft_lds;
    fft_v2f *bufB = bufA + (size_t)fy * M;
    fft_v2f *tw = bufB + (size_t)fy * M;
    float *mean_s = (float *)(tw + M);
    const uint32_t tid = threadIdx.x;
    const uint32_t slot = tid / lpf, l = tid - slot * lpf;
    // the twiddle table
    for (uint32_t k = tid; k < M; k += kFftBlock) {
        double sn, cs;
        sincospi((double)k * 2.0 / (double)n, &sn, &cs);
        tw[k] = fft_v2f{(float)cs, (float)-sn};
    }
    // bit c of cols: the lane has a column c (c * lpf + l < n_fft: the last one may be missing); of wins: it is a window column
    uint32_t cols = 0, wins = 0;
#pragma unroll
    for (uint32_t c = 0; c < kFftMaxCpl; ++c) {
        const uint32_t j = c * lpf + l;
        if (c < a.cpl && j < n) {
            cols |= 1u << c;
            if (j - a.col0 < a.len) wins |= 1u << c;                   // unsigned: a window column
        }
    }
    // the lane's coefficients
    float v[kFftMaxCpl];
    {
        const float *vbuf = (const float *)bufA;
#pragma unroll
        for (uint32_t c = 0; c < kFftMaxCpl; ++c) v[c] = ((cols >> c) & 1u) ? vbuf[c * lpf + l] : 0.0f;
    }
    __syncthreads();
    const uint32_t wave = tid >> 6, lane = tid & 63u;
    const uint64_t T = a.samples;
    float *rowA = (float *)bufA + (size_t)slot * n;               // the slot's row as floats = its M complex points
    for (uint64_t g = mfft_first_group(epilogue); g < a.groups; g = mfft_next_group(epilogue, g)) {
        bool live;
        uint64_t b, f;
        [[maybe_unused]] uint64_t f0 = 0;
        if constexpr (Epilogue::kRuns) {
            const uint64_t r0 = g * fy;                                // fpad is a multiple of fy: a group never crosses a signal
            b = r0 / epilogue.fpad;
            f0 = r0 - b * epilogue.fpad;
            live = f0 + slot < a.frames;
            f = live ? f0 + slot : 0;
        } else {
            const uint64_t r = g * fy + slot;
            live = r < a.rows;
            b = live ? r / a.frames : 0;
            f = live ? r - b * a.frames : 0;
        }
        const float *xb = a.x + b * a.x_stride;
        const uint64_t t0 = f * a.hop + l - a.pad;                     // the (wrapped) time of column l
        asm volatile("" : "+v"(cols), "+v"(wins));
        const uint32_t take = live ? wins : 0u;
        float e[kFftMaxCpl];
#pragma unroll
        for (uint32_t c = 0; c < kFftMaxCpl; ++c) {
            e[c] = 0.0f;
            if ((take >> c) & 1u) {
                uint64_t t = t0 + c * lpf;                             // unsigned: t < T is the whole interior test
                bool zero = false;
                if (t >= T) {
                    const int64_t ts = (int64_t)t;
                    if (a.reflect) t = ts < 0 ? (uint64_t)(-ts) : 2 * (T - 1) - t;
                    else {
                        t = 0;
                        zero = true;
                    }
                }
                const float xv = xb[t];
                e[c] = zero ? 0.0f : xv;
            }
        }
        if (a.detrend) {
            // the raw row (col0 0: column j is sample j), then one wave per row: the order of k_welch_mean
#pragma unroll
            for (uint32_t c = 0; c < kFftMaxCpl; ++c)
                if ((cols >> c) & 1u) rowA[c * lpf + l] = e[c];
            __syncthreads();
            for (uint32_t s = wave; s < fy; s += kFftBlock / 64u) {
                const float *row = (const float *)bufA + (size_t)s * n;
                double P = 0.0;
                for (uint32_t j = lane; j < a.len; j += 64u) P += (double)row[j];
#pragma unroll
                for (int sh = 32; sh >= 1; sh >>= 1) P += __shfl_down(P, sh, 64);
                if (lane == 0) mean_s[s] = (float)(P / (double)a.len);
            }
            __syncthreads();
            const float mu = mean_s[slot];
#pragma unroll
            for (uint32_t c = 0; c < kFftMaxCpl; ++c)
                if ((cols >> c) & 1u) {
                    const float d = e[c] - mu;
                    rowA[c * lpf + l] = ((take >> c) & 1u) ? d * v[c] : 0.0f;
                }
        } else {
#pragma unroll
            for (uint32_t c = 0; c < kFftMaxCpl; ++c)
                if ((cols >> c) & 1u) rowA[c * lpf + l] = ((take >> c) & 1u) ? e[c] * v[c] : 0.0f;
        }
        __syncthreads();
        // the passes: Ns the product of the radices so far, rest = M / (Ns * r) after this pass, so n_fft / (r Ns) = 2 * rest
        fft_v2f *src = bufA + (size_t)slot * M, *dst = bufB + (size_t)slot * M;
        uint32_t Ns = 1, rest = M;
        for (uint32_t p = 0; p < a.passes; ++p) {
            const uint32_t rdx = (a.sched >> (4u * p)) & 15u;
            if (rdx == 5u) {
                rest /= 5u;
                mfft_pass<5>(src, dst, tw, M, M / 5u, Ns, 2u * rest, l, lpf);
            } else if (rdx == 3u) {
                rest /= 3u;
                mfft_pass<3>(src, dst, tw, M, M / 3u, Ns, 2u * rest, l, lpf);
            } else if (rdx == 4u) {
                rest >>= 2;
                mfft_pass<4>(src, dst, tw, M, M >> 2, Ns, 2u * rest, l, lpf);
            } else {
                rest >>= 1;
                mfft_pass<2>(src, dst, tw, M, M >> 1, Ns, 2u * rest, l, lpf);
            }
            __syncthreads();
            fft_v2f *sw = src;
            src = dst;
            dst = sw;
            Ns *= rdx;
        }
        if constexpr (Epilogue::kStore) {
            // the split pass, once, and the output form; dst is the slot's idle buffer now
            float *out = a.Y + b * a.y_bstride + f * a.y_stride;
            float *pw = (float *)dst;                                   // the slot's K powers in bank form (K <= n_fft floats)
            if (live) {
                for (uint32_t k = l; k <= M; k += lpf) {
                    const fft_v2f y = fft_split_bin(src, tw, k, M);
                    if (a.form == BHWP_MFFT_SPECTRUM) ((fft_v2f *)out)[k] = y;
                    else if (a.form == BHWP_MFFT_POWER) out[k] = mfft_power(y);
                    else pw[k] = mfft_power(y);
                }
            }
            if (a.form == BHWP_MFFT_BANK) {
                __syncthreads();                                        // every lane: the form is uniform, outside `live`
                if (live) {
                    const uint32_t K = M + 1u, W = a.weights;
                    for (uint32_t m = l; m < a.filters; m += lpf) {
                        uint32_t o0 = a.offset[m], o1 = a.offset[m + 1u];
                        o0 = o0 < W ? o0 : W;
                        o1 = o1 < W ? o1 : W;
                        o1 = o1 < o0 ? o0 : o1;
                        const uint32_t k0 = a.first[m];
                        uint32_t c = o1 - o0;
                        const uint32_t room = k0 < K ? K - k0 : 0u;           // a band stops at bin K
                        c = c < room ? c : room;
                        double acc = 0.0;
                        for (uint32_t i = 0; i < c; ++i) acc = fma((double)pw[k0 + i], (double)a.weight[o0 + i], acc);
                        out[m] = (float)acc;
                    }
                }
            }
        } else if constexpr (mfft_takes_rows<Epilogue>::value) {
            epilogue(a, lpf, live, b, f, l, src, dst, tw);
        } else {
            epilogue(a, g, b, f0, src - (size_t)slot * M, tw);
        }
        __syncthreads();                                                // the next group overwrites both buffers
    }
}

} // namespace
