// bhw_mask_fft.hip -- window, real FFT, a real gain per bin, inverse real FFT, window and overlap-add in one kernel
// (bhw_mask_fft_f32_device / _from_table; contract: include/bhw.h, plan: BhwMaskFftPlan in bhw_plan.h, reasons: DESIGN.md section 41).
// The same kernel with a complex gain per bin: bhw_cmask_fft_f32_device / _from_table, k_cmask_fft_* below.
// The same kernel over n_ch channels summed behind their gains: bhw_beam_fft_f32_device / _from_table, k_beam_fft_* (section 45).
//
// The span / ring / flush kernel of bhw_istft_fft.hip (istft_fft_spans in bhw_istft_fft.h) with another frame source: where that
// kernel loads the bins Y[k], Y[M - k] of a frame from memory, this one forms them in LDS from the signal.  Prologue, once per
// workgroup: the window coefficients v[0..L) as the inverse kernels keep them, and TWO twiddle tables of M = n_fft / 2 entries, the
// inverse one exp(+2 pi i k / n_fft) and behind it the forward one exp(-2 pi i k / n_fft), both from the same binary64 sincospi.
// Then, per frame f of a slot (MaskSource::frame):
//   a. lane l takes the columns j = l, l + lpf, ... of the row: sample t = f * hop + j - pad of the signal under the padding rule of
//      bhw_stft_fft.h (reflect, or +0.0 in place of the sample), times v[j - col0]; +0.0 outside the window and in a slot without a
//      frame.  The float row goes to the slot's buffer A; one barrier;
//   b. the forward passes of bhw_stft_fft.h, the same text reading the forward table;
//   c. the lane of k <= M / 2 forms Y[k] and Y[M - k] by fft_split_bin, multiplies each by its gain (one float32 rounding per part,
//      never contracted into the adds that follow), forms Z[k] and Z[M - k] by the pre-split of bhw_istft_fft.h and writes them to the
//      slot's OTHER buffer: the split reads src[k], src[M - k] and src[0] of the transformed points, which no lane overwrites.
// The inverse passes, the ring and the flush follow as they stand.  The bits of a masked row are those bhw_stft_fft_f32_* stores,
// times the gains; the bits of an output those bhw_istft_fft_f32_* gives for these rows.
//
// tests/cpp/san_mask_fft.cpp replays a., the gain reads of c. and the buffer each phase writes from a copy of its own; an edit of
// MaskSource::frame is an edit of the replay too.
#include "bhw_istft_fft.h"

namespace {

// Steps a. and b. of a frame source, one text for MaskSourceT and BeamSource below.
// a. the windowed row of frame f of the signal at xb, into `row` (the caller's barrier follows)
__device__ __forceinline__ void mask_fft_row(const IfftIo &a, bool act, const float *xb, uint64_t samples, uint64_t pad, uint64_t hop,
                                             uint32_t reflect, uint64_t f, uint32_t l, const float *vS, float *row)
{
    const uint32_t n = a.n_fft, lpf = a.lpf;
    const uint64_t T = samples, t0 = f * hop - pad;              // the (wrapped) time of column 0
    for (uint32_t j = l; j < n; j += lpf) {
        const uint32_t k = j - a.col0;                           // unsigned: k < L is the window test
        float r = 0.0f;
        if (act && k < a.len) {
            uint64_t t = t0 + j;                                 // unsigned: t < T is the whole interior test
            bool zero = false;
            if (t >= T) {
                const int64_t ts = (int64_t)t;
                if (reflect) t = ts < 0 ? (uint64_t)(-ts) : 2 * (T - 1) - t;
                else {
                    t = 0;
                    zero = true;
                }
            }
            const float xv = xb[t];
            r = (zero ? 0.0f : xv) * vS[k];
        }
        row[j] = r;
    }
}

// b. the forward passes over the forward table twf: the transformed points end in src
__device__ __forceinline__ void mask_fft_forward(const IfftIo &a, uint32_t l, const fft_v2f *twf, fft_v2f *&src, fft_v2f *&dst)
{
    const uint32_t M = a.m, lpf = a.lpf, H = M >> 1, Q = M >> 2;
    uint32_t Ns = 1;
    for (uint32_t p = 0; p < a.radix4; ++p) {
        const uint32_t ts = M / (2u * Ns);                           // n_fft / (4 Ns)
        for (uint32_t i = l; i < Q; i += lpf) {
            const uint32_t k = i & (Ns - 1u);
            fft_v2f a0 = src[i], a1 = src[i + Q], a2 = src[i + 2u * Q], a3 = src[i + 3u * Q];
            if (Ns > 1u) {
                const uint32_t kt = k * ts;
                a1 = cmul(a1, twiddle(twf, kt, M));
                a2 = cmul(a2, twiddle(twf, 2u * kt, M));
                a3 = cmul(a3, twiddle(twf, 3u * kt, M));
            }
            const fft_v2f t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3;
            const fft_v2f t3 = fft_v2f{a1.y - a3.y, a3.x - a1.x};   // -i (a1 - a3)
            const uint32_t o = ((i - k) << 2) + k;
            dst[o] = t0 + t2;
            dst[o + Ns] = t1 + t3;
            dst[o + 2u * Ns] = t0 - t2;
            dst[o + 3u * Ns] = t1 - t3;
        }
        __syncthreads();
        fft_v2f *sw = src;
        src = dst;
        dst = sw;
        Ns <<= 2;
    }
    if (a.radix2) {                                                  // Ns = M / 2: k = i, twiddle W_M^i = W[2 i]
        for (uint32_t i = l; i < H; i += lpf) {
            const fft_v2f a0 = src[i], a1 = cmul(src[i + H], twf[2u * i]);
            dst[i] = a0 + a1;
            dst[i + H] = a0 - a1;
        }
        __syncthreads();
        fft_v2f *sw = src;
        src = dst;
        dst = sw;
    }
}

// G, the gain of a bin: float (bhw_mask_fft_f32_*) or the pair fft_v2f (gr, gi) (bhw_cmask_fft_f32_*).  g points to G and the two gain
// strides count G, so step c. loads gp[k] ascending and gp[M - k] descending as 4-byte words or as 8-byte pairs from the one text of
// frame(); masked() is overloaded on G.  tests/cpp/san_cmask.cpp replays the pair reads.
template <typename G>
struct MaskSourceT {
    static constexpr bool kBins = false;
    static constexpr uint32_t kTables = 2;
    static constexpr uint32_t kMaxCpl = 8;                            // n_fft <= 2048: 16 columns per lane come with 4096 only
    const float *x;
    const G *g;
    uint64_t samples, pad, hop, x_stride, g_stride, g_bstride;
    uint32_t reflect;

    __device__ __forceinline__ void tables(fft_v2f *twf, uint32_t k, double cs, double sn) const { twf[k] = fft_v2f{(float)cs, (float)-sn}; }

    // the masked bin: one rounding per part, whatever is added to it afterwards
    static __device__ __forceinline__ fft_v2f masked(fft_v2f y, float gain)
    {
#pragma clang fp contract(off)
        return fft_v2f{y.x * gain, y.y * gain};
    }
    // by a pair (gr, gi): four products, each rounded on its own, then one subtraction and one addition (include/bhw.h)
    static __device__ __forceinline__ fft_v2f masked(fft_v2f y, fft_v2f gain)
    {
#pragma clang fp contract(off)
        const float rr = y.x * gain.x, ii = y.y * gain.y, ri = y.x * gain.y, ir = y.y * gain.x;
        return fft_v2f{rr - ii, ri + ir};
    }

    __device__ __forceinline__ void frame(const IfftIo &a, bool act, uint64_t b, uint64_t f, uint32_t l, const fft_v2f *tw, const float *vS,
                                          fft_v2f *&src, fft_v2f *&dst) const
    {
        const uint32_t M = a.m, lpf = a.lpf, H = M >> 1;
        const fft_v2f *twf = tw + M;
        mask_fft_row(a, act, x + b * x_stride, samples, pad, hop, reflect, f, l, vS, (float *)src);   // a.
        __syncthreads();
        mask_fft_forward(a, l, twf, src, dst);                                                          // b.
        // c. the split, the gains and the pre-split, into the other buffer
        if (act) {
            const G *gp = g + b * g_bstride + f * g_stride;
            for (uint32_t k = l; k <= H; k += lpf) {
#pragma clang fp contract(off)
                const fft_v2f A = masked(fft_split_bin(src, twf, k, M), gp[k]);
                const fft_v2f B = masked(fft_split_bin(src, twf, M - k, M), gp[M - k]);
                if (k == 0u) dst[0] = fft_v2f{A.x + B.x, A.x - B.x};
                else         istft_presplit(dst, k, M, A, B, tw[k]);
            }
        }
        fft_v2f *sw = src;                                               // the inverse passes start from Z
        src = dst;
        dst = sw;
    }
};
using MaskSource = MaskSourceT<float>;
using CMaskSource = MaskSourceT<fft_v2f>;

// The filter-and-sum source (bhw_beam_fft_f32_*): n_ch channels of signal b, each with its own pair-gain rows.
// frame() runs a. and b. per channel, always from the slot's first buffer, and in c. adds the masked bins of the lane's own k into a
// running sum in registers (channel 0 sets it: +0 + -0 would lose a sign), in ascending channel order and one float32 add per part.
// After the last channel the pre-split of the sums goes to the buffer the transformed points are not in, as MaskSourceT's does.
//   Between channels: step c. reads src[k], src[M - k] and src[0] of the transformed points of OTHER lanes' passes.  With an even
// pass count they lie in the first buffer, which the next channel's row overwrites: a barrier that every lane reaches, active or
// not, stands between.  With an odd count they lie in the second buffer; the next row goes to the first, which no lane reads after
// the last pass's barrier, and the barrier behind that row stands before the first pass writes the second buffer.
//   A lane owns k = l, l + lpf, ... <= M / 2: at most M / (2 lpf) + 1 <= cpl / 4 + 1 = kMaxK values (the launcher checks it).
struct BeamSource {
    static constexpr bool kBins = false;
    static constexpr uint32_t kTables = 2;
    static constexpr uint32_t kMaxCpl = CMaskSource::kMaxCpl;
    static constexpr uint32_t kMaxK = kMaxCpl / 4u + 1u;
    const float *x;
    const fft_v2f *g;
    uint64_t samples, pad, hop, x_stride, x_cstride, g_stride, g_cstride, g_bstride;
    uint32_t reflect, n_ch;

    __device__ __forceinline__ void tables(fft_v2f *twf, uint32_t k, double cs, double sn) const { twf[k] = fft_v2f{(float)cs, (float)-sn}; }

    __device__ __forceinline__ void frame(const IfftIo &a, bool act, uint64_t b, uint64_t f, uint32_t l, const fft_v2f *tw, const float *vS,
                                          fft_v2f *&src, fft_v2f *&dst) const
    {
        const uint32_t M = a.m, lpf = a.lpf, H = M >> 1;
        const fft_v2f *twf = tw + M;
        fft_v2f *const first = src, *const second = dst;
        const bool even = ((a.radix4 + a.radix2) & 1u) == 0u;
        fft_v2f sA[kMaxK], sB[kMaxK];                                    // the sums of the masked Y[k] and Y[M - k]
#pragma unroll
        for (uint32_t i = 0; i < kMaxK; ++i) sA[i] = sB[i] = fft_v2f{0.0f, 0.0f};
        for (uint32_t c = 0; c < n_ch; ++c) {
            src = first;                                                 // every channel ends in the same buffer
            dst = second;
            mask_fft_row(a, act, x + b * x_stride + c * x_cstride, samples, pad, hop, reflect, f, l, vS, (float *)src);   // a.
            __syncthreads();
            mask_fft_forward(a, l, twf, src, dst);                                                                      // b.
            if (act) {                                                   // c. the split, the gains and the sum
                const fft_v2f *gp = g + b * g_bstride + c * g_cstride + f * g_stride;
#pragma unroll
                for (uint32_t i = 0; i < kMaxK; ++i) {
#pragma clang fp contract(off)
                    const uint32_t k = l + i * lpf;
                    if (k <= H) {
                        const fft_v2f A = CMaskSource::masked(fft_split_bin(src, twf, k, M), gp[k]);
                        const fft_v2f B = CMaskSource::masked(fft_split_bin(src, twf, M - k, M), gp[M - k]);
                        sA[i] = c ? fft_v2f{sA[i].x + A.x, sA[i].y + A.y} : A;
                        sB[i] = c ? fft_v2f{sB[i].x + B.x, sB[i].y + B.y} : B;
                    }
                }
            }
            if (even && c + 1u < n_ch) __syncthreads();                  // the next row overwrites the points c. reads
        }
        if (act) {                                                       // the pre-split of the sums, into the other buffer
#pragma unroll
            for (uint32_t i = 0; i < kMaxK; ++i) {
#pragma clang fp contract(off)
                const uint32_t k = l + i * lpf;
                if (k <= H) {
                    if (k == 0u) dst[0] = fft_v2f{sA[i].x + sB[i].x, sA[i].x - sB[i].x};
                    else         istft_presplit(dst, k, M, sA[i], sB[i], tw[k]);
                }
            }
        }
        fft_v2f *sw = src;                                               // the inverse passes start from Z
        src = dst;
        dst = sw;
    }
};

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_istft_fft_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock, 4) void k_mask_fft_direct(BhwCordicCfg cfg, BhwWinCfg win, IfftIo a, MaskSource m, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vS = (float *)(fft_lds + (size_t)(2u * a.fy + 2u) * a.m * sizeof(fft_v2f));
    for (uint32_t k = threadIdx.x; k < a.len; k += kFftBlock) {
        int32_t w;
        if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
        else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
        vS[k] = fft_coeff(w, a.shift);
    }
    istft_fft_spans(a, m);
}

// Coefficient gathered from a resident table in format FMT; every lane reaches the gather (at k = 0 past the window) for the escape
// format's wave-wide fix.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock, 4) void k_mask_fft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, IfftIo a,
                                                               MaskSource m, BhwLenPhase lp)
{
    float *vS = (float *)(fft_lds + (size_t)(2u * a.fy + 2u) * a.m * sizeof(fft_v2f));
    for (uint32_t k0 = 0; k0 < a.len; k0 += kFftBlock) {
        const uint32_t k = k0 + threadIdx.x;
        const bool in = k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (in) vS[k] = fft_coeff(w, a.shift);
    }
    istft_fft_spans(a, m);
}

// The same two kernels under the pair-gain source (bhw_cmask_fft_f32_*): the prologues are the ones above, word for word.
template <int FORM>
__global__ __launch_bounds__(kFftBlock, 4) void k_cmask_fft_direct(BhwCordicCfg cfg, BhwWinCfg win, IfftIo a, CMaskSource m, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vS = (float *)(fft_lds + (size_t)(2u * a.fy + 2u) * a.m * sizeof(fft_v2f));
    for (uint32_t k = threadIdx.x; k < a.len; k += kFftBlock) {
        int32_t w;
        if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
        else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
        vS[k] = fft_coeff(w, a.shift);
    }
    istft_fft_spans(a, m);
}

template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock, 4) void k_cmask_fft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, IfftIo a,
                                                                CMaskSource m, BhwLenPhase lp)
{
    float *vS = (float *)(fft_lds + (size_t)(2u * a.fy + 2u) * a.m * sizeof(fft_v2f));
    for (uint32_t k0 = 0; k0 < a.len; k0 += kFftBlock) {
        const uint32_t k = k0 + threadIdx.x;
        const bool in = k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (in) vS[k] = fft_coeff(w, a.shift);
    }
    istft_fft_spans(a, m);
}

// The same two kernels under the filter-and-sum source (bhw_beam_fft_f32_*): the prologues are the ones above, word for word.
// Unhinted, unlike their siblings: the twelve sums a lane carries across the channel loop do not fit the 128 registers of four
// workgroups per CU without a spill, so the compiler's own choice stands and a workgroup of occupancy is given up (section 45).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_beam_fft_direct(BhwCordicCfg cfg, BhwWinCfg win, IfftIo a, BeamSource m, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vS = (float *)(fft_lds + (size_t)(2u * a.fy + 2u) * a.m * sizeof(fft_v2f));
    for (uint32_t k = threadIdx.x; k < a.len; k += kFftBlock) {
        int32_t w;
        if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
        else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
        vS[k] = fft_coeff(w, a.shift);
    }
    istft_fft_spans(a, m);
}

template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_beam_fft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, IfftIo a,
                                                            BeamSource m, BhwLenPhase lp)
{
    float *vS = (float *)(fft_lds + (size_t)(2u * a.fy + 2u) * a.m * sizeof(fft_v2f));
    for (uint32_t k0 = 0; k0 < a.len; k0 += kFftBlock) {
        const uint32_t k = k0 + threadIdx.x;
        const bool in = k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (in) vS[k] = fft_coeff(w, a.shift);
    }
    istft_fft_spans(a, m);
}

} // namespace

// One launcher for both gain types: G float launches k_mask_fft_*, G fft_v2f (d_g: pairs, the strides in pairs) k_cmask_fft_*.
template <typename G>
static int mask_fft_launch(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwMaskFftPlan &pl, const bhw_stft *sa,
                           const bhw_stft *ss, const float *d_x, const G *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp)
{
    if (!ss->samples) return 0;
    if (pl.cpl > MaskSource::kMaxCpl) return (int)hipErrorInvalidValue;   // (the checks refuse 4096)
    hipStream_t st = (hipStream_t)l.stream;
    IfftIo a = istft_io<IfftIo>(pl, ss, nullptr, d_out);
    a.n_fft = (uint32_t)ss->n_fft;
    a.m = pl.m;
    a.radix4 = pl.radix4;
    a.radix2 = pl.radix2;
    MaskSourceT<G> m;
    m.x = d_x;
    m.g = d_g;
    m.samples = sa->samples;
    m.pad = sa->pad;
    m.hop = sa->hop;
    m.x_stride = pl.in_stride;
    m.g_stride = pl.g_stride;
    m.g_bstride = pl.g_bstride;
    m.reflect = sa->pad_mode == BHW_PAD_REFLECT ? 1u : 0u;
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) {
            if constexpr (std::is_same_v<G, float>) launch_lds(k_mask_fft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, m, lp);
            else                                    launch_lds(k_cmask_fft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, m, lp);
        },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            if constexpr (std::is_same_v<G, float>) launch_lds(k_mask_fft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, m, lp);
            else                                    launch_lds(k_cmask_fft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, m, lp);
        });
}

int bhwk_mask_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwMaskFftPlan &pl, const bhw_stft *sa,
                      const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp)
{
    return mask_fft_launch<float>(l, c_in, w, pl, sa, ss, d_x, d_g, d_out, d_table, lp);
}

int bhwk_cmask_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwMaskFftPlan &pl, const bhw_stft *sa,
                       const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp)
{
    return mask_fft_launch<fft_v2f>(l, c_in, w, pl, sa, ss, d_x, (const fft_v2f *)d_g, d_out, d_table, lp);
}

int bhwk_beam_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwBeamFftPlan &pl, const bhw_stft *sa,
                      const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp)
{
    if (!ss->samples) return 0;
    if (pl.cpl > BeamSource::kMaxCpl || (pl.m >> 1) / pl.lpf + 1u > BeamSource::kMaxK) return (int)hipErrorInvalidValue;   // (no plan has either)
    hipStream_t st = (hipStream_t)l.stream;
    IfftIo a = istft_io<IfftIo>(pl, ss, nullptr, d_out);
    a.n_fft = (uint32_t)ss->n_fft;
    a.m = pl.m;
    a.radix4 = pl.radix4;
    a.radix2 = pl.radix2;
    BeamSource m;
    m.x = d_x;
    m.g = (const fft_v2f *)d_g;
    m.samples = sa->samples;
    m.pad = sa->pad;
    m.hop = sa->hop;
    m.x_stride = pl.in_stride;
    m.x_cstride = pl.x_cstride;
    m.g_stride = pl.g_stride;
    m.g_cstride = pl.g_cstride;
    m.g_bstride = pl.g_bstride;
    m.reflect = sa->pad_mode == BHW_PAD_REFLECT ? 1u : 0u;
    m.n_ch = pl.n_ch;
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_beam_fft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, m, lp); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_beam_fft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, m, lp);
        });
}
