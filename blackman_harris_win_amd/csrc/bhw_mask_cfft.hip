// bhw_mask_cfft.hip -- window, complex FFT, a real or complex gain per bin, inverse complex FFT, window and overlap-add in one kernel
// for I/Q input and output (bhw_mask_cfft_f32_device / _from_table and bhw_cmask_cfft_f32_device / _from_table; contract:
// include/bhw.h, plan: BhwMaskCfftPlan in bhw_plan.h, reasons: DESIGN.md section 44).
//
// The span / ring / flush kernel of bhw_istft_cfft.hip (istft_cfft_spans in bhw_istft_cfft.h) with another frame source: where that
// kernel loads the n bins of a frame from memory, this one forms them in LDS from the signal.  Prologue, once per workgroup: the window
// coefficients v[0..L) as the inverse kernels keep them, and TWO twiddle tables of n / 2 entries, the inverse one exp(+2 pi i k / n)
// and behind it the forward one exp(-2 pi i k / n), both from the same binary64 sincospi (the forward one is the table of
// bhw_stft_cfft.h word for word; a conjugating read of the inverse table would give the same values to cmul, but what the compiler
// contracts around a negated operand is not what it contracts around a loaded one, and the rows must be the forward parent's bits).
// Then, per frame f of a slot (MaskCfftSourceT::frame), on the slot's buffers A (src) and B (dst):
//   a. lane l takes the columns j = l, l + lpf, ... < n of the row: complex sample t = f * hop + j - pad of the signal (floats 2 t
//      and 2 t + 1: one 8-byte load where iq_vec allows it, else two 4-byte ones) under the padding rule of bhw_stft_cfft.h (reflect,
//      or +0.0 in place of both parts), each part times v[j - col0]; (+0.0, +0.0) outside the window and in a slot without a frame.
//      Writes A[j]; one barrier;
//   b. the forward passes of bhw_stft_cfft.h, the same text reading the forward table: each reads one buffer, writes the other, and
//      ends in a barrier;
//   c. the lane takes the bins k = l, l + lpf, ... < n of the transformed row, multiplies each by its gain -- read from gain column k
//      or, under the shift flag, from column (k + n / 2) mod n: a load index, not a pass -- with one float32 rounding per product, never
//      contracted, and writes the bin back where it read it.  A lane writes only positions it has itself read after the last pass's
//      barrier, so no barrier of its own follows: the one the inverse passes begin with (istft_cfft_spans') orders these writes before
//      any other lane's read.
// No bin is special: bins 0 and n / 2 of a complex signal carry an imaginary part and take gi like any other.
// The inverse passes, the ring and the flush follow as they stand.  The bits of a masked row are those bhw_stft_cfft_f32_* stores,
// times the gains; the bits of an output those bhw_istft_cfft_f32_* gives for these rows.
//
// tests/cpp/san_mask_iq.cpp replays the sample reads of a. and the gain reads of c. from a copy of its own; an edit of
// MaskCfftSourceT::frame is an edit of the replay too.
#include "bhw_istft_cfft.h"

namespace {

// G, the gain of a bin: float (bhw_mask_cfft_f32_*) or the pair fft_v2f (gr, gi) (bhw_cmask_cfft_f32_*).  g points to G and the two
// gain strides count G, so step c. loads 4-byte words or 8-byte pairs from the one text of frame(); masked() is overloaded on G.
template <typename G>
struct MaskCfftSourceT {
    static constexpr bool kBins = false;
    static constexpr uint32_t kTables = 2;
    const float *x;
    const G *g;
    uint64_t samples, pad, hop, x_stride, g_stride, g_bstride;
    uint32_t reflect, xvec;

    __device__ __forceinline__ void tables(fft_v2f *twf, uint32_t k, double cs, double sn) const { twf[k] = fft_v2f{(float)cs, (float)-sn}; }

    // the masked bin: one rounding per part
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

    __device__ __forceinline__ void frame(const IcfftIo &a, bool act, uint64_t b, uint64_t f, uint32_t l, const fft_v2f *tw, const float *vS,
                                          fft_v2f *&src, fft_v2f *&dst) const
    {
        const uint32_t n = a.n, H = n >> 1, Q = n >> 2, lpf = a.lpf;
        const fft_v2f *twf = tw + H;
        // a. the windowed row
        {
            const float *xb = x + b * x_stride;
            const uint64_t T = samples, t0 = f * hop - pad;              // the (wrapped) time of column 0
            for (uint32_t j = l; j < n; j += lpf) {
                const uint32_t k = j - a.col0;                           // unsigned: k < L is the window test
                fft_v2f r = fft_v2f{0.0f, 0.0f};
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
                    const float *px = xb + 2 * t;
                    fft_v2f xv;
                    if (xvec) xv = *(const fft_v2f *)px;
                    else      xv = fft_v2f{px[0], px[1]};
                    const fft_v2f e = zero ? fft_v2f{0.0f, 0.0f} : xv;
                    const float v = vS[k];
                    r = fft_v2f{e.x * v, e.y * v};
                }
                src[j] = r;
            }
        }
        __syncthreads();
        // b. the forward passes
        uint32_t Ns = 1;
        for (uint32_t p = 0; p < a.radix4; ++p) {
            const uint32_t ts = n / (4u * Ns);
            for (uint32_t i = l; i < Q; i += lpf) {
                const uint32_t k = i & (Ns - 1u);
                fft_v2f a0 = src[i], a1 = src[i + Q], a2 = src[i + 2u * Q], a3 = src[i + 3u * Q];
                if (Ns > 1u) {
                    const uint32_t kt = k * ts;
                    a1 = cmul(a1, twiddle(twf, kt, H));
                    a2 = cmul(a2, twiddle(twf, 2u * kt, H));
                    a3 = cmul(a3, twiddle(twf, 3u * kt, H));
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
        if (a.radix2) {                                                  // Ns = n / 2: k = i, twiddle W[i]
            for (uint32_t i = l; i < H; i += lpf) {
                const fft_v2f a0 = src[i], a1 = cmul(src[i + H], twf[i]);
                dst[i] = a0 + a1;
                dst[i + H] = a0 - a1;
            }
            __syncthreads();
            fft_v2f *sw = src;
            src = dst;
            dst = sw;
        }
        // c. the gains, in place: bin k by gain column k, or (k + n / 2) mod n
        if (act) {
            const G *gp = g + b * g_bstride + f * g_stride;
            const uint32_t turn = a.binshift ? H : 0u;
            for (uint32_t k = l; k < n; k += lpf) src[k] = masked(src[k], gp[(k + turn) & (n - 1u)]);
        }
    }
};

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_istft_cfft_direct): the prologues and the launch bounds below are
// the inverse parent's, but for the second table in front of the window coefficients.
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_mask_cfft_direct(BhwCordicCfg cfg, BhwWinCfg win, IcfftIo a, MaskCfftSourceT<float> m, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vS = (float *)(fft_lds + ((size_t)2u * a.fy * a.n + a.n) * sizeof(fft_v2f));
    for (uint32_t k = threadIdx.x; k < a.len; k += kFftBlock) {
        int32_t w;
        if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
        else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
        vS[k] = fft_coeff(w, a.shift);
    }
    istft_cfft_spans(a, m);
}

// Coefficient gathered from a resident table in format FMT; every lane reaches the gather (at k = 0 past the window) for the escape
// format's wave-wide fix.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_mask_cfft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, IcfftIo a,
                                                                MaskCfftSourceT<float> m, BhwLenPhase lp)
{
    float *vS = (float *)(fft_lds + ((size_t)2u * a.fy * a.n + a.n) * sizeof(fft_v2f));
    for (uint32_t k0 = 0; k0 < a.len; k0 += kFftBlock) {
        const uint32_t k = k0 + threadIdx.x;
        const bool in = k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (in) vS[k] = fft_coeff(w, a.shift);
    }
    istft_cfft_spans(a, m);
}

// The same two kernels under the pair-gain source (bhw_cmask_cfft_f32_*): the prologues are the ones above, word for word.
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_cmask_cfft_direct(BhwCordicCfg cfg, BhwWinCfg win, IcfftIo a, MaskCfftSourceT<fft_v2f> m,
                                                                  BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vS = (float *)(fft_lds + ((size_t)2u * a.fy * a.n + a.n) * sizeof(fft_v2f));
    for (uint32_t k = threadIdx.x; k < a.len; k += kFftBlock) {
        int32_t w;
        if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
        else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
        vS[k] = fft_coeff(w, a.shift);
    }
    istft_cfft_spans(a, m);
}

template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_cmask_cfft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, IcfftIo a,
                                                                 MaskCfftSourceT<fft_v2f> m, BhwLenPhase lp)
{
    float *vS = (float *)(fft_lds + ((size_t)2u * a.fy * a.n + a.n) * sizeof(fft_v2f));
    for (uint32_t k0 = 0; k0 < a.len; k0 += kFftBlock) {
        const uint32_t k = k0 + threadIdx.x;
        const bool in = k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (in) vS[k] = fft_coeff(w, a.shift);
    }
    istft_cfft_spans(a, m);
}

} // namespace

// One launcher for both gain types: G float launches k_mask_cfft_*, G fft_v2f (d_g: pairs, the strides in pairs) k_cmask_cfft_*.
template <typename G>
static int mask_cfft_launch(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwMaskCfftPlan &pl, const bhw_stft *sa,
                            const bhw_stft *ss, const float *d_x, const G *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp)
{
    if (!ss->samples) return 0;
    if (pl.cpl > kCfftMaxCpl) return (int)hipErrorInvalidValue;         // (the checks refuse what would need more)
    hipStream_t st = (hipStream_t)l.stream;
    IcfftIo a = istft_io<IcfftIo>(pl, ss, nullptr, d_out);
    a.n = pl.n;
    a.radix4 = pl.radix4;
    a.radix2 = pl.radix2;
    a.binshift = pl.shifted ? 1u : 0u;                                   // here: of the gain columns
    a.vec = iq_vec(d_out, ss->batch, pl.x_stride);
    MaskCfftSourceT<G> m;
    m.x = d_x;
    m.g = d_g;
    m.samples = sa->samples;
    m.pad = sa->pad;
    m.hop = sa->hop;
    m.x_stride = pl.in_stride;
    m.g_stride = pl.g_stride;
    m.g_bstride = pl.g_bstride;
    m.reflect = sa->pad_mode == BHW_PAD_REFLECT ? 1u : 0u;
    m.xvec = iq_vec(d_x, sa->batch, pl.in_stride);
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) {
            if constexpr (std::is_same_v<G, float>) launch_lds(k_mask_cfft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, m, lp);
            else                                    launch_lds(k_cmask_cfft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, m, lp);
        },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            if constexpr (std::is_same_v<G, float>) launch_lds(k_mask_cfft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, m, lp);
            else                                    launch_lds(k_cmask_cfft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, m, lp);
        });
}

int bhwk_mask_cfft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwMaskCfftPlan &pl, const bhw_stft *sa,
                       const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp)
{
    return mask_cfft_launch<float>(l, c_in, w, pl, sa, ss, d_x, d_g, d_out, d_table, lp);
}

int bhwk_cmask_cfft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwMaskCfftPlan &pl, const bhw_stft *sa,
                        const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp)
{
    return mask_cfft_launch<fft_v2f>(l, c_in, w, pl, sa, ss, d_x, (const fft_v2f *)d_g, d_out, d_table, lp);
}
