// bhw_mask_cmfft.hip -- window, mixed-radix complex FFT, a real or complex gain per bin, inverse mixed-radix complex FFT, window and
// overlap-add in one kernel for I/Q input and output, at n_fft = 2^a 3^b 5^c that is no power of two, odd lengths included
// (bhw_mask_cmfft_f32_device / _from_table and bhw_cmask_cmfft_f32_device / _from_table; contract: include/bhw.h, plan:
// BhwMaskCmfftPlan in bhw_plan.h, reasons: DESIGN.md section 44).
//
// The span / ring / flush kernel of bhw_istft_cmfft.hip (istft_cmfft_spans in bhw_istft_cmfft.h) with another frame source: where
// that kernel loads the n bins of a frame from memory, this one forms them in LDS from the signal.  The prologue and the LDS are the
// inverse parent's: it already runs the forward passes over the forward table (n IDFT(Y) = swap(DFT(swap(Y)))), so one table serves
// both directions.  Per frame f of a slot (MaskCmfftSourceT::frame), on the slot's buffers A (src) and B (dst):
//   a. lane l takes the columns j = l, l + lpf, ... < n of the row (the last column of a lane need not exist): complex sample
//      t = f * hop + j - pad of the signal (floats 2 t and 2 t + 1: one 8-byte load where iq_vec allows it, else two 4-byte ones)
//      under the padding rule of bhw_stft_cmfft.h (reflect, or +0.0 in place of both parts), each part times v[j - col0];
//      (+0.0, +0.0) outside the window and in a slot without a frame.  Writes A[j]; one barrier;
//   b. the plan's schedule by mfft_pass<R>, called exactly as stft_cmfft_rows calls it: each pass reads one buffer, writes the other,
//      and a barrier follows it;
//   c. the lane takes the bins k = l, l + lpf, ... < n of the transformed row, multiplies each by its gain -- read from gain column k
//      or, under the shift flag, from column (k + n / 2) mod n (integer division; a compare and a subtract): a load index, not a pass
//      -- with one float32 rounding per product, never contracted, and writes the bin back where it read it WITH THE PARTS SWAPPED,
//      as the inverse parent's load stores them.  A lane writes only positions it has itself read after the last pass's barrier, so
//      no barrier of its own follows: the one the inverse passes begin with (istft_cmfft_spans') orders these writes before any other
//      lane's read.
// No bin is special: bins 0 and n / 2 of a complex signal carry an imaginary part and take gi like any other.
// The inverse passes, the ring and the flush follow as they stand.  The bits of a masked row are those bhw_stft_cmfft_f32_* stores,
// times the gains; the bits of an output those bhw_istft_cmfft_f32_* gives for these rows.
//
// tests/cpp/san_mask_iq.cpp replays the sample reads of a. and the gain reads of c. from a copy of its own; an edit of
// MaskCmfftSourceT::frame is an edit of the replay too.
#include "bhw_istft_cmfft.h"

namespace {

// G, the gain of a bin: float (bhw_mask_cmfft_f32_*) or the pair fft_v2f (gr, gi) (bhw_cmask_cmfft_f32_*), as in bhw_mask_cfft.hip.
template <typename G>
struct MaskCmfftSourceT {
    static constexpr bool kBins = false;
    const float *x;
    const G *g;
    uint64_t samples, pad, hop, x_stride, g_stride, g_bstride;
    uint32_t reflect, xvec;

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

    __device__ __forceinline__ void frame(const IcmfftIo &a, bool act, uint64_t b, uint64_t f, uint32_t l, const fft_v2f *tw, const float *vS,
                                          fft_v2f *&src, fft_v2f *&dst) const
    {
        const uint32_t n = a.n, fold = a.fold, lpf = a.lpf;
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
        // b. the forward passes: Ns the product of the radices so far, rest = n / (Ns * r) after this pass
        uint32_t Ns = 1, rest = n;
        for (uint32_t p = 0; p < a.passes; ++p) {
            const uint32_t rdx = (a.sched >> (4u * p)) & 15u;
            if (rdx == 5u) {
                rest /= 5u;
                mfft_pass<5>(src, dst, tw, fold, n / 5u, Ns, rest, l, lpf);
            } else if (rdx == 3u) {
                rest /= 3u;
                mfft_pass<3>(src, dst, tw, fold, n / 3u, Ns, rest, l, lpf);
            } else if (rdx == 4u) {
                rest >>= 2;
                mfft_pass<4>(src, dst, tw, fold, n >> 2, Ns, rest, l, lpf);
            } else {
                rest >>= 1;
                mfft_pass<2>(src, dst, tw, fold, n >> 1, Ns, rest, l, lpf);
            }
            __syncthreads();
            fft_v2f *sw = src;
            src = dst;
            dst = sw;
            Ns *= rdx;
        }
        // c. the gains, in place and parts swapped: bin k by gain column k, or (k + n / 2) mod n
        if (act) {
            const G *gp = g + b * g_bstride + f * g_stride;
            const uint32_t turn = a.binshift ? n >> 1 : 0u;
            for (uint32_t k = l; k < n; k += lpf) {
                uint32_t col = k + turn;
                col = col >= n ? col - n : col;
                const fft_v2f y = masked(src[k], gp[col]);
                src[k] = fft_v2f{y.y, y.x};
            }
        }
    }
};

// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_istft_cmfft_direct): the prologues and the launch bounds below are
// the inverse parent's, word for word.
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_mask_cmfft_direct(BhwCordicCfg cfg, BhwWinCfg win, IcmfftIo a, MaskCmfftSourceT<float> m,
                                                                  BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vS = (float *)(fft_lds + icmfft_window_offset(a));
    for (uint32_t k = threadIdx.x; k < a.len; k += kFftBlock) {
        int32_t w;
        if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
        else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
        vS[k] = fft_coeff(w, a.shift);
    }
    istft_cmfft_spans(a, m);
}

// Coefficient gathered from a resident table in format FMT; every lane reaches the gather (at k = 0 past the window) for the escape
// format's wave-wide fix.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_mask_cmfft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, IcmfftIo a,
                                                                 MaskCmfftSourceT<float> m, BhwLenPhase lp)
{
    float *vS = (float *)(fft_lds + icmfft_window_offset(a));
    for (uint32_t k0 = 0; k0 < a.len; k0 += kFftBlock) {
        const uint32_t k = k0 + threadIdx.x;
        const bool in = k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (in) vS[k] = fft_coeff(w, a.shift);
    }
    istft_cmfft_spans(a, m);
}

// The same two kernels under the pair-gain source (bhw_cmask_cmfft_f32_*): the prologues are the ones above, word for word.
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_cmask_cmfft_direct(BhwCordicCfg cfg, BhwWinCfg win, IcmfftIo a, MaskCmfftSourceT<fft_v2f> m,
                                                                   BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vS = (float *)(fft_lds + icmfft_window_offset(a));
    for (uint32_t k = threadIdx.x; k < a.len; k += kFftBlock) {
        int32_t w;
        if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
        else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
        vS[k] = fft_coeff(w, a.shift);
    }
    istft_cmfft_spans(a, m);
}

template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_cmask_cmfft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, IcmfftIo a,
                                                                  MaskCmfftSourceT<fft_v2f> m, BhwLenPhase lp)
{
    float *vS = (float *)(fft_lds + icmfft_window_offset(a));
    for (uint32_t k0 = 0; k0 < a.len; k0 += kFftBlock) {
        const uint32_t k = k0 + threadIdx.x;
        const bool in = k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (in) vS[k] = fft_coeff(w, a.shift);
    }
    istft_cmfft_spans(a, m);
}

} // namespace

// One launcher for both gain types: G float launches k_mask_cmfft_*, G fft_v2f (d_g: pairs, the strides in pairs) k_cmask_cmfft_*.
template <typename G>
static int mask_cmfft_launch(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwMaskCmfftPlan &pl, const bhw_stft *sa,
                             const bhw_stft *ss, const float *d_x, const G *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp)
{
    if (!ss->samples) return 0;
    if (pl.cpl > kCfftMaxCpl) return (int)hipErrorInvalidValue;         // (the checks refuse what would need more)
    hipStream_t st = (hipStream_t)l.stream;
    IcmfftIo a = istft_io<IcmfftIo>(pl, ss, nullptr, d_out);
    a.n = pl.n;
    a.fold = pl.fold;
    a.passes = pl.passes;
    for (uint32_t p = 0; p < pl.passes; ++p) a.sched |= (uint32_t)pl.radix[p] << (4u * p);
    a.binshift = pl.shifted ? 1u : 0u;                                   // here: of the gain columns
    a.vec = iq_vec(d_out, ss->batch, pl.x_stride);
    MaskCmfftSourceT<G> m;
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
            if constexpr (std::is_same_v<G, float>) launch_lds(k_mask_cmfft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, m, lp);
            else                                    launch_lds(k_cmask_cmfft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, m, lp);
        },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            if constexpr (std::is_same_v<G, float>) launch_lds(k_mask_cmfft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, m, lp);
            else                                    launch_lds(k_cmask_cmfft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, m, lp);
        });
}

int bhwk_mask_cmfft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwMaskCmfftPlan &pl, const bhw_stft *sa,
                        const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp)
{
    return mask_cmfft_launch<float>(l, c_in, w, pl, sa, ss, d_x, d_g, d_out, d_table, lp);
}

int bhwk_cmask_cmfft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwMaskCmfftPlan &pl, const bhw_stft *sa,
                         const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp)
{
    return mask_cmfft_launch<fft_v2f>(l, c_in, w, pl, sa, ss, d_x, (const fft_v2f *)d_g, d_out, d_table, lp);
}
