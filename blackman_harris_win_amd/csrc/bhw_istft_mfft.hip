// bhw_istft_mfft.hip -- inverse mixed-radix real FFT, window and overlap-add in one kernel, for even n_fft = 2^a 3^b 5^c that is no
// power of two (bhw_istft_mfft_f32_device / _from_table; contract: include/bhw.h, plan: BhwIstftMfftPlan in bhw_plan.h, reasons and
// measurements: DESIGN.md section 24).
//
// The span / halo / ring / flush kernel of bhw_istft_fft.hip with the generic Stockham pass of bhw_stft_mfft.hip inside.  A slot of
// lpf lanes owns one span of a signal's window-start axis w = t + pad - col0 and walks, in ascending f, the frames that reach the
// span's outputs (bhwp_istft_span).  Prologue, once per workgroup: the window coefficients v[0..L) by the direct CORDIC chains or the
// gather over a resident table, and the twiddle table W[k] = exp(+2 pi i k / n_fft), k < M = n_fft / 2, each component the float32
// rounding of a binary64 sincospi; both stay in LDS.  Then, per frame of the slot:
//   1. the pre-split for any M: a lane loads the bins Y[k] and Y[M - k], k = l, l + lpf, ... <= floor(M / 2), each bin once, and forms
//      Z[k] = (Y[k] + conj Y[M - k]) + i (Y[k] - conj Y[M - k]) W[k] and its partner Z[M - k] with W[M - k] = -conj W[k];
//      Z[0] = (Y[0].re + Y[M].re, Y[0].re - Y[M].re): the imaginary parts of bins 0 and M are never read into the arithmetic.  M may
//      be odd: then no bin is its own mirror, and the self-partner test is 2 k == M;
//   2. an inverse Stockham FFT of M points, out of place between two LDS buffers, in the forward's schedule (radix-5 passes, radix-3,
//      radix-4, a last radix-2): butterfly i < M / r reads src[i + q * M / r], multiplies by W at the EXACT index
//      q * k * (n_fft / (r Ns)), k = i mod Ns (indices >= M fold by W[i + M] = -W[i] with a compare), runs the conjugated butterfly
//      and writes dst[(i - k) * r + k + q * Ns].  i mod Ns is the forward's one float multiply.  The result
//      z[i] = (row[2 i], row[2 i + 1]) is n_fft times the row; the row is fl32(z * c), c = (float)(1.0 / (double) n_fft): one
//      float32 multiply, a rounding the power-of-two kernel does not have;
//   3. the ring: position q = c * lpf + l < n_fft belongs to lane l (a lane's last column may be missing: the cols mask).  With
//      base = f * hop, ring position q holds w = base + k, k = q - (base mod n_fft), plus n_fft when negative, which frame f reaches
//      at window index k < L and row column col0 + k.  base mod n_fft is taken once per span and stepped by hop mod n_fft with one
//      conditional subtraction per frame.  S[q] += (double) fl32(row[col0 + k] * c) * (double) v[k], E[q] += (double) v[k]^2, in
//      binary64 registers;
//   4. the flush of bhw_istft_fft.hip: after frame f every w < (f + 1) * hop of the span (after its last frame: every w) is complete;
//      the lane stores fl32(S) or fl32(S / E) (consecutive lanes, consecutive samples) and clears the position.  Outputs no frame
//      reaches are stored as +0.0 directly.
// The fy slots of a workgroup hold different spans (of any signals) and pass the same barriers: every slot makes `trips` rounds,
// idle once its frames are done.  A row's arithmetic does not depend on its slot, span or grid, and an output's sum takes its rows in
// ascending f whatever the spans are: the bits of an output are a function of the window and the rows that reach it.
//
// Kept in step by hand: imf_pass restates mfft_pass of bhw_stft_mfft.h around the conjugated butterfly, and the span walk, the ring
// and the flush stand in all four inverse units (bhw_istft_fft.hip, this one, bhw_istft_cfft.hip, bhw_istft_cmfft.hip);
// tests/cpp/san_istft_mfft.cpp replays this file's index arithmetic -- the pre-split pairs, the pass indices and the float i mod Ns,
// the ring's stepped base mod n_fft and the flush bound `end` -- from a copy of its own, since only bhwp_istft_span is shared
// through bhw_plan.h.  An edit of any of these here is an edit of the siblings and of the replay too.  cmul, mfft_twiddle, the radix
// constants and the dynamic LDS array are bhw_stft_mfft.h's and bhw_stft_fft.h's, the Io fill and istft_out bhw_istft.h's.
#include "bhw_istft.h"
#include "bhw_stft_mfft.h"

namespace {

struct ImfftIo {
    const float *Y;
    float *x;
    uint64_t batch, frames, hop, samples, t0;
    uint64_t x_stride, y_stride, y_bstride;
    uint64_t span, spans, groups, trips;
    uint32_t n_fft, m, col0, len;
    uint32_t lpf, fy, cpl, passes;
    uint32_t sched;                       // the radix of pass p in bits 4p .. 4p + 3
    uint32_t shift, normalize;
};

// X[q] = sum over j of a[j] exp(+2 pi i j q / R), in place: the forward's butterflies conjugated
template <uint32_t R>
__device__ __forceinline__ void imf_butterfly(fft_v2f (&a)[R])
{
    if constexpr (R == 2) {
        const fft_v2f a0 = a[0], a1 = a[1];
        a[0] = a0 + a1;
        a[1] = a0 - a1;
    } else if constexpr (R == 3) {
        const fft_v2f t1 = a[1] + a[2], d = a[1] - a[2];
        const fft_v2f t2 = a[0] - 0.5f * t1, t3 = kSin3 * d;
        a[0] = a[0] + t1;
        a[1] = fft_v2f{t2.x - t3.y, t2.y + t3.x};                  // t2 + i t3
        a[2] = fft_v2f{t2.x + t3.y, t2.y - t3.x};                  // t2 - i t3
    } else if constexpr (R == 4) {
        const fft_v2f t0 = a[0] + a[2], t1 = a[0] - a[2], t2 = a[1] + a[3];
        const fft_v2f t3 = fft_v2f{a[3].y - a[1].y, a[1].x - a[3].x};   // +i (a1 - a3)
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
        a[1] = fft_v2f{m1.x - n1.y, m1.y + n1.x};                  // m1 + i n1
        a[4] = fft_v2f{m1.x + n1.y, m1.y - n1.x};
        a[2] = fft_v2f{m2.x - n2.y, m2.y + n2.x};                  // m2 + i n2
        a[3] = fft_v2f{m2.x + n2.y, m2.y - n2.x};
    }
}

// One Stockham pass of radix R over the slot's M points: Q = M / R butterflies, sub-transform length Ns, ts = n_fft / (R Ns).
template <uint32_t R>
__device__ __forceinline__ void imf_pass(const fft_v2f *src, fft_v2f *dst, const fft_v2f *tw, uint32_t M, uint32_t Q, uint32_t Ns, uint32_t ts,
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
        imf_butterfly<R>(a);
        const uint32_t o = (i - k) * R + k;
#pragma unroll
        for (uint32_t q = 0; q < R; ++q) dst[o + q * Ns] = a[q];
    }
}

// Everything after the prologue's coefficients: vS (behind the twiddles) holds v[0..L).
__device__ __forceinline__ void istft_mfft_spans(const ImfftIo &a)
{
    const uint32_t M = a.m, n = a.n_fft, lpf = a.lpf, fy = a.fy, L = a.len;
    fft_v2f *bufA = (fft_v2f *)fft_lds;
    fft_v2f *bufB = bufA + (size_t)fy * M;
    fft_v2f *tw = bufB + (size_t)fy * M;
    const float *vS = (const float *)(tw + M);
    const uint32_t tid = threadIdx.x;
    const uint32_t slot = tid / lpf, l = tid - slot * lpf;
    for (uint32_t k = tid; k < M; k += kFftBlock) {
        double sn, cs;
        sincospi((double)k * 2.0 / (double)n, &sn, &cs);
        tw[k] = fft_v2f{(float)cs, (float)sn};
    }
    __syncthreads();
    const float scale = (float)(1.0 / (double)n);                        // not a power of two: the multiply rounds
    const uint64_t pool = a.batch * a.spans, hop = a.hop;
    const uint32_t H = M >> 1;                                           // floor(M / 2)
    const uint32_t hm = (uint32_t)(hop % (uint64_t)n);
    // bit c of cols: the lane has a ring position c (c * lpf + l < n_fft: the last one may be missing)
    uint32_t cols = 0;
#pragma unroll
    for (uint32_t c = 0; c < kFftMaxCpl; ++c)
        if (c < a.cpl && c * lpf + l < n) cols |= 1u << c;
    double acc[kFftMaxCpl], env[kFftMaxCpl];
#pragma unroll
    for (uint32_t c = 0; c < kFftMaxCpl; ++c) acc[c] = env[c] = 0.0;
    for (uint64_t g = blockIdx.x; g < a.groups; g += gridDim.x) {
        const uint64_t sp = g * fy + slot;
        const bool live = sp < pool;
        const uint64_t b = live ? sp / a.spans : 0, s = live ? sp - b * a.spans : 0;
        BhwIstftSpan r = bhwp_istft_span(s, a.span, hop, L, a.t0, a.samples, a.frames);
        if (!live) r.wlo = r.whi = r.f_lo = r.f_hi = 0;
        const float *yb = a.Y + b * a.y_bstride;
        float *xb = a.x + b * a.x_stride;                                // output t = w - t0 (every w formed below is >= wlo >= t0)
        uint64_t cur = r.wlo;                                            // the span's outputs below cur are stored
        uint32_t bm = (uint32_t)((r.f_lo * hop) % (uint64_t)n);          // (f * hop) mod n_fft of the round's frame, stepped below
        for (uint64_t it = 0; it < a.trips; ++it) {
            const uint64_t f = r.f_lo + it;
            const bool act = f < r.f_hi;
            // 1. the pre-split, into the slot's half of buffer A
            fft_v2f *src = bufA + (size_t)slot * M, *dst = bufB + (size_t)slot * M;
            if (act) {
                const fft_v2f *yp = (const fft_v2f *)(yb + f * a.y_stride);
                for (uint32_t k = l; k <= H; k += lpf) {
                    const fft_v2f A = yp[k], B = yp[M - k];
                    if (k == 0u) {
                        src[0] = fft_v2f{A.x + B.x, A.x - B.x};
                    } else {
                        const fft_v2f w = tw[k];
                        const fft_v2f e0 = fft_v2f{A.x + B.x, A.y - B.y}, d0 = fft_v2f{A.x - B.x, A.y + B.y};
                        const fft_v2f o0 = cmul(d0, w);
                        src[k] = fft_v2f{e0.x - o0.y, e0.y + o0.x};
                        if (2u * k != M) {                               // the partner M - k: W[M - k] = -conj W[k]
                            const fft_v2f e1 = fft_v2f{e0.x, -e0.y}, d1 = fft_v2f{-d0.x, d0.y};
                            const fft_v2f o1 = cmul(d1, fft_v2f{-w.x, w.y});
                            src[M - k] = fft_v2f{e1.x - o1.y, e1.y + o1.x};
                        }
                    }
                }
            }
            __syncthreads();
            // 2. the passes (every slot, idle ones on stale data: their result is not read): Ns the product of the radices so far,
            //    rest = M / (Ns * r) after this pass, so n_fft / (r Ns) = 2 * rest
            uint32_t Ns = 1, rest = M;
            for (uint32_t p = 0; p < a.passes; ++p) {
                const uint32_t rdx = (a.sched >> (4u * p)) & 15u;
                if (rdx == 5u) {
                    rest /= 5u;
                    imf_pass<5>(src, dst, tw, M, M / 5u, Ns, 2u * rest, l, lpf);
                } else if (rdx == 3u) {
                    rest /= 3u;
                    imf_pass<3>(src, dst, tw, M, M / 3u, Ns, 2u * rest, l, lpf);
                } else if (rdx == 4u) {
                    rest >>= 2;
                    imf_pass<4>(src, dst, tw, M, M >> 2, Ns, 2u * rest, l, lpf);
                } else {
                    rest >>= 1;
                    imf_pass<2>(src, dst, tw, M, M >> 1, Ns, 2u * rest, l, lpf);
                }
                __syncthreads();
                fft_v2f *sw = src;
                src = dst;
                dst = sw;
                Ns *= rdx;
            }
            // 3. and 4.: the ring
            if (act) {
                const float *row = (const float *)src + a.col0;
                const uint64_t base = f * hop;
                if (cur < base) {                                        // a gap no frame reaches (hop > L, or the span's start)
                    for (uint64_t w = cur + l; w < base; w += lpf) xb[w - a.t0] = 0.0f;
                    cur = base;
                }
                uint64_t end = (f + 1 == r.f_hi || base + hop > r.whi) ? r.whi : base + hop;
                if (end < cur) end = cur;                                // a halo frame whose own hop lies before the span
#pragma unroll
                for (uint32_t c = 0; c < kFftMaxCpl; ++c) {
                    if ((cols >> c) & 1u) {
                        const uint32_t q = c * lpf + l;
                        const uint32_t k = q >= bm ? q - bm : q + n - bm;
                        const uint64_t w = base + k;
                        if (k < L && w >= cur && w < r.whi) {
                            const double v = (double)vS[k];
                            acc[c] += (double)(row[k] * scale) * v;
                            env[c] += v * v;
                            if (w < end) {
                                xb[w - a.t0] = istft_out(acc[c], env[c], a.normalize);
                                acc[c] = env[c] = 0.0;
                            }
                        }
                    }
                }
                const uint64_t reach = base + L;                         // the frame's extent: beyond it up to `end` nothing is summed
                if (reach < end)
                    for (uint64_t w = (reach > cur ? reach : cur) + l; w < end; w += lpf) xb[w - a.t0] = 0.0f;
                cur = end;
            }
            bm += hm;                                                    // ((f + 1) * hop) mod n_fft: both terms are below n_fft
            if (bm >= n) bm -= n;
            __syncthreads();                                             // the next round overwrites both buffers
        }
        if (live)
            for (uint64_t w = cur + l; w < r.whi; w += lpf) xb[w - a.t0] = 0.0f;   // a span with no frame, or outputs past the last one
    }
}

// The compiler's own choice of registers: 156 a lane and three workgroups per CU.  Under __launch_bounds__(kFftBlock, 4), which
// bhw_istft_fft.hip holds at 127, the radix-5 butterfly spills 26 registers to scratch, and the library has no scratch.
// Coefficient by the direct CORDIC chains (FORM: direct_form, as k_istft_fft_direct).
template <int FORM>
__global__ __launch_bounds__(kFftBlock) void k_istft_mfft_direct(BhwCordicCfg cfg, BhwWinCfg win, ImfftIo a, BhwLenPhase lp)
{
    using T = std::conditional_t<FORM == 0, int32_t, int64_t>;
    using L = std::conditional_t<FORM == 2, uint32_t, T>;
    __shared__ L lut_s[32];
    if (threadIdx.x < 32) lut_s[threadIdx.x] = (L)cfg.lut[threadIdx.x];
    __syncthreads();
    float *vS = (float *)(fft_lds + (size_t)(2u * a.fy + 1u) * a.m * sizeof(fft_v2f));
    for (uint32_t k = threadIdx.x; k < a.len; k += kFftBlock) {
        int32_t w;
        if constexpr (FORM == 2) w = direct_coeff_mad_ph(cfg, win, lut_s, len_theta_of(lp, k));
        else                     w = direct_coeff_ph<T>(cfg, win, lut_s, len_theta_of(lp, k));
        vS[k] = fft_coeff(w, a.shift);
    }
    istft_mfft_spans(a);
}

// Coefficient gathered from a resident table in format FMT; every lane reaches the gather (at k = 0 past the window) for the escape
// format's wave-wide fix.
template <int FMT, int NT, int MODE>
__global__ __launch_bounds__(kFftBlock) void k_istft_mfft_table(BhwCordicCfg cfg, BhwWinCfg win, const void *__restrict__ table, ImfftIo a,
                                                                 BhwLenPhase lp)
{
    float *vS = (float *)(fft_lds + (size_t)(2u * a.fy + 1u) * a.m * sizeof(fft_v2f));
    for (uint32_t k0 = 0; k0 < a.len; k0 += kFftBlock) {
        const uint32_t k = k0 + threadIdx.x;
        const bool in = k < a.len;
        const int32_t w = range_coeff_ph<FMT, NT, MODE>(cfg, win, table, len_theta_of(lp, in ? k : 0u));
        if (in) vS[k] = fft_coeff(w, a.shift);
    }
    istft_mfft_spans(a);
}

} // namespace

int bhwk_istft_mfft_f32(const BhwLaunch &l, const BhwCordicCfg &c_in, const BhwWinCfg &w, const BhwIstftMfftPlan &pl, const bhw_stft *s,
                        const float *d_Y, float *d_x, const int32_t *d_table, const BhwLenPhase &lp)
{
    if (!s->samples) return 0;
    hipStream_t st = (hipStream_t)l.stream;
    ImfftIo a = istft_io<ImfftIo>(pl, s, d_Y, d_x);
    a.n_fft = (uint32_t)s->n_fft;
    a.m = pl.m;
    a.passes = pl.passes;
    for (uint32_t p = 0; p < pl.passes; ++p) a.sched |= (uint32_t)pl.radix[p] << (4u * p);
    const dim3 grid((unsigned)pl.grid), block(kFftBlock);
    return with_window_source(
        c_in, w, d_table, [&](auto D) { launch_lds(k_istft_mfft_direct<D>, grid, block, pl.lds_bytes, st, c_in, w, a, lp); },
        [&](auto F, auto NT, auto M, const BhwCordicCfg &c, const void *tab) {
            launch_lds(k_istft_mfft_table<F, NT, M>, grid, block, pl.lds_bytes, st, c, w, tab, a, lp);
        });
}
