// san_istft_mfft.cpp -- the planner's part of the fused inverse mixed-radix FFT + overlap-add calls (bhw_plan.cpp:
// bhwp_istft_mfft_checks / bhwp_istft_mfft_plan / bhwp_describe_istft_mfft, bhwp_istft_span of bhw_plan.h) swept under
// AddressSanitizer + UBSan over EVERY supported n_fft against L, hop, batch, frames and `samples` at the edges, padded and packed,
// centred and not.  Besides "no report" it asserts the plan's invariants -- LDS within 64 KiB, lanes x slots = the workgroup,
// ceil(n_fft / lanes) <= 16 columns, the forward's schedule, S >= 4 * halo, the spans covering the outputs, grid within its bound --
// and replays on the host, lane by lane, the kernel's index arithmetic (bhw_istft_mfft.hip):
//   - the pre-split for odd and even M: every bin of the row read exactly once, every point Z written exactly once, the self-partner
//     test 2 k == M; the imaginary parts of bins 0 and M poisoned with NaN;
//   - every pass: every point read and written exactly once, every twiddle index below n_fft and inside the table after the fold, the
//     float i mod Ns equal to the integer one with the reciprocal moved one ulp each way;
//   - the float32 result -- pre-split, conjugated butterflies, table twiddles, one multiply by fl32(1 / n_fft) -- against a direct
//     binary64 inverse DFT of the Hermitian extension: relative l2 error under 2^-24 * log2(n_fft);
//   - the span walk, the ring and the flush on the geometries of tests/istft_mfft_cases.py and a sweep: every span taken by exactly
//     one (workgroup, trip of the group loop, slot); its frame list within `trips`, and exactly the frames that reach its outputs;
//     every output (b, t) stored exactly once, inside x's extent and never in a stride gap; the products added to an output are
//     exactly (f, u - f * hop) for the frames reaching it, each once, in ascending f; outputs no frame reaches stored as zeros; every
//     accumulator clear when its slot leaves a span; the stepped base mod n_fft equal to the true modulo for every frame.
// The replay is a SECOND COPY of the kernel's index arithmetic, kept in step by hand (only bhwp_istft_span is shared code): a change
// of the pre-split pairs, the pass indices, the ring, the stepped modulo or the flush bound in bhw_istft_mfft.hip has to be made here
// as well, or this program goes on checking the old kernel.
#include <cinttypes>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "bhw_plan.h"

static long g_checks = 0;
#define REQUIRE(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}
static double unit() { return (double)(rnd() >> 11) / 9007199254740992.0 - 0.5; }
// a standard normal deviate (the sum of twelve uniforms)
static double gauss()
{
    double s = 0.0;
    for (int i = 0; i < 12; ++i) s += unit();
    return s;
}

static bool supported(uint64_t n)
{
    if (n < 16 || n > 4095 || n % 2 || !(n & (n - 1))) return false;
    for (uint64_t r : {2, 3, 5})
        while (n % r == 0) n /= r;
    return n == 1;
}

static bhw_stft desc_of(uint64_t B, uint64_t T, uint64_t frames, uint64_t hop, uint64_t n_fft, uint64_t col0, uint64_t pad)
{
    bhw_stft s;
    memset(&s, 0, sizeof s);
    s.struct_size = sizeof s;
    s.channels = 1;
    s.batch = B;
    s.samples = T;
    s.frames = frames;
    s.hop = hop;
    s.n_fft = n_fft;
    s.col0 = col0;
    s.pad = pad;
    s.shift = 15;
    return s;
}

static void plan_invariants(const BhwIstftMfftPlan &pl, const bhw_stft &s, uint64_t L)
{
    const uint32_t n = (uint32_t)s.n_fft, M = n / 2;
    const uint64_t end = s.pad - s.col0 + s.samples;
    REQUIRE(pl.m == M && pl.lpf * pl.fy == kFftBlock && pl.lpf >= 4 && pl.lpf <= kFftBlock && !(pl.lpf & (pl.lpf - 1)), "lanes %u x %u", pl.lpf, pl.fy);
    REQUIRE((4 * pl.lpf >= M || pl.lpf == kFftBlock) && (pl.lpf == 4 || 4 * (pl.lpf / 2) < M), "lanes per row %u for M %u", pl.lpf, M);
    REQUIRE(pl.cpl == (n + pl.lpf - 1) / pl.lpf && pl.cpl <= kFftMaxCpl && pl.cpl >= 1, "%u columns per lane", pl.cpl);
    uint32_t prod = 1, last = 5;
    static const int rank[6] = {0, 0, 3, 1, 2, 0};                       // 5 < 3 < 4 < 2 in schedule order
    REQUIRE(pl.passes >= 2 && pl.passes <= kMfftMaxPasses, "%u passes", pl.passes);
    for (uint32_t i = 0; i < pl.passes; ++i) {
        const uint32_t r = pl.radix[i];
        REQUIRE(r == 2 || r == 3 || r == 4 || r == 5, "radix %u", r);
        REQUIRE(rank[r] >= rank[last], "radix %u after %u", r, last);
        REQUIRE(r != 2 || i + 1 == pl.passes, "a radix-2 pass that is not the last");
        last = r;
        prod *= r;
    }
    REQUIRE(prod == M, "the schedule transforms %u points, M = %u", prod, M);
    REQUIRE(pl.lds_bytes == 2u * pl.fy * M * 8u + M * 8u + n * 4u && pl.lds_bytes <= 64u * 1024u, "LDS %u", pl.lds_bytes);
    REQUIRE(pl.t0 == s.pad - s.col0 && pl.hop >= 1 && pl.hop <= s.hop && (pl.hop == s.hop || pl.hop == end), "t0 %" PRIu64 " hop %" PRIu64, pl.t0, pl.hop);
    REQUIRE(pl.halo == (L + pl.hop - 1) / pl.hop - 1, "halo %" PRIu64, pl.halo);
    REQUIRE(pl.span >= 1 && pl.span <= s.frames && (pl.span >= kIfftHaloFactor * pl.halo || pl.span == s.frames || pl.span * pl.hop >= end), "S %" PRIu64 " halo %" PRIu64, pl.span, pl.halo);
    REQUIRE(pl.spans >= 1 && pl.spans * pl.span * pl.hop >= end && (pl.spans - 1) * pl.span * pl.hop < end, "spans %" PRIu64, pl.spans);
    REQUIRE(pl.groups == (s.batch * pl.spans + pl.fy - 1) / pl.fy, "groups %" PRIu64, pl.groups);
    REQUIRE(pl.grid >= 1 && pl.grid <= kFftMaxGrid && (pl.grid == pl.groups || (pl.grid == kFftMaxGrid && pl.groups > pl.grid)), "grid %" PRIu64, pl.grid);
    REQUIRE(pl.trips >= 1 && pl.trips <= s.frames && pl.trips <= pl.span + pl.halo, "trips %" PRIu64, pl.trips);
    REQUIRE(pl.y_stride >= n + 2 && pl.y_stride % 2 == 0 && pl.y_bstride % 2 == 0 && pl.x_stride >= s.samples, "strides");
}

struct C32 {
    float x, y;
};
static C32 cmul(C32 a, C32 w) { return C32{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }
static C32 add(C32 a, C32 b) { return C32{a.x + b.x, a.y + b.y}; }
static C32 sub(C32 a, C32 b) { return C32{a.x - b.x, a.y - b.y}; }
static C32 scl(float s, C32 a) { return C32{s * a.x, s * a.y}; }

// the kernel's conjugated butterflies
static void butterfly(uint32_t R, C32 *a)
{
    static const float kSin3 = (float)0.86602540378443864676, kCos5a = (float)0.30901699437494742410, kCos5b = (float)-0.80901699437494742410,
                       kSin5a = (float)0.95105651629515357212, kSin5b = (float)0.58778525229247312917;
    if (R == 2) {
        const C32 a0 = a[0], a1 = a[1];
        a[0] = add(a0, a1);
        a[1] = sub(a0, a1);
    } else if (R == 3) {
        const C32 t1 = add(a[1], a[2]), d = sub(a[1], a[2]);
        const C32 t2 = sub(a[0], scl(0.5f, t1)), t3 = scl(kSin3, d);
        a[0] = add(a[0], t1);
        a[1] = C32{t2.x - t3.y, t2.y + t3.x};
        a[2] = C32{t2.x + t3.y, t2.y - t3.x};
    } else if (R == 4) {
        const C32 t0 = add(a[0], a[2]), t1 = sub(a[0], a[2]), t2 = add(a[1], a[3]);
        const C32 t3 = C32{a[3].y - a[1].y, a[1].x - a[3].x};
        a[0] = add(t0, t2);
        a[1] = add(t1, t3);
        a[2] = sub(t0, t2);
        a[3] = sub(t1, t3);
    } else {
        const C32 b1 = add(a[1], a[4]), b2 = add(a[2], a[3]), d1 = sub(a[1], a[4]), d2 = sub(a[2], a[3]);
        const C32 m1 = add(add(a[0], scl(kCos5a, b1)), scl(kCos5b, b2)), m2 = add(add(a[0], scl(kCos5b, b1)), scl(kCos5a, b2));
        const C32 n1 = add(scl(kSin5a, d1), scl(kSin5b, d2)), n2 = sub(scl(kSin5b, d1), scl(kSin5a, d2));
        a[0] = add(add(a[0], b1), b2);
        a[1] = C32{m1.x - n1.y, m1.y + n1.x};
        a[4] = C32{m1.x + n1.y, m1.y - n1.x};
        a[2] = C32{m2.x - n2.y, m2.y + n2.x};
        a[3] = C32{m2.x + n2.y, m2.y - n2.x};
    }
}

// The pre-split, the passes and the scaling of one row in float32, lane by lane; returns the relative l2 error of the row against a
// direct binary64 inverse DFT of the Hermitian extension.
static long g_butterflies = 0, g_odd = 0, g_even = 0;
static double replay_transform(const BhwIstftMfftPlan &pl, uint32_t n)
{
    const uint32_t M = n / 2, lpf = pl.lpf, H = M >> 1;
    const double pi = 3.14159265358979323846;
    std::vector<C32> Y(M + 1), A(M), Bf(M), tw(M);
    for (auto &y : Y) y = C32{(float)gauss(), (float)gauss()};
    std::vector<C32> Yk = Y;                                              // what the kernel reads: the two imaginary parts poisoned
    Yk[0].y = Yk[M].y = NAN;
    for (uint32_t k = 0; k < M; ++k) tw[k] = C32{(float)cos(2.0 * pi * k / n), (float)sin(2.0 * pi * k / n)};
    C32 *src = A.data(), *dst = Bf.data();
    std::vector<int> hit(M, 0), readY(M + 1, 0);
    for (uint32_t l = 0; l < lpf; ++l)
        for (uint32_t k = l; k <= H; k += lpf) {
            REQUIRE(k <= M && M - k <= M, "bin %u", M - k);
            const C32 Ab = Yk[k], Bb = Yk[M - k];
            ++readY[k];
            ++readY[M - k];
            if (k == 0u) {
                src[0] = C32{Ab.x + Bb.x, Ab.x - Bb.x};
                ++hit[0];
                continue;
            }
            const C32 w = tw[k];
            const C32 e0{Ab.x + Bb.x, Ab.y - Bb.y}, d0{Ab.x - Bb.x, Ab.y + Bb.y};
            const C32 o0 = cmul(d0, w);
            src[k] = C32{e0.x - o0.y, e0.y + o0.x};
            ++hit[k];
            if (2u * k != M) {
                const C32 e1{e0.x, -e0.y}, d1{-d0.x, d0.y};
                const C32 o1 = cmul(d1, C32{-w.x, w.y});
                src[M - k] = C32{e1.x - o1.y, e1.y + o1.x};
                ++hit[M - k];
            } else {
                --readY[k];                                               // the self-mirrored bin: A and B are one load of it
                REQUIRE(M % 2 == 0, "a self-partner with odd M");
            }
        }
    for (uint32_t i = 0; i < M; ++i) REQUIRE(hit[i] == 1, "n %u pre-split: point %u written %d times", n, i, hit[i]);
    for (uint32_t k = 0; k <= M; ++k) REQUIRE(readY[k] == 1, "n %u pre-split: bin %u read %d times", n, k, readY[k]);
    if (M % 2) ++g_odd; else ++g_even;
    uint32_t Ns = 1, rest = M;
    for (uint32_t p = 0; p < pl.passes; ++p) {
        const uint32_t R = pl.radix[p];
        REQUIRE(rest % R == 0, "pass %u of radix %u over %u", p, R, rest);
        rest /= R;
        const uint32_t Q = M / R, ts = 2u * rest;
        REQUIRE((uint64_t)ts * R * Ns == n, "twiddle stride %u", ts);
        std::vector<int> rd(M, 0), wr(M, 0);
        const float inv = 1.0f / (float)Ns;
        // a reciprocal one ulp off either way gives the same quotients (the hardware's is not correctly rounded)
        const float inv_lo = nextafterf(inv, 0.0f), inv_hi = nextafterf(inv, 2.0f);
        for (uint32_t l = 0; l < lpf; ++l)
            for (uint32_t i = l; i < Q; i += lpf) {
                C32 a[5];
                for (uint32_t q = 0; q < R; ++q) {
                    REQUIRE(i + q * Q < M, "read %u", i + q * Q);
                    ++rd[i + q * Q];
                    a[q] = src[i + q * Q];
                }
                uint32_t k = i;
                if (Ns < Q) {
                    const uint32_t d = (uint32_t)(((float)i + 0.5f) * inv);
                    REQUIRE(d == i / Ns && d == (uint32_t)(((float)i + 0.5f) * inv_lo) && d == (uint32_t)(((float)i + 0.5f) * inv_hi), "%u / %u", i, Ns);
                    k = i - d * Ns;
                }
                REQUIRE(k == i % Ns, "%u mod %u", i, Ns);
                if (Ns > 1u) {
                    const uint32_t kt = k * ts;
                    for (uint32_t q = 1; q < R; ++q) {
                        const uint32_t idx = q * kt;
                        REQUIRE(idx < n, "twiddle index %u of %u", idx, n);
                        const bool hi = idx >= M;
                        const uint32_t at = hi ? idx - M : idx;
                        REQUIRE(at < M, "folded twiddle index %u", at);
                        const C32 w = hi ? C32{-tw[at].x, -tw[at].y} : tw[at];
                        a[q] = cmul(a[q], w);
                    }
                }
                butterfly(R, a);
                ++g_butterflies;
                const uint32_t o = (i - k) * R + k;
                for (uint32_t q = 0; q < R; ++q) {
                    REQUIRE(o + q * Ns < M, "write %u", o + q * Ns);
                    ++wr[o + q * Ns];
                    dst[o + q * Ns] = a[q];
                }
            }
        for (uint32_t i = 0; i < M; ++i) REQUIRE(rd[i] == 1 && wr[i] == 1, "n %u pass %u: point %u read %d, written %d times", n, p, i, rd[i], wr[i]);
        std::swap(src, dst);
        Ns *= R;
    }
    REQUIRE(Ns == M && rest == 1, "the passes end at Ns = M: %u", Ns);
    const float c = (float)(1.0 / (double)n);
    // the reference: x[j] = (1 / n) (Y0 + (-1)^j YM + 2 sum Re(Y[k] e^{+2 pi i j k / n})) in binary64, twiddles by exact index
    std::vector<double> cs(n), sn(n);
    for (uint32_t j = 0; j < n; ++j) {
        cs[j] = cos(2.0 * pi * j / n);
        sn[j] = sin(2.0 * pi * j / n);
    }
    double err = 0.0, ref2 = 0.0;
    for (uint32_t j = 0; j < n; ++j) {
        double d = (double)Y[0].x + ((j & 1u) ? -(double)Y[M].x : (double)Y[M].x);
        uint32_t jk = 0;
        for (uint32_t k = 1; k < M; ++k) {
            jk += j;
            if (jk >= n) jk -= n;
            d += 2.0 * ((double)Y[k].x * cs[jk] - (double)Y[k].y * sn[jk]);
        }
        d /= (double)n;
        const float z = (j & 1u) ? src[j >> 1].y : src[j >> 1].x;
        const float r = z * c;
        REQUIRE(std::isfinite(r), "n %u element %u is not finite: an imaginary part of bin 0 or M was read", n, j);
        err += ((double)r - d) * ((double)r - d);
        ref2 += d * d;
    }
    return sqrt(err / ref2);
}

// The group loop, the frame walk, the ring and the stores of every lane.  An accumulator is the list of the (f, k) it was given.
typedef std::vector<std::pair<uint64_t, uint32_t>> Terms;
static long g_missing = 0, g_wraps = 0;
static void replay_spans(const BhwIstftMfftPlan &pl, const bhw_stft &s, uint64_t L)
{
    const uint64_t F = s.frames, B = s.batch, T = s.samples, K = s.n_fft / 2 + 1, hop = pl.hop;
    const uint32_t n = (uint32_t)s.n_fft, M = n / 2;
    const uint64_t yext = (B - 1) * pl.y_bstride + (F - 1) * pl.y_stride + 2 * K, pool = B * pl.spans;
    std::vector<int> owned(pool, 0), stored(B * T, 0);
    std::vector<Terms> ring(kFftBlock * kFftMaxCpl);                       // [tid][c]
    auto store = [&](uint64_t b, uint64_t w, const Terms &terms) {
        REQUIRE(w >= pl.t0 && w - pl.t0 < T, "output w %" PRIu64 " (t0 %" PRIu64 ", samples %" PRIu64 ", n_fft %u, L %" PRIu64 ", hop %" PRIu64 ", frames %" PRIu64 ")", w, pl.t0, T, n, L, s.hop, F);
        const uint64_t t = w - pl.t0;
        REQUIRE(b * pl.x_stride + t < (B - 1) * pl.x_stride + T, "x index");
        ++stored[b * T + t];
        // the contract: the frames f with 0 <= w - f * hop < L, ascending (the real hop: a hop past the outputs leaves frame 0 alone)
        Terms want;
        for (uint64_t f = w >= L ? (w - L) / s.hop : 0; f < F && (unsigned __int128)f * s.hop <= w; ++f)
            if (w - f * s.hop < L) want.push_back({f, (uint32_t)(w - f * s.hop)});
        REQUIRE(terms == want, "output b %" PRIu64 " t %" PRIu64 ": %zu terms, the contract has %zu", b, t, terms.size(), want.size());
    };
    const uint32_t hm = (uint32_t)(hop % (uint64_t)n);
    for (uint64_t wg = 0; wg < pl.grid; ++wg)
        for (uint64_t g = wg; g < pl.groups; g += pl.grid)
            for (uint32_t slot = 0; slot < pl.fy; ++slot) {
                const uint64_t sp = g * pl.fy + slot;
                if (sp >= pool) continue;
                ++owned[sp];
                const uint64_t b = sp / pl.spans, si = sp - b * pl.spans;
                const BhwIstftSpan r = bhwp_istft_span(si, pl.span, hop, L, pl.t0, T, F);
                REQUIRE(r.f_hi - r.f_lo <= pl.trips && r.f_hi <= F && r.wlo <= r.whi, "span %" PRIu64 ": frames [%" PRIu64 ", %" PRIu64 ") of %" PRIu64 " trips", si, r.f_lo, r.f_hi, pl.trips);
                // exactly the frames that reach the span's outputs
                for (uint64_t f = r.wlo >= L + hop ? (r.wlo - L) / hop - 1 : 0; f < F; ++f) {
                    const bool reaches = f * hop < r.whi && f * hop + L > r.wlo && r.whi > r.wlo;
                    REQUIRE(reaches == (f >= r.f_lo && f < r.f_hi), "span %" PRIu64 " frame %" PRIu64, si, f);
                    if (f * hop >= r.whi) break;
                }
                std::vector<uint64_t> cur(pl.lpf, r.wlo);
                uint32_t bm = (uint32_t)((r.f_lo * hop) % (uint64_t)n);
                for (uint64_t it = 0; it < pl.trips; ++it) {
                    const uint64_t f = r.f_lo + it;
                    REQUIRE(bm < n && bm == (uint32_t)((unsigned __int128)f * hop % n), "stepped base mod n_fft: frame %" PRIu64 " hop %" PRIu64 " n %u: %u", f, hop, n, bm);
                    if (f < r.f_hi)
                        for (uint32_t l = 0; l < pl.lpf; ++l) {
                            const uint32_t tid = slot * pl.lpf + l;
                            for (uint32_t k = l; k <= M / 2; k += pl.lpf) {
                                const uint64_t y0 = b * pl.y_bstride + f * pl.y_stride;
                                REQUIRE(y0 + 2 * (M - k) + 2 <= yext && 2 * (uint64_t)(M - k) + 2 <= pl.y_stride, "Y index");
                            }
                            const uint64_t base = f * hop;
                            uint64_t c0 = cur[l];
                            if (c0 < base) {
                                for (uint64_t w = c0 + l; w < base; w += pl.lpf) store(b, w, Terms());
                                c0 = base;
                            }
                            uint64_t end = (f + 1 == r.f_hi || base + hop > r.whi) ? r.whi : base + hop;
                            if (end < c0) end = c0;
                            for (uint32_t c = 0; c < kFftMaxCpl; ++c) {
                                if (!(c < pl.cpl && c * pl.lpf + l < n)) {        // the cols mask
                                    if (c < pl.cpl) ++g_missing;
                                    continue;
                                }
                                const uint32_t q = c * pl.lpf + l;
                                const uint32_t k = q >= bm ? q - bm : q + n - bm;
                                REQUIRE(k < n && (base + k) % n == q, "ring position %u of base %" PRIu64, q, base);
                                const uint64_t w = base + k;
                                if (k < L && w >= c0 && w < r.whi) {
                                    REQUIRE(s.col0 + k < n, "row column %" PRIu64, s.col0 + k);
                                    Terms &acc = ring[tid * kFftMaxCpl + c];
                                    acc.push_back({f, k});
                                    if (w < end) {
                                        store(b, w, acc);
                                        acc.clear();
                                    }
                                }
                            }
                            const uint64_t reach = base + L;
                            if (reach < end)
                                for (uint64_t w = (reach > c0 ? reach : c0) + l; w < end; w += pl.lpf) store(b, w, Terms());
                            cur[l] = end;
                        }
                    bm += hm;
                    if (bm >= n) {
                        bm -= n;
                        ++g_wraps;
                    }
                }
                for (uint32_t l = 0; l < pl.lpf; ++l) {
                    for (uint64_t w = cur[l] + l; w < r.whi; w += pl.lpf) store(b, w, Terms());
                    for (uint32_t c = 0; c < kFftMaxCpl; ++c) REQUIRE(ring[(slot * pl.lpf + l) * kFftMaxCpl + c].empty(), "accumulator left full");
                }
            }
    for (uint64_t i = 0; i < pool; ++i) REQUIRE(owned[i] == 1, "span %" PRIu64 " owned %d times", i, owned[i]);
    for (uint64_t i = 0; i < stored.size(); ++i) REQUIRE(stored[i] == 1, "output %" PRIu64 " stored %d times", i, stored[i]);
}

// the geometries of tests/istft_mfft_cases.py (the benchmarked batch at 4 signals: its S comes from the batch, see the sweep)
struct Geometry {
    uint32_t n, L;
    uint64_t hop;
    int centred;
    uint64_t B, F;
    int64_t extra;
    int padded;
};
static const Geometry kTable[] = {
    {18, 13, 5, 1, 3, 18, 0, 0},      {20, 20, 10, 1, 5, 4, 0, 0},       {30, 24, 7, 1, 3, 40, -9, 0},     {50, 50, 4, 1, 2, 6, 90, 0},
    {54, 40, 9, 1, 4, 50, 300, 1},    {96, 96, 37, 0, 2, 44, 0, 0},      {250, 100, 300, 1, 3, 5, 0, 1},   {400, 400, 160, 1, 2, 26, 0, 0},
    {480, 400, 100, 1, 3, 15, 0, 0},  {1000, 1000, 300, 1, 3, 15, 0, 0}, {1200, 1200, 300, 0, 1, 20, 0, 0}, {1200, 1200, 8, 1, 1, 1100, 0, 0},
    {1536, 1536, 512, 1, 2, 8, 0, 0}, {2560, 100, 200, 1, 1, 2047, 1000, 0}, {4000, 4000, 1000, 1, 2, 8, 0, 0}, {4050, 4050, 1000, 1, 2, 8, 0, 0},
    {400, 400, 160, 1, 4, 998, 0, 0},
};

int main()
{
    char buf[1100];
    long span_replays = 0, pass_replays = 0, cut = 0, sizes = 0;
    double worst = 0.0;
    uint32_t worst_n = 0;
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 12, 24);
    const uint64_t xa = 0x10000000ull, ya = 0x100000000000ull;
    for (const Geometry &g : kTable) {
        const uint64_t pad = g.centred ? g.n / 2 : 0, col0 = (g.n - g.L) / 2;
        const uint64_t T = (uint64_t)((int64_t)(g.n + g.hop * (g.F - 1) - 2 * pad) + g.extra);
        bhw_stft s = desc_of(g.B, T, g.F, g.hop, g.n, col0, pad);
        if (g.padded) {
            s.x_stride = T + 5;
            s.y_stride = g.n + 2 + 6;
            s.y_batch_stride = g.F * s.y_stride + 10;
        }
        REQUIRE(bhwp_istft_mfft_checks(&p, g.L, &s, 1, (const void *)ya, (const void *)xa) == BHW_OK, "table geometry n %u", g.n);
        const BhwIstftMfftPlan pl = bhwp_istft_mfft_plan(&p, g.L, &s, 1, false);
        plan_invariants(pl, s, g.L);
        replay_spans(pl, s, g.L);
        ++span_replays;
        if (pl.spans > 1) ++cut;
    }
    for (uint64_t n = 1; n <= 5000; ++n) {
        if (!supported(n)) {
            bhw_stft s = desc_of(1, 100 + n, 2, 1, n, 0, n / 2);
            REQUIRE(bhwp_istft_mfft_checks(&p, 1, &s, 0, nullptr, nullptr, false) != BHW_OK, "n_fft %" PRIu64, n);
            REQUIRE(!bhwp_mfft_supported(n), "n_fft %" PRIu64, n);
            continue;
        }
        REQUIRE(bhwp_mfft_supported(n), "n_fft %" PRIu64, n);
        ++sizes;
        {
            bhw_stft s = desc_of(1, n, 1, 1, n, 0, 0);
            const BhwIstftMfftPlan pl = bhwp_istft_mfft_plan(&p, n, &s, 0, false);
            const double err = replay_transform(pl, (uint32_t)n), cap = ldexp(1.0, -24) * log2((double)n);
            REQUIRE(err < cap, "n %" PRIu64 ": the float32 row is %g from the binary64 inverse DFT, the cap is %g", n, err, cap);
            if (err / cap > worst) {
                worst = err / cap;
                worst_n = (uint32_t)n;
            }
            ++pass_replays;
        }
        for (uint64_t L : {(uint64_t)1, (uint64_t)13, n / 2 + 1, n - 1, n})
            for (uint64_t hop : {(uint64_t)1, (uint64_t)7, n / 4 + 3, n, n + 5})
                for (uint64_t B : {1ull, 3ull, 70ull})
                    for (uint64_t F : {1ull, 2ull, 65ull, 700ull})
                        for (int centred = 0; centred <= 1; ++centred)
                            for (int tail = 0; tail < 3; ++tail)            // samples: torch's default, shorter, past the frames' extent
                                for (int padded = 0; padded <= 1; ++padded) {
                                    if (!centred && L < n) continue;        // pad < col0
                                    const uint64_t pad = centred ? n / 2 : 0, col0 = (n - L) / 2;
                                    const uint64_t full = n + hop * (F - 1);
                                    if (full <= 2 * pad) continue;
                                    uint64_t T = full - 2 * pad;
                                    if (tail == 1) T = T > 5 ? T - 5 : 1;
                                    if (tail == 2) T += n + 2 * hop + 3;
                                    bhw_stft s = desc_of(B, T, F, hop, n, col0, pad);
                                    if (padded) {
                                        s.x_stride = T + 3;
                                        s.y_stride = n + 2 + 6;
                                        s.y_batch_stride = F * s.y_stride + 10;
                                    }
                                    if ((unsigned __int128)B * F * n > (1ull << 34)) continue;
                                    for (uint32_t flags = 0; flags <= 1; ++flags) {
                                        int rc = bhwp_istft_mfft_checks(&p, L, &s, flags, nullptr, nullptr, false);
                                        REQUIRE(rc == BHW_OK, "checks rc %d: n %" PRIu64 " L %" PRIu64 " hop %" PRIu64 " B %" PRIu64 " F %" PRIu64, rc, n, L, hop, B, F);
                                        rc = bhwp_istft_mfft_checks(&p, L, &s, flags, (const void *)ya, (const void *)xa);
                                        REQUIRE(rc == BHW_OK, "pointer checks rc %d", rc);
                                    }
                                    REQUIRE(bhwp_istft_mfft_checks(&p, L, &s, 0, (const void *)(ya + 4), (const void *)xa) == BHW_ERR_BADARG, "misaligned Y");
                                    REQUIRE(bhwp_istft_mfft_checks(&p, L, &s, 0, (const void *)ya, (const void *)ya) == BHW_ERR_BADARG, "overlap");
                                    REQUIRE(bhwp_istft_mfft_checks(&p, L, &s, 0, nullptr, (const void *)xa) == BHW_ERR_BADARG, "NULL Y");
                                    REQUIRE(bhwp_istft_mfft_checks(&p, L, &s, 2u, nullptr, nullptr, false) == BHW_ERR_BADARG, "flags");
                                    const BhwIstftMfftPlan pl = bhwp_istft_mfft_plan(&p, L, &s, tail == 0, (B + F) % 2 == 0);
                                    plan_invariants(pl, s, L);
                                    REQUIRE(bhwp_describe_istft_mfft(&p, nullptr, L, &s, 1, buf, sizeof buf) == BHW_OK && strlen(buf) > 40 && strlen(buf) < sizeof buf - 1, "describe");
                                    if (B * (T + F * L) <= 600 || (n <= 54 && B == 1 && F == 700 && hop == 7 && L == 13)) {
                                        replay_spans(pl, s, L);
                                        ++span_replays;
                                        if (pl.spans > 1) ++cut;
                                    }
                                    bhw_stft bad = s;
                                    bad.y_stride = n + 1;
                                    REQUIRE(bhwp_istft_mfft_checks(&p, L, &bad, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "short y_stride");
                                    bad.y_stride = n + 3;
                                    REQUIRE(bhwp_istft_mfft_checks(&p, L, &bad, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "odd y_stride");
                                    bad = s;
                                    bad.y_batch_stride = (F - 1) * pl.y_stride + n;
                                    REQUIRE(bhwp_istft_mfft_checks(&p, L, &bad, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "short y_batch_stride");
                                    bad = s;
                                    bad.channels = 2;
                                    bad.x_stride = 0;
                                    REQUIRE(bhwp_istft_mfft_checks(&p, L, &bad, 0, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED, "channels");
                                    bad = s;
                                    bad.pad_mode = BHW_PAD_REFLECT;
                                    REQUIRE(bhwp_istft_mfft_checks(&p, L, &bad, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "pad_mode");
                                    bad = s;
                                    bad.samples = 0;
                                    bad.x_stride = 0;
                                    REQUIRE(bhwp_istft_mfft_checks(&p, L, &bad, 0, nullptr, nullptr) == BHW_OK, "samples 0");
                                    REQUIRE(bhwp_describe_istft_mfft(&p, nullptr, L, &bad, 0, buf, sizeof buf) == BHW_OK, "describe samples 0");
                                }
    }
    // a hop past every output, up to 2^63: frame 0 alone
    for (uint64_t hop : {5000ull, 1ull << 40, 1ull << 63}) {
        bhw_stft s = desc_of(2, 700, 3, hop, 250, 25, 125);
        REQUIRE(bhwp_istft_mfft_checks(&p, 200, &s, 1, nullptr, nullptr, false) == BHW_OK, "hop %" PRIu64, hop);
        const BhwIstftMfftPlan pl = bhwp_istft_mfft_plan(&p, 200, &s, 1, false);
        plan_invariants(pl, s, 200);
        replay_spans(pl, s, 200);
    }
    // a power of two names the other family; the Taylor sources have no float32 kernels
    {
        bhw_stft s = desc_of(1, 1000, 3, 7, 512, 0, 256);
        REQUIRE(bhwp_istft_mfft_checks(&p, 512, &s, 0, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED, "a power of two");
        s = desc_of(1ull << 20, 100, 2048, 18, 18, 0, 9);                      // 2^31 rows x 18 columns > 2^34
        REQUIRE(bhwp_istft_mfft_checks(&p, 18, &s, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "cap");
        s = desc_of(1, 100, 0, 18, 18, 0, 9);
        REQUIRE(bhwp_istft_mfft_checks(&p, 18, &s, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "frames 0 with samples");
        s = desc_of(1, 100, 4, 18, 18, 3, 2);
        REQUIRE(bhwp_istft_mfft_checks(&p, 10, &s, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "pad < col0");
    }
    REQUIRE(bhwp_istft_mfft_checks(&p, 18, nullptr, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "NULL descriptor");
    REQUIRE(sizes == 95 && pass_replays == 95 && g_odd > 5 && g_even > 50, "%ld sizes, %ld pass replays (%ld with M odd)", sizes, pass_replays, g_odd);
    REQUIRE(span_replays > 1500 && cut > 200 && g_missing > 1000 && g_wraps > 1000, "replays %ld (%ld cut into spans), %ld missing columns, %ld wraps", span_replays, cut, g_missing, g_wraps);
    printf("ok %ld checks, %ld span replays (%ld of signals cut into several spans), %ld pass replays (%ld with M odd, %ld butterflies), "
           "worst row error %.3f of 2^-24 log2 n at n_fft %u\n", g_checks, span_replays, cut, pass_replays, g_odd, g_butterflies, worst, worst_n);
    return 0;
}
