// san_stft_mfft.cpp -- the planner's part of the mixed-radix fused window + FFT calls (bhw_plan.cpp: bhwp_stft_mfft_checks /
// bhwp_stft_mfft_plan / bhwp_describe_stft_mfft) swept under AddressSanitizer + UBSan over EVERY supported n_fft, every flag
// combination and the three output forms.  Besides "no report" it asserts the plan's invariants -- lanes x rows = the workgroup, lanes
// per row the smallest power of two >= M / 4 in 4..256, columns per lane ceil(n_fft / lanes) <= 16, the schedule 5s, 3s, 4s and a last
// 2 whose product is M, LDS within 64 KiB (20 KiB while several rows share a workgroup: fy * M <= 1024), the window staged inside the first buffer
// -- and replays on the host the kernel's index arithmetic (bhw_stft_mfft.hip):
//   - ownership: every row (b, f) of the pool is taken by exactly one (workgroup, trip of the group loop, slot);
//   - the columns: c * lpf + l < n_fft is the column test; every column of a row belongs to exactly one (lane, c);
//   - the loads: every window column of every row reads a sample inside its signal under both padding modes;
//   - the mean: one wave per row, lane i over j = i, i + 64, ..., then the shuffle butterfly, against the order bhw.h writes down, bit
//     for bit on binary64 sums of float32 data;
//   - the passes: i mod Ns by the float multiply for every butterfly, every point read exactly once and written exactly once per pass,
//     every twiddle index < n_fft (and inside the table after folding), and the passes and the split pass IN FLOAT, with
//     float32-rounded binary64 twiddles and butterfly constants, against a direct binary64 DFT of the float32 row within
//     2^-24 * log2(n_fft) in relative l2 error;
//   - the stores: every output column of every row written exactly once in the three forms, inside the row's floats and the output's
//     extent, never in a gap;
//   - the bank: whatever first / offset hold, no read leaves d_weight or the slot's K powers.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
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
static double uniform() { return (double)(rnd() >> 11) / 9007199254740992.0 - 0.5; }

static bhw_stft desc_of(uint64_t B, uint64_t T, uint64_t frames, uint64_t hop, uint64_t n_fft, uint64_t col0, uint64_t pad, uint32_t mode)
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
    s.pad_mode = mode;
    s.shift = 15;
    return s;
}

static bhw_fbank bank_of(uint32_t filters, uint32_t bins, uint32_t weights)
{
    bhw_fbank fb;
    memset(&fb, 0, sizeof fb);
    fb.struct_size = sizeof fb;
    fb.filters = filters;
    fb.bins = bins;
    fb.weights = weights;
    return fb;
}

static bool supported(uint64_t n)
{
    if (n < 16 || n > 4095 || n % 2 || !(n & (n - 1))) return false;
    for (uint64_t r : {2, 3, 5})
        while (n % r == 0) n /= r;
    return n == 1;
}

static void plan_invariants(const BhwStftMfftPlan &pl, const bhw_stft &s, uint32_t flags, const bhw_fbank *fb)
{
    const uint32_t n = (uint32_t)s.n_fft, M = n / 2;
    const uint64_t K = M + 1, W = !(flags & BHW_MFFT_POWER) ? 2 * K : fb ? fb->filters : K;
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
    REQUIRE(pl.lds_bytes == 2u * pl.fy * M * 8u + M * 8u + pl.fy * 4u && pl.lds_bytes <= 65536u, "LDS %u", pl.lds_bytes);
    REQUIRE(pl.fy == 1 || (pl.fy * M <= 1024u && pl.lds_bytes <= 20488u), "LDS %u with %u rows per workgroup", pl.lds_bytes, pl.fy);
    REQUIRE((uint64_t)n * 4u <= (uint64_t)pl.fy * M * 8u && K <= n, "the staged window and the bank's powers inside one buffer");
    REQUIRE(pl.rows == s.batch * s.frames && pl.groups == (pl.rows + pl.fy - 1) / pl.fy, "rows %" PRIu64 " groups %" PRIu64, pl.rows, pl.groups);
    REQUIRE(pl.grid >= 1 && pl.grid <= kFftMaxGrid && pl.grid <= pl.groups && (pl.grid == pl.groups || pl.grid == kFftMaxGrid), "grid %" PRIu64, pl.grid);
    REQUIRE(pl.y_stride >= W && pl.x_stride >= s.samples, "strides");
    REQUIRE(pl.detrend == ((flags & BHW_WELCH_DETREND_CONSTANT) != 0), "flags 0x%x", flags);
    REQUIRE(pl.form == (!(flags & BHW_MFFT_POWER) ? BHWP_MFFT_SPECTRUM : fb ? BHWP_MFFT_BANK : BHWP_MFFT_POWER), "form %u", pl.form);
}

// the group loop, the columns, the loads and the stores of every lane
static void replay_rows(const BhwStftMfftPlan &pl, const bhw_stft &s, uint64_t L, const bhw_fbank *fb)
{
    const uint64_t F = s.frames, B = s.batch, T = s.samples, n = s.n_fft, M = n / 2, K = M + 1;
    const uint64_t W = pl.form == BHWP_MFFT_SPECTRUM ? 2 * K : pl.form == BHWP_MFFT_BANK ? fb->filters : K;
    const uint64_t per = pl.form == BHWP_MFFT_SPECTRUM ? 2 : 1, cols = W / per;
    std::vector<int> owned(pl.rows, 0), written(pl.rows * cols, 0), column(pl.rows * n, 0);
    const uint64_t yext = (B - 1) * pl.y_bstride + (F - 1) * pl.y_stride + W, xext = (B - 1) * pl.x_stride + T;
    for (uint64_t wg = 0; wg < pl.grid; ++wg)
        for (uint64_t g = wg; g < pl.groups; g += pl.grid)
            for (uint32_t tid = 0; tid < kFftBlock; ++tid) {
                const uint32_t slot = tid / pl.lpf, l = tid - slot * pl.lpf;
                REQUIRE(slot < pl.fy, "slot %u", slot);
                const uint64_t r = g * pl.fy + slot;
                if (r >= pl.rows) continue;
                const uint64_t b = r / F, f = r - b * F;
                REQUIRE(b < B, "row %" PRIu64, r);
                if (l == 0) ++owned[r];
                for (uint32_t c = 0; c < kFftMaxCpl; ++c) {
                    const uint32_t j = c * pl.lpf + l;
                    if (!(c < pl.cpl && j < n)) continue;                   // the column test
                    ++column[r * n + j];
                    if ((uint32_t)(j - (uint32_t)s.col0) >= L) continue;
                    uint64_t t = f * s.hop + j - s.pad;
                    if (t >= T) {
                        const int64_t ts = (int64_t)t;
                        if (s.pad_mode == BHW_PAD_REFLECT) t = ts < 0 ? (uint64_t)(-ts) : 2 * (T - 1) - t;
                        else t = 0;
                    }
                    REQUIRE(t < T && b * pl.x_stride + t + 1 <= xext, "frame %" PRIu64 " column %u reads sample %" PRIu64 " of %" PRIu64, f, j, t, T);
                }
                if (pl.form != BHWP_MFFT_BANK) {
                    for (uint64_t k = l; k <= M; k += pl.lpf) {
                        const uint64_t yi = b * pl.y_bstride + f * pl.y_stride + per * k;
                        REQUIRE(yi + per <= yext && per * k + per <= W && W <= pl.y_stride, "output index %" PRIu64, yi);
                        ++written[r * cols + k];
                    }
                } else {
                    for (uint64_t m = l; m < fb->filters; m += pl.lpf) {
                        const uint64_t yi = b * pl.y_bstride + f * pl.y_stride + m;
                        REQUIRE(yi + 1 <= yext && m < W && W <= pl.y_stride, "output index %" PRIu64, yi);
                        ++written[r * cols + m];
                    }
                }
            }
    for (uint64_t r = 0; r < pl.rows; ++r) REQUIRE(owned[r] == 1, "row %" PRIu64 " owned %d times", r, owned[r]);
    for (uint64_t i = 0; i < pl.rows * cols; ++i) REQUIRE(written[i] == 1, "output column %" PRIu64 " written %d times", i, written[i]);
    for (uint64_t i = 0; i < pl.rows * n; ++i) REQUIRE(column[i] == 1, "row column %" PRIu64 " held %d times", i, column[i]);
}

// the bank's clamps: random and hostile first / offset
static long replay_bank(uint32_t K, uint32_t filters, uint32_t weights)
{
    long reads = 0;
    for (int trial = 0; trial < 4; ++trial)
        for (uint32_t m = 0; m < filters; ++m) {
            uint32_t o0 = trial == 0 ? 0xFFFFFFFFu : (uint32_t)rnd(), o1 = trial == 1 ? 0xFFFFFFFFu : (uint32_t)rnd();
            uint32_t k0 = trial == 2 ? K - 1 : (uint32_t)rnd();
            if (trial == 3) {
                o0 %= weights + 1;
                o1 %= weights + 1;
                k0 %= K + 2;
            }
            const uint32_t W = weights;
            o0 = o0 < W ? o0 : W;
            o1 = o1 < W ? o1 : W;
            o1 = o1 < o0 ? o0 : o1;
            uint32_t c = o1 - o0;
            const uint32_t room = k0 < K ? K - k0 : 0u;
            c = c < room ? c : room;
            for (uint32_t i = 0; i < c; ++i) {
                REQUIRE(k0 + i < K && o0 + i < weights, "filter %u reads power %u of %u, weight %u of %u", m, k0 + i, K, o0 + i, weights);
                ++reads;
            }
        }
    return reads;
}

// the mean of a row of L floats: the kernel's wave against the header's order
static void replay_mean(uint32_t L)
{
    std::vector<float> row(L);
    for (auto &v : row) v = (float)(uniform() * 2000.0 + 250.0);
    double P[64];
    for (uint32_t lane = 0; lane < 64; ++lane) {
        P[lane] = 0.0;
        for (uint32_t j = lane; j < L; j += 64u) P[lane] += (double)row[j];
    }
    double S[64];
    for (int i = 0; i < 64; ++i) S[i] = 0.0;
    for (uint32_t j = 0; j < L; ++j) S[j % 64] += (double)row[j];          // 64 partial sums by j mod 64 in ascending j
    for (int sh = 32; sh >= 1; sh >>= 1) {
        double Q[64];
        for (int i = 0; i < 64; ++i) Q[i] = P[i] + (i + sh < 64 ? P[i + sh] : P[i]);   // __shfl_down past the wave: the lane's own
        memcpy(P, Q, sizeof P);
        for (int i = 0; i < sh; ++i) S[i] += S[i + sh];
    }
    const float a = (float)(P[0] / (double)L), b = (float)(S[0] / (double)L);
    REQUIRE(memcmp(&a, &b, 4) == 0, "mean of %u", L);
}

struct C32 {
    float x, y;
};
static C32 cmul(C32 a, C32 w) { return C32{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }
static C32 add(C32 a, C32 b) { return C32{a.x + b.x, a.y + b.y}; }
static C32 sub(C32 a, C32 b) { return C32{a.x - b.x, a.y - b.y}; }
static C32 scl(float s, C32 a) { return C32{s * a.x, s * a.y}; }

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
        a[1] = C32{t2.x + t3.y, t2.y - t3.x};
        a[2] = C32{t2.x - t3.y, t2.y + t3.x};
    } else if (R == 4) {
        const C32 t0 = add(a[0], a[2]), t1 = sub(a[0], a[2]), t2 = add(a[1], a[3]);
        const C32 t3 = C32{a[1].y - a[3].y, a[3].x - a[1].x};
        a[0] = add(t0, t2);
        a[1] = add(t1, t3);
        a[2] = sub(t0, t2);
        a[3] = sub(t1, t3);
    } else {
        const C32 b1 = add(a[1], a[4]), b2 = add(a[2], a[3]), d1 = sub(a[1], a[4]), d2 = sub(a[2], a[3]);
        const C32 m1 = add(add(a[0], scl(kCos5a, b1)), scl(kCos5b, b2)), m2 = add(add(a[0], scl(kCos5b, b1)), scl(kCos5a, b2));
        const C32 n1 = add(scl(kSin5a, d1), scl(kSin5b, d2)), n2 = sub(scl(kSin5b, d1), scl(kSin5a, d2));
        a[0] = add(add(a[0], b1), b2);
        a[1] = C32{m1.x + n1.y, m1.y - n1.x};
        a[4] = C32{m1.x - n1.y, m1.y + n1.x};
        a[2] = C32{m2.x + n2.y, m2.y - n2.x};
        a[3] = C32{m2.x - n2.y, m2.y + n2.x};
    }
}

// the passes and the split pass of one row, lane by lane; returns the relative l2 error against a direct binary64 DFT
static long g_butterflies = 0, g_idle = 0, g_trips = 0;
static double replay_fft(const BhwStftMfftPlan &pl, uint32_t n)
{
    const uint32_t M = n / 2, lpf = pl.lpf;
    std::vector<float> row(n);
    for (auto &v : row) v = (float)(uniform() * 2000.0);
    std::vector<C32> A(M), Bf(M), tw(M);
    const double pi = 3.14159265358979323846;
    for (uint32_t k = 0; k < M; ++k) tw[k] = C32{(float)cos(2.0 * pi * k / n), (float)-sin(2.0 * pi * k / n)};
    for (uint32_t i = 0; i < M; ++i) A[i] = C32{row[2 * i], row[2 * i + 1]};
    C32 *src = A.data(), *dst = Bf.data();
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
        if (Q < lpf) ++g_idle;
        if (Q > lpf) ++g_trips;
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
                const uint32_t o = (i - k) * R + k;
                for (uint32_t q = 0; q < R; ++q) {
                    REQUIRE(o + q * Ns < M, "write %u", o + q * Ns);
                    ++wr[o + q * Ns];
                    dst[o + q * Ns] = a[q];
                }
                ++g_butterflies;
            }
        for (uint32_t i = 0; i < M; ++i) REQUIRE(rd[i] == 1 && wr[i] == 1, "n_fft %u pass %u point %u read %d written %d", n, p, i, rd[i], wr[i]);
        C32 *sw = src;
        src = dst;
        dst = sw;
        Ns *= R;
    }
    REQUIRE(Ns == M && rest == 1, "the passes transform %u of %u points", Ns, M);
    // the split pass against the direct transform
    std::vector<double> cs(n), sn(n);
    for (uint32_t k = 0; k < n; ++k) {
        cs[k] = cos(2.0 * pi * k / n);
        sn[k] = sin(2.0 * pi * k / n);
    }
    double ne = 0.0, nr = 0.0;
    std::vector<int> bins(M + 1, 0);
    for (uint32_t l = 0; l < lpf; ++l)
        for (uint32_t k = l; k <= M; k += lpf) {
            ++bins[k];
            C32 y;
            if (k == 0u || k == M) {
                const C32 z = src[0];
                y = C32{k ? z.x - z.y : z.x + z.y, 0.0f};
            } else {
                REQUIRE(M - k < M && k < M, "split reads %u", k);
                const C32 Az = src[k], Bz = src[M - k], w = tw[k];
                const C32 E = C32{0.5f * (Az.x + Bz.x), 0.5f * (Az.y - Bz.y)};
                const C32 O = C32{0.5f * (Az.y + Bz.y), 0.5f * (Bz.x - Az.x)};
                y = add(E, cmul(O, w));
            }
            double re = 0.0, im = 0.0;
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t at = (uint32_t)(((uint64_t)j * k) % n);
                re += (double)row[j] * cs[at];
                im -= (double)row[j] * sn[at];
            }
            ne += ((double)y.x - re) * ((double)y.x - re) + ((double)y.y - im) * ((double)y.y - im);
            nr += re * re + im * im;
            if (k == 0u || k == M) REQUIRE(y.y == 0.0f && !std::signbit(y.y), "bin %u has an imaginary part", k);
        }
    for (uint32_t k = 0; k <= M; ++k) REQUIRE(bins[k] == 1, "bin %u formed %d times", k, bins[k]);
    return sqrt(ne / nr);
}

int main()
{
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 12, 24);
    long sizes = 0, refused = 0, plans = 0;
    double worst = 0.0;
    uint32_t max_cpl = 0, max_lds = 0, max_lds_shared = 0;
    char line[1024], sched[48];
    for (uint32_t n = 1; n <= 5000; ++n) {
        const bhw_stft probe = desc_of(2, 100000, 3, 7, n, 0, 0, 0);
        const int rc = bhwp_stft_mfft_checks(&p, n < 16 ? n : 16, &probe, 0, nullptr, nullptr, nullptr, false);
        REQUIRE(bhwp_mfft_supported(n) == supported(n), "n_fft %u", n);
        if (!supported(n)) {
            REQUIRE(rc == BHW_ERR_UNSUPPORTED, "n_fft %u: rc %d", n, rc);
            ++refused;
            continue;
        }
        REQUIRE(rc == BHW_OK, "n_fft %u: rc %d", n, rc);
        ++sizes;
        const uint32_t M = n / 2, K = M + 1;
        // every flag combination and form, at row counts at the edges of a group and of the grid
        for (uint32_t flags = 0; flags < 4; ++flags)
            for (int bank = 0; bank < ((flags & BHW_MFFT_POWER) ? 2 : 1); ++bank)
                for (uint64_t rows : {1ull, 3ull, 63ull, 64ull, 65ull, 257ull, 2048ull, 2049ull, 64ull * 2048 + 1}) {
                    bhw_stft s = desc_of(1, (rows - 1) * 7 + n, rows, 7, n, 0, 0, 0);
                    bhw_fbank fb = bank_of(80, K, 1000);
                    const bhw_fbank *fbp = bank ? &fb : nullptr;
                    REQUIRE(bhwp_stft_mfft_checks(&p, n, &s, flags, fbp, nullptr, nullptr, false) == BHW_OK, "n_fft %u flags %u", n, flags);
                    const BhwStftMfftPlan pl = bhwp_stft_mfft_plan(&p, n, &s, flags, fbp, bank != 0);
                    plan_invariants(pl, s, flags, fbp);
                    REQUIRE(bhwp_describe_stft_mfft(&p, nullptr, n, &s, flags, fbp, line, sizeof line) == BHW_OK && strstr(line, "stft mfft"), "describe");
                    ++plans;
                    max_cpl = pl.cpl > max_cpl ? pl.cpl : max_cpl;
                    max_lds = pl.lds_bytes > max_lds ? pl.lds_bytes : max_lds;
                    if (pl.fy > 1) max_lds_shared = pl.lds_bytes > max_lds_shared ? pl.lds_bytes : max_lds_shared;
                }
        // the rows, lane by lane: centred under both padding modes with L < n_fft, the Welch segments with detrending, padded strides
        const uint64_t L = n - n / 5, hop = n / 3 + 1;
        for (uint32_t mode : {(uint32_t)BHW_PAD_CONSTANT, (uint32_t)BHW_PAD_REFLECT})
            for (uint32_t form = 0; form < 3; ++form) {
                const uint64_t T = 3 * n + 11, pad = n / 2, frames = 1 + (T + 2 * pad - n) / hop;
                bhw_stft s = desc_of(3, T, frames, hop, n, (n - L) / 2, pad, mode);
                const uint32_t flags = form ? BHW_MFFT_POWER : 0;
                bhw_fbank fb = bank_of(37, K, 500);
                const bhw_fbank *fbp = form == 2 ? &fb : nullptr;
                const uint64_t W = form == 0 ? 2 * K : form == 1 ? K : fb.filters;
                if (mode == BHW_PAD_REFLECT) {
                    s.x_stride = T + 5;
                    s.y_stride = W + (form ? 5 : 6);
                    s.y_batch_stride = frames * s.y_stride + (form ? 7 : 10);
                }
                REQUIRE(bhwp_stft_mfft_checks(&p, L, &s, flags, fbp, nullptr, nullptr, false) == BHW_OK, "n_fft %u centred", n);
                replay_rows(bhwp_stft_mfft_plan(&p, L, &s, flags, fbp, false), s, L, fbp);
            }
        {
            const uint64_t T = 5 * n + 3, frames = 1 + (T - L) / hop;
            bhw_stft s = desc_of(2, T, frames, hop, n, 0, 0, 0);
            REQUIRE(bhwp_stft_mfft_checks(&p, L, &s, BHW_WELCH_DETREND_CONSTANT, nullptr, nullptr, nullptr, false) == BHW_OK, "n_fft %u segments", n);
            replay_rows(bhwp_stft_mfft_plan(&p, L, &s, BHW_WELCH_DETREND_CONSTANT, nullptr, true), s, L, nullptr);
            replay_mean((uint32_t)L);
            replay_mean(n);
        }
        replay_bank(K, 80, 1000);
        // the transform
        const bhw_stft s = desc_of(1, n, 1, 1, n, 0, 0, 0);
        const BhwStftMfftPlan pl = bhwp_stft_mfft_plan(&p, n, &s, 0, nullptr, false);
        const double err = replay_fft(pl, n), cap = ldexp(1.0, -24) * log2((double)n);
        REQUIRE(err <= cap, "n_fft %u: float passes %.3e against the direct transform, cap %.3e", n, err, cap);
        worst = err / cap > worst ? err / cap : worst;
        bhwp_stft_mfft_schedule(pl, sched, sizeof sched);
        if (n == 400) REQUIRE(!strcmp(sched, "5x5x4x2"), "%s", sched);
        if (n == 480) REQUIRE(!strcmp(sched, "5x3x4x4"), "%s", sched);
        if (n == 18) REQUIRE(!strcmp(sched, "3x3"), "%s", sched);
        if (n == 4050) REQUIRE(!strcmp(sched, "5x5x3x3x3x3") && pl.cpl == 16 && pl.lds_bytes <= 49800u, "%s", sched);
    }
    REQUIRE(max_cpl == 16 && max_lds <= 65536u && max_lds_shared <= 20488u, "cpl %u, LDS %u / %u", max_cpl, max_lds, max_lds_shared);
    // the refusals of the checks
    {
        bhw_stft s = desc_of(2, 16000, 98, 160, 400, 0, 0, 0);
        bhw_fbank fb = bank_of(80, 201, 1000);
        REQUIRE(bhwp_stft_mfft_checks(&p, 400, &s, 4, nullptr, nullptr, nullptr, false) == BHW_ERR_BADARG, "unknown flag");
        REQUIRE(bhwp_stft_mfft_checks(&p, 400, &s, 0, &fb, nullptr, nullptr, false) == BHW_ERR_BADARG, "a bank without the power flag");
        REQUIRE(bhwp_stft_mfft_checks(&p, 400, &s, 2, &fb, nullptr, nullptr, false) == BHW_OK, "a bank");
        fb.bins = 257;
        REQUIRE(bhwp_stft_mfft_checks(&p, 400, &s, 2, &fb, nullptr, nullptr, false) == BHW_ERR_BADARG, "bins");
        s.channels = 2;
        REQUIRE(bhwp_stft_mfft_checks(&p, 400, &s, 0, nullptr, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED, "channels 2");
        s.channels = 1;
        s.n_fft = 512;
        REQUIRE(bhwp_stft_mfft_checks(&p, 400, &s, 0, nullptr, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED && strstr(bhw_last_error(), "bhw_stft_fft_f32_"), "a power of two");
        s.n_fft = 400;
        s.y_stride = 403;
        REQUIRE(bhwp_stft_mfft_checks(&p, 400, &s, 0, nullptr, nullptr, nullptr, false) == BHW_ERR_BADARG, "an odd spectrum stride");
        REQUIRE(bhwp_stft_mfft_checks(&p, 400, &s, 2, nullptr, nullptr, nullptr, false) == BHW_OK, "an odd power stride");
        s.y_stride = 0;
        REQUIRE(bhwp_stft_mfft_checks(&p, 400, &s, 0, nullptr, (const void *)0x1000, (const void *)0x100004, true) == BHW_ERR_BADARG, "alignment");
        REQUIRE(bhwp_stft_mfft_checks(&p, 400, &s, 2, nullptr, (const void *)0x1000, (const void *)0x10000004, true) == BHW_OK, "power rows are 4-byte aligned");
    }
    printf("ok %ld checks, %ld sizes, %ld refused, %ld plans, %ld butterflies, %ld passes with idle lanes, %ld with several trips, worst error %.3f of the cap\n",
           g_checks, sizes, refused, plans, g_butterflies, g_idle, g_trips, worst);
    return 0;
}
