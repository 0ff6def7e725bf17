// san_stft_cmfft.cpp -- the planner's part of the mixed-radix fused window + complex FFT calls for I/Q input (bhw_plan.cpp:
// bhwp_stft_cmfft_checks / bhwp_stft_cmfft_plan / bhwp_describe_stft_cmfft) swept under AddressSanitizer + UBSan over EVERY supported
// n_fft (91 sizes, 18 of them odd), every flag combination and both routes.  Besides "no report" it asserts the plan's invariants --
// lanes x rows = the workgroup, lanes per row the smallest power of two >= n / 4 in 4..256, columns per lane ceil(n / lanes) <= 8, the
// schedule 5s, 3s, 4s and a last 2 whose product is n, the twiddle entries n / 2 (even n) or n (odd n), the LDS formula and 64 KiB,
// the window staged inside the first buffer -- and replays on the host the kernel's index arithmetic (bhw_stft_cmfft.h):
//   - ownership: every row (b, f) of the pool is taken by exactly one (workgroup, trip of the group loop, slot);
//   - the columns: c * lpf + l < n is the column test; every column of a row belongs to exactly one (lane, c);
//   - the loads: every window column of every row reads a complex sample inside its signal under both padding modes;
//   - the means: one wave per row, lane i over j = i, i + 64, ..., then the shuffle butterfly, per part, against the order bhw.h
//     writes down, bit for bit on binary64 sums of float32 data;
//   - the passes: i mod Ns by the float multiply against the integer remainder for every (i, Ns) the schedule produces, every point
//     read exactly once and written exactly once per pass, every twiddle index < n and below fold after the fold (never folded at an
//     odd n), and the passes IN FLOAT, with float32-rounded binary64 twiddles and butterfly constants, against a direct binary64 DFT of
//     the float32 row within 2^-24 * log2(n) in relative l2 error;
//   - the stores: every output column of every row written exactly once in both forms, with and without the shift, at the column
//     (k + n / 2) mod n of torch.fft.fftshift, inside the row's floats and the output's extent, never in a gap.
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
    s.channels = 2;
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

static bool supported(uint64_t n)
{
    if (n < 16 || n > 2047 || !(n & (n - 1))) return false;
    for (uint64_t r : {2, 3, 5})
        while (n % r == 0) n /= r;
    return n == 1;
}

static void plan_invariants(const BhwStftCmfftPlan &pl, const bhw_stft &s, uint32_t flags, bool from_table)
{
    const uint32_t n = (uint32_t)s.n_fft;
    const uint64_t W = (flags & BHW_CFFT_POWER) ? n : 2 * n;
    REQUIRE(pl.n == n && pl.lpf * pl.fy == kFftBlock && pl.lpf >= 4 && pl.lpf <= kFftBlock && !(pl.lpf & (pl.lpf - 1)), "lanes %u x %u", pl.lpf, pl.fy);
    REQUIRE((4 * pl.lpf >= n || pl.lpf == kFftBlock) && (pl.lpf == 4 || 4 * (pl.lpf / 2) < n), "lanes per row %u for n %u", pl.lpf, n);
    REQUIRE(pl.cpl == (n + pl.lpf - 1) / pl.lpf && pl.cpl <= kCfftMaxCpl && pl.cpl >= 3, "%u columns per lane", pl.cpl);
    REQUIRE(pl.fold == ((n & 1u) ? n : n / 2), "%u twiddles for n %u", pl.fold, n);
    uint32_t prod = 1, last = 5;
    static const int rank[6] = {0, 0, 3, 1, 2, 0};                       // 5 < 3 < 4 < 2 in schedule order
    REQUIRE(pl.passes >= 2 && pl.passes <= 7 && pl.passes <= kMfftMaxPasses, "%u passes", pl.passes);
    for (uint32_t i = 0; i < pl.passes; ++i) {
        const uint32_t r = pl.radix[i];
        REQUIRE(r == 2 || r == 3 || r == 4 || r == 5, "radix %u", r);
        REQUIRE(rank[r] >= rank[last], "radix %u after %u", r, last);
        REQUIRE(r != 2 || i + 1 == pl.passes, "a radix-2 pass that is not the last");
        REQUIRE((n & 1u) == 0 || (r != 2 && r != 4), "an even radix at an odd n");
        last = r;
        prod *= r;
    }
    REQUIRE(prod == n, "the schedule transforms %u points, n = %u", prod, n);
    REQUIRE(pl.lds_bytes == 2u * pl.fy * n * 8u + pl.fold * 8u + pl.fy * 8u && pl.lds_bytes <= 65536u, "LDS %u", pl.lds_bytes);
    REQUIRE((uint64_t)n * 4u <= (uint64_t)pl.fy * n * 8u, "the staged window inside the first buffer");
    REQUIRE(pl.rows == s.batch * s.frames && pl.groups == (pl.rows + pl.fy - 1) / pl.fy, "rows %" PRIu64 " groups %" PRIu64, pl.rows, pl.groups);
    REQUIRE(pl.grid >= 1 && pl.grid <= kFftMaxGrid && pl.grid <= pl.groups && (pl.grid == pl.groups || pl.grid == kFftMaxGrid), "grid %" PRIu64, pl.grid);
    REQUIRE(pl.y_stride >= W && pl.x_stride >= 2 * s.samples, "strides");
    REQUIRE(pl.detrend == ((flags & BHW_WELCH_DETREND_CONSTANT) != 0) && pl.power == ((flags & BHW_CFFT_POWER) != 0) &&
            pl.shifted == ((flags & BHW_CFFT_SHIFT) != 0), "flags 0x%x", flags);
    REQUIRE(pl.route == (from_table ? BHWP_FRAMES_TABLE : BHWP_FRAMES_DIRECT), "route %d", pl.route);
}

// the group loop, the columns, the loads and the stores of every lane
static void replay_rows(const BhwStftCmfftPlan &pl, const bhw_stft &s, uint64_t L)
{
    const uint64_t F = s.frames, B = s.batch, T = s.samples, n = s.n_fft;
    const uint64_t per = pl.power ? 1 : 2, W = per * n;
    std::vector<int> owned(pl.rows, 0), written(pl.rows * n, 0), column(pl.rows * n, 0);
    const uint64_t yext = (B - 1) * pl.y_bstride + (F - 1) * pl.y_stride + W, xext = (B - 1) * pl.x_stride + 2 * T;
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
                for (uint32_t c = 0; c < kCfftMaxCpl; ++c) {
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
                    REQUIRE(t < T && b * pl.x_stride + 2 * t + 2 <= xext, "frame %" PRIu64 " column %u reads sample %" PRIu64 " of %" PRIu64, f, j, t, T);
                }
                const uint32_t turn = pl.shifted ? (uint32_t)n >> 1 : 0u;
                for (uint32_t k = l; k < n; k += pl.lpf) {
                    uint32_t col = k + turn;
                    col = col >= n ? col - (uint32_t)n : col;
                    REQUIRE(col < n && col == (k + (pl.shifted ? n / 2 : 0)) % n, "bin %u to column %u", k, col);
                    const uint64_t yi = b * pl.y_bstride + f * pl.y_stride + per * col;
                    REQUIRE(yi + per <= yext && per * col + per <= W && W <= pl.y_stride, "output index %" PRIu64, yi);
                    ++written[r * n + col];
                }
            }
    for (uint64_t r = 0; r < pl.rows; ++r) REQUIRE(owned[r] == 1, "row %" PRIu64 " owned %d times", r, owned[r]);
    for (uint64_t i = 0; i < pl.rows * n; ++i) REQUIRE(written[i] == 1, "output column %" PRIu64 " written %d times", i, written[i]);
    for (uint64_t i = 0; i < pl.rows * n; ++i) REQUIRE(column[i] == 1, "row column %" PRIu64 " held %d times", i, column[i]);
}

// the two means of a row of L complex samples: the kernel's wave against the header's order, per part
static void replay_means(uint32_t L)
{
    std::vector<float> row(2 * (size_t)L);
    for (auto &v : row) v = (float)(uniform() * 2000.0 + 250.0);
    for (uint32_t part = 0; part < 2; ++part) {
        double P[64], S[64];
        for (uint32_t lane = 0; lane < 64; ++lane) {
            P[lane] = 0.0;
            for (uint32_t j = lane; j < L; j += 64u) P[lane] += (double)row[2 * j + part];
        }
        for (int i = 0; i < 64; ++i) S[i] = 0.0;
        for (uint32_t j = 0; j < L; ++j) S[j % 64] += (double)row[2 * j + part];   // 64 partial sums by j mod 64 in ascending j
        for (int sh = 32; sh >= 1; sh >>= 1) {
            double Q[64];
            for (int i = 0; i < 64; ++i) Q[i] = P[i] + (i + sh < 64 ? P[i + sh] : P[i]);   // __shfl_down past the wave: the lane's own
            memcpy(P, Q, sizeof P);
            for (int i = 0; i < sh; ++i) S[i] += S[i + sh];
        }
        const float a = (float)(P[0] / (double)L), b = (float)(S[0] / (double)L);
        REQUIRE(memcmp(&a, &b, 4) == 0, "mean of part %u of %u", part, L);
    }
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

// the passes of one row of n complex points, lane by lane, as stft_cmfft_rows calls mfft_pass (M = fold, Q = n / R, ts = n / (R Ns));
// returns the relative l2 error against a direct binary64 DFT
static long g_butterflies = 0, g_idle = 0, g_trips = 0, g_folds = 0;
static double replay_fft(const BhwStftCmfftPlan &pl)
{
    const uint32_t n = pl.n, fold = pl.fold, lpf = pl.lpf;
    std::vector<C32> row(n), A(n), Bf(n), tw(fold);
    for (auto &v : row) v = C32{(float)(uniform() * 2000.0), (float)(uniform() * 2000.0)};
    const double pi = 3.14159265358979323846;
    for (uint32_t k = 0; k < fold; ++k) tw[k] = C32{(float)cos(2.0 * pi * k / n), (float)-sin(2.0 * pi * k / n)};
    A = row;
    C32 *src = A.data(), *dst = Bf.data();
    uint32_t Ns = 1, rest = n;
    for (uint32_t p = 0; p < pl.passes; ++p) {
        const uint32_t R = pl.radix[p];
        REQUIRE(rest % R == 0, "pass %u of radix %u over %u", p, R, rest);
        rest /= R;
        const uint32_t Q = n / R, ts = rest;
        REQUIRE((uint64_t)ts * R * Ns == n && Ns < 2048u, "twiddle stride %u", ts);
        std::vector<int> rd(n, 0), wr(n, 0);
        const float inv = 1.0f / (float)Ns;
        // a reciprocal one ulp off either way gives the same quotients (the hardware's is not correctly rounded)
        const float inv_lo = nextafterf(inv, 0.0f), inv_hi = nextafterf(inv, 2.0f);
        if (Q < lpf) ++g_idle;
        if (Q > lpf) ++g_trips;
        for (uint32_t l = 0; l < lpf; ++l)
            for (uint32_t i = l; i < Q; i += lpf) {
                C32 a[5];
                for (uint32_t q = 0; q < R; ++q) {
                    REQUIRE(i + q * Q < n, "read %u", i + q * Q);
                    ++rd[i + q * Q];
                    a[q] = src[i + q * Q];
                }
                uint32_t k = i;
                if (Ns < Q) {
                    const uint32_t d = (uint32_t)(((float)i + 0.5f) * inv);
                    REQUIRE(d == i / Ns && d == (uint32_t)(((float)i + 0.5f) * inv_lo) && d == (uint32_t)(((float)i + 0.5f) * inv_hi), "%u / %u", i, Ns);
                    k = i - d * Ns;
                } else {
                    REQUIRE(Ns == Q && p + 1 == pl.passes, "k = i outside the last pass");
                }
                REQUIRE(k == i % Ns, "%u mod %u", i, Ns);
                if (Ns > 1u) {
                    const uint32_t kt = k * ts;
                    for (uint32_t q = 1; q < R; ++q) {
                        const uint32_t idx = q * kt;
                        REQUIRE(idx < n, "twiddle index %u of %u", idx, n);
                        const bool hi = idx >= fold;
                        REQUIRE(!hi || !(n & 1u), "a fold at the odd n %u", n);
                        const uint32_t at = hi ? idx - fold : idx;
                        REQUIRE(at < fold, "folded twiddle index %u", at);
                        g_folds += hi;
                        const C32 w = hi ? C32{-tw[at].x, -tw[at].y} : tw[at];
                        a[q] = cmul(a[q], w);
                    }
                }
                butterfly(R, a);
                const uint32_t o = (i - k) * R + k;
                for (uint32_t q = 0; q < R; ++q) {
                    REQUIRE(o + q * Ns < n, "write %u", o + q * Ns);
                    ++wr[o + q * Ns];
                    dst[o + q * Ns] = a[q];
                }
                ++g_butterflies;
            }
        for (uint32_t i = 0; i < n; ++i) REQUIRE(rd[i] == 1 && wr[i] == 1, "n_fft %u pass %u point %u read %d written %d", n, p, i, rd[i], wr[i]);
        C32 *sw = src;
        src = dst;
        dst = sw;
        Ns *= R;
    }
    REQUIRE(Ns == n && rest == 1, "the passes transform %u of %u points", Ns, n);
    std::vector<double> cs(n), sn(n);
    for (uint32_t k = 0; k < n; ++k) {
        cs[k] = cos(2.0 * pi * k / n);
        sn[k] = sin(2.0 * pi * k / n);
    }
    double ne = 0.0, nr = 0.0;
    for (uint32_t k = 0; k < n; ++k) {
        double re = 0.0, im = 0.0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t at = (uint32_t)(((uint64_t)j * k) % n);
            re += (double)row[j].x * cs[at] + (double)row[j].y * sn[at];
            im += (double)row[j].y * cs[at] - (double)row[j].x * sn[at];
        }
        ne += ((double)src[k].x - re) * ((double)src[k].x - re) + ((double)src[k].y - im) * ((double)src[k].y - im);
        nr += re * re + im * im;
    }
    return sqrt(ne / nr);
}

int main()
{
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 12, 24);
    long sizes = 0, odd = 0, refused = 0, plans = 0;
    double worst = 0.0;
    uint32_t max_cpl = 0, max_lds = 0, max_passes = 0, worst_n = 0;
    char line[1024], tline[1024];
    BhwCordicCfg tc;
    memset(&tc, 0, sizeof tc);
    for (uint32_t n = 1; n <= 5000; ++n) {
        const bhw_stft probe = desc_of(2, 100000, 3, 7, n, 0, 0, 0);
        const int rc = bhwp_stft_cmfft_checks(&p, n < 16 ? n : 16, &probe, 0, nullptr, nullptr, false);
        REQUIRE(bhwp_cmfft_supported(n) == supported(n), "n_fft %u", n);
        if (!supported(n)) {
            REQUIRE(rc == BHW_ERR_UNSUPPORTED, "n_fft %u: rc %d", n, rc);
            if (n >= 16 && !(n & (n - 1))) REQUIRE(strstr(bhw_last_error(), "bhw_stft_cfft_f32_"), "a power of two names the other route");
            ++refused;
            continue;
        }
        REQUIRE(rc == BHW_OK, "n_fft %u: rc %d", n, rc);
        ++sizes;
        odd += n & 1u;
        // every flag combination and both routes, at row counts at the edges of a group and of the grid
        for (uint32_t flags = 0; flags < 8; ++flags)
            for (int table = 0; table < 2; ++table)
                for (uint64_t rows : {1ull, 3ull, 31ull, 32ull, 33ull, 257ull, 2048ull, 2049ull, 32ull * 2048 + 1}) {
                    bhw_stft s = desc_of(1, (rows - 1) * 7 + n, rows, 7, n, 0, 0, 0);
                    REQUIRE(bhwp_stft_cmfft_checks(&p, n, &s, flags, nullptr, nullptr, false) == BHW_OK, "n_fft %u flags %u", n, flags);
                    const BhwStftCmfftPlan pl = bhwp_stft_cmfft_plan(&p, n, &s, flags, table != 0);
                    plan_invariants(pl, s, flags, table != 0);
                    const BhwStftCmfftPlan other = bhwp_stft_cmfft_plan(&p, n, &s, flags, table == 0);
                    REQUIRE(other.lpf == pl.lpf && other.fy == pl.fy && other.cpl == pl.cpl && other.fold == pl.fold && other.passes == pl.passes &&
                            !memcmp(other.radix, pl.radix, sizeof pl.radix) && other.lds_bytes == pl.lds_bytes && other.groups == pl.groups &&
                            other.grid == pl.grid, "the route changes the plan at n_fft %u", n);
                    ++plans;
                    max_cpl = pl.cpl > max_cpl ? pl.cpl : max_cpl;
                    max_lds = pl.lds_bytes > max_lds ? pl.lds_bytes : max_lds;
                    max_passes = pl.passes > max_passes ? pl.passes : max_passes;
                }
        {
            bhw_stft s = desc_of(2, 100000, 5, 7, n, 0, 0, 0);
            REQUIRE(bhwp_describe_stft_cmfft(&p, nullptr, 16, &s, 6, line, sizeof line) == BHW_OK && strstr(line, "stft cmfft direct") &&
                    strstr(line, "k_stft_cmfft_direct") && strstr(line, "power rows, bins shifted") && strstr(line, "(no split)"), "describe: %s", line);
            tc = BhwCordicCfg{};
            if (bhwp_describe_stft_cmfft(&p, &tc, 16, &s, 1, tline, sizeof tline) == BHW_OK)
                REQUIRE(strstr(tline, "stft cmfft table"), "describe: %s", tline);
            s.frames = 0;
            REQUIRE(bhwp_describe_stft_cmfft(&p, nullptr, 16, &s, 0, line, sizeof line) == BHW_OK && strstr(line, "nothing (frames 0)"), "describe: %s", line);
        }
        // the rows, lane by lane: centred under both padding modes with L < n_fft in all four forms, the Welch segments with detrending,
        // padded strides
        const uint64_t L = n - n / 5, hop = n / 3 + 1;
        for (uint32_t mode : {(uint32_t)BHW_PAD_CONSTANT, (uint32_t)BHW_PAD_REFLECT})
            for (uint32_t form = 0; form < 4; ++form) {
                const uint64_t T = 3 * n + 11, pad = n / 2, frames = 1 + (T + 2 * pad - n) / hop;
                bhw_stft s = desc_of(3, T, frames, hop, n, (n - L) / 2, pad, mode);
                const uint32_t flags = ((form & 1) ? BHW_CFFT_POWER : 0) | ((form & 2) ? BHW_CFFT_SHIFT : 0);
                const uint64_t W = (form & 1) ? n : 2 * n;
                if (mode == BHW_PAD_REFLECT) {
                    s.x_stride = 2 * T + 5;
                    s.y_stride = W + ((form & 1) ? 5 : 6);
                    s.y_batch_stride = frames * s.y_stride + ((form & 1) ? 7 : 10);
                }
                REQUIRE(bhwp_stft_cmfft_checks(&p, L, &s, flags, nullptr, nullptr, false) == BHW_OK, "n_fft %u centred: %s", n, bhw_last_error());
                replay_rows(bhwp_stft_cmfft_plan(&p, L, &s, flags, false), s, L);
            }
        {
            const uint64_t T = 5 * n + 3, frames = 1 + (T - L) / hop;
            bhw_stft s = desc_of(2, T, frames, hop, n, 0, 0, 0);
            const uint32_t flags = BHW_WELCH_DETREND_CONSTANT | BHW_CFFT_SHIFT;
            REQUIRE(bhwp_stft_cmfft_checks(&p, L, &s, flags, nullptr, nullptr, false) == BHW_OK, "n_fft %u segments", n);
            replay_rows(bhwp_stft_cmfft_plan(&p, L, &s, flags, true), s, L);
            replay_means((uint32_t)L);
            replay_means(n);
        }
        // the transform
        const bhw_stft s = desc_of(1, n, 1, 1, n, 0, 0, 0);
        const BhwStftCmfftPlan pl = bhwp_stft_cmfft_plan(&p, n, &s, 0, false);
        const double err = replay_fft(pl), cap = ldexp(1.0, -24) * log2((double)n);
        REQUIRE(err <= cap, "n_fft %u: float passes %.3e against the direct transform, cap %.3e", n, err, cap);
        if (err / cap > worst) {
            worst = err / cap;
            worst_n = n;
        }
    }
    REQUIRE(max_cpl == 8 && max_lds == 48608u && max_passes == 7, "cpl %u, LDS %u, %u passes", max_cpl, max_lds, max_passes);
    // the refusals of the checks
    {
        bhw_stft s = desc_of(2, 16000, 98, 160, 400, 0, 0, 0);
        REQUIRE(bhwp_stft_cmfft_checks(&p, 400, &s, 8, nullptr, nullptr, false) == BHW_ERR_BADARG, "unknown flag");
        REQUIRE(bhwp_stft_cmfft_checks(&p, 400, &s, 7, nullptr, nullptr, false) == BHW_OK, "every flag");
        s.channels = 1;
        REQUIRE(bhwp_stft_cmfft_checks(&p, 400, &s, 0, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED && strstr(bhw_last_error(), "bhw_stft_mfft_f32_"), "channels 1");
        s.channels = 2;
        s.n_fft = 512;
        REQUIRE(bhwp_stft_cmfft_checks(&p, 400, &s, 0, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED && strstr(bhw_last_error(), "bhw_stft_cfft_f32_"), "a power of two");
        s.n_fft = 420;
        REQUIRE(bhwp_stft_cmfft_checks(&p, 400, &s, 0, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED && strstr(bhw_last_error(), "2^a 3^b 5^c in 16..2047"), "a factor of 7");
        s.n_fft = 400;
        s.y_stride = 801;
        REQUIRE(bhwp_stft_cmfft_checks(&p, 400, &s, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "an odd spectrum stride");
        s.y_stride = 401;
        REQUIRE(bhwp_stft_cmfft_checks(&p, 400, &s, 2, nullptr, nullptr, false) == BHW_OK, "an odd power stride");
        s.y_stride = 0;
        REQUIRE(bhwp_stft_cmfft_checks(&p, 400, &s, 0, (const void *)0x1000, (const void *)0x10000004, true) == BHW_ERR_BADARG, "alignment");
        REQUIRE(bhwp_stft_cmfft_checks(&p, 400, &s, 2, (const void *)0x1000, (const void *)0x10000004, true) == BHW_OK, "power rows are 4-byte aligned");
        s.frames = 0;
        s.y_stride = 3;
        REQUIRE(bhwp_stft_cmfft_checks(&p, 400, &s, 0, nullptr, nullptr, true) == BHW_OK, "frames 0");
    }
    printf("ok %ld checks, %ld sizes, %ld odd, %ld refused, %ld plans, %ld butterflies, %ld folded twiddles, %ld passes with idle lanes, %ld with several "
           "trips, worst error %.3f of the cap at n_fft %u\n", g_checks, sizes, odd, refused, plans, g_butterflies, g_folds, g_idle, g_trips, worst, worst_n);
    return 0;
}
