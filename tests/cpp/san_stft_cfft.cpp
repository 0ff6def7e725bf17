// san_stft_cfft.cpp -- the planner's part of the fused window + complex FFT calls for I/Q input (bhw_plan.cpp: bhwp_stft_cfft_checks /
// bhwp_stft_cfft_plan / bhwp_describe_stft_cfft) swept under AddressSanitizer + UBSan over every supported n_fft and every flag
// combination against L, hop, batch and frames at the edges, padded and packed, centred and Welch framing.  Besides "no report" it
// asserts the plan's invariants -- LDS within 40 KiB + 8, lanes x rows = the workgroup, lanes x columns = n_fft, 4 or 8 columns per
// lane, the window staged inside the first buffer, the lanes, rows and passes of the real plan of 2 n_fft points -- and replays on the
// host the kernel's index arithmetic (bhw_stft_cfft.hip):
//   - ownership: every row (b, f) of the pool is taken by exactly one (workgroup, trip of the group loop, slot);
//   - the loads: every window column of every row reads a complex sample inside its signal under both padding modes;
//   - the mean: one wave per row with two accumulators, lane i over j = i, i + 64, ..., then the shuffle butterfly, against the order
//     bhw.h writes down, per channel, bit for bit on binary64 sums of float32 data;
//   - the passes: every butterfly reads and writes inside its row's n points, every point of the destination is written exactly once
//     per pass, every twiddle index is inside the table after folding, and the passes IN FLOAT, with float32-rounded binary64
//     twiddles, agree with a direct binary64 DFT of the float32 row within 2^-24 * log2(n_fft) in relative l2 error;
//   - the stores: every output column of every row written exactly once, with and without the shift, in both forms, inside the row's
//     floats and Y's extent, never in a gap.
#include <cinttypes>
#include <cmath>
#include <complex>
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

static void plan_invariants(const bhw_params &p, const BhwStftCfftPlan &pl, const bhw_stft &s, uint32_t flags)
{
    const uint64_t n = s.n_fft;
    const uint64_t W = (flags & BHW_CFFT_POWER) ? n : 2 * n;
    REQUIRE((1ull << pl.log2n) == n && pl.n == n, "log2n %u n %u", pl.log2n, pl.n);
    REQUIRE(pl.lpf * pl.fy == kFftBlock && (uint64_t)pl.lpf * pl.cpl == n && pl.cpl <= kCfftMaxCpl && (pl.cpl == 4 || pl.cpl == 8), "lanes %u x %u, %u columns", pl.lpf, pl.fy, pl.cpl);
    REQUIRE(pl.lpf >= 4 && (pl.lpf == n / 4 || pl.lpf == kFftBlock), "lanes per row %u", pl.lpf);
    REQUIRE(2 * pl.radix4 + pl.radix2 == pl.log2n && pl.radix2 <= 1, "schedule %u x 4, %u x 2", pl.radix4, pl.radix2);
    REQUIRE(pl.lds_bytes == 2u * pl.fy * pl.n * 8u + pl.n / 2u * 8u + pl.fy * 8u && pl.lds_bytes <= 2u * 2048u * 8u + 1024u * 8u + 8u, "LDS %u", pl.lds_bytes);
    REQUIRE(n * 4u <= (uint64_t)pl.fy * pl.n * 8u, "the staged window (%" PRIu64 " floats) inside the first buffer", n);
    REQUIRE(pl.rows == s.batch * s.frames && pl.groups == (pl.rows + pl.fy - 1) / pl.fy, "rows %" PRIu64 " groups %" PRIu64, pl.rows, pl.groups);
    REQUIRE(pl.grid >= 1 && pl.grid <= kFftMaxGrid && pl.grid <= pl.groups && (pl.grid == pl.groups || pl.grid == kFftMaxGrid), "grid %" PRIu64, pl.grid);
    REQUIRE(pl.y_stride >= W && pl.x_stride >= 2 * s.samples, "strides");
    REQUIRE(pl.detrend == ((flags & BHW_WELCH_DETREND_CONSTANT) != 0) && pl.power == ((flags & BHW_CFFT_POWER) != 0) &&
            pl.shifted == ((flags & BHW_CFFT_SHIFT) != 0), "flags 0x%x", flags);
    // the lanes, the rows and the passes of the real plan of 2n points
    bhw_stft r = s;
    r.channels = 1;
    r.n_fft = 2 * n;
    r.x_stride = r.y_stride = r.y_batch_stride = 0;
    const BhwStftFftPlan f = bhwp_stft_fft_plan(&p, 1, &r, 0, false);
    REQUIRE(f.m == pl.n && f.lpf == pl.lpf && f.fy == pl.fy && f.radix4 == pl.radix4 && f.radix2 == pl.radix2, "the real plan of %" PRIu64 " points", 2 * n);
}

// the group loop, the loads and the stores of every lane
static void replay_rows(const BhwStftCfftPlan &pl, const bhw_stft &s, uint64_t L)
{
    const uint64_t F = s.frames, B = s.batch, T = s.samples, n = s.n_fft;
    const uint64_t W = pl.power ? n : 2 * n, per = pl.power ? 1 : 2;
    std::vector<int> owned(pl.rows, 0), written(pl.rows * n, 0);
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
                for (uint32_t c = 0; c < pl.cpl; ++c) {
                    const uint32_t j = c * pl.lpf + l;
                    REQUIRE(j < n, "column %u", j);
                    if ((uint32_t)(j - (uint32_t)s.col0) >= L) continue;
                    uint64_t t = f * s.hop + j - s.pad;
                    if (t >= T) {
                        const int64_t ts = (int64_t)t;
                        if (s.pad_mode == BHW_PAD_REFLECT) t = ts < 0 ? (uint64_t)(-ts) : 2 * (T - 1) - t;
                        else t = 0;
                    }
                    REQUIRE(t < T && b * pl.x_stride + 2 * t + 2 <= xext, "frame %" PRIu64 " column %u reads sample %" PRIu64 " of %" PRIu64, f, j, t, T);
                }
                const uint32_t turn = pl.shifted ? (uint32_t)(n / 2) : 0u;
                for (uint64_t k = l; k < n; k += pl.lpf) {
                    const uint64_t col = (k + turn) & (n - 1);
                    REQUIRE(pl.shifted ? (col + n / 2) % n == k : col == k, "bin %" PRIu64 " goes to column %" PRIu64, k, col);
                    const uint64_t yi = b * pl.y_bstride + f * pl.y_stride + per * col;
                    REQUIRE(yi + per <= yext && per * col + per <= W && W <= pl.y_stride, "Y index %" PRIu64, yi);
                    ++written[r * n + col];
                }
            }
    for (uint64_t r = 0; r < pl.rows; ++r) REQUIRE(owned[r] == 1, "row %" PRIu64 " owned %d times", r, owned[r]);
    for (uint64_t i = 0; i < written.size(); ++i) REQUIRE(written[i] == 1, "column %" PRIu64 " written %d times", i, written[i]);
}

typedef std::complex<float> cf;
// the kernel's cmul, unfused
static cf cmulf(cf a, cf w) { return cf(a.real() * w.real() - a.imag() * w.imag(), a.real() * w.imag() + a.imag() * w.real()); }

// the passes of one row in float, with the kernel's indices and its twiddle table; returns the spectrum
static std::vector<cf> replay_passes(const BhwStftCfftPlan &pl, const std::vector<cf> &row)
{
    const uint32_t n = pl.n, H = n / 2, Q = n / 4;
    std::vector<cf> tw(H), a(row), b(n);
    for (uint32_t k = 0; k < H; ++k) tw[k] = cf((float)cos(2.0 * M_PI * k / n), (float)-sin(2.0 * M_PI * k / n));
    auto W = [&](uint32_t idx) {
        REQUIRE(idx < n, "twiddle index %u of %u", idx, n);
        const cf w = tw[idx & (H - 1)];
        return (idx & H) ? -w : w;
    };
    cf *src = a.data(), *dst = b.data();
    uint32_t Ns = 1;
    std::vector<int> hit(n);
    for (uint32_t p = 0; p < pl.radix4; ++p) {
        const uint32_t ts = n / (4 * Ns);
        std::fill(hit.begin(), hit.end(), 0);
        for (uint32_t l = 0; l < pl.lpf; ++l)
            for (uint32_t i = l; i < Q; i += pl.lpf) {
                const uint32_t k = i & (Ns - 1);
                REQUIRE(i + 3 * Q < n, "read %u", i + 3 * Q);
                cf a0 = src[i], a1 = src[i + Q], a2 = src[i + 2 * Q], a3 = src[i + 3 * Q];
                if (Ns > 1) {
                    a1 = cmulf(a1, W(k * ts));
                    a2 = cmulf(a2, W(2 * k * ts));
                    a3 = cmulf(a3, W(3 * k * ts));
                }
                const cf t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, t3 = cf(a1.imag() - a3.imag(), a3.real() - a1.real());
                const uint32_t o = ((i - k) << 2) + k;
                REQUIRE(o + 3 * Ns < n, "write %u", o + 3 * Ns);
                dst[o] = t0 + t2;
                dst[o + Ns] = t1 + t3;
                dst[o + 2 * Ns] = t0 - t2;
                dst[o + 3 * Ns] = t1 - t3;
                for (uint32_t q = 0; q < 4; ++q) ++hit[o + q * Ns];
            }
        for (uint32_t i = 0; i < n; ++i) REQUIRE(hit[i] == 1, "pass %u: point %u written %d times", p, i, hit[i]);
        std::swap(src, dst);
        Ns *= 4;
    }
    if (pl.radix2) {
        REQUIRE(Ns == H, "the radix-2 pass is the last: Ns %u", Ns);
        std::fill(hit.begin(), hit.end(), 0);
        for (uint32_t l = 0; l < pl.lpf; ++l)
            for (uint32_t i = l; i < H; i += pl.lpf) {
                const cf a0 = src[i], a1 = cmulf(src[i + H], tw[i]);
                dst[i] = a0 + a1;
                dst[i + H] = a0 - a1;
                ++hit[i];
                ++hit[i + H];
            }
        for (uint32_t i = 0; i < n; ++i) REQUIRE(hit[i] == 1, "radix-2 pass: point %u written %d times", i, hit[i]);
        std::swap(src, dst);
        Ns *= 2;
    }
    REQUIRE(Ns == n, "the passes end at Ns = n: %u", Ns);
    return std::vector<cf>(src, src + n);
}

// the two means of the kernel (one wave per row over the raw complex row in LDS) against the order of include/bhw.h, per channel
static void replay_mean_order()
{
    for (uint64_t L : {1ull, 2ull, 13ull, 63ull, 64ull, 65ull, 100ull, 400ull, 1000ull, 2048ull}) {
        std::vector<cf> x(L);
        for (int trial = 0; trial < 3; ++trial) {
            for (uint64_t j = 0; j < L; ++j) {
                const double u = uniform(), w = uniform();
                x[j] = cf((float)(trial == 1 ? 1e6 + u : trial == 2 ? u * 1e30 : u * 1000.0), (float)(trial == 1 ? w - 3e5 : trial == 2 ? w * 1e-20 : w * 10.0));
            }
            double P[2][64], Q[64], C[2][64];
            for (int ch = 0; ch < 2; ++ch)
                for (int i = 0; i < 64; ++i) P[ch][i] = C[ch][i] = 0.0;
            for (uint32_t lane = 0; lane < 64; ++lane)
                for (uint64_t j = lane; j < L; j += 64) {                                    // the kernel's lane loop: both accumulators
                    P[0][lane] += (double)x[j].real();
                    P[1][lane] += (double)x[j].imag();
                }
            for (int ch = 0; ch < 2; ++ch) {
                for (int s = 32; s >= 1; s >>= 1) {                                          // __shfl_down: lane i adds lane i + s (its own past 63)
                    memcpy(Q, P[ch], sizeof Q);
                    for (int i = 0; i < 64; ++i) P[ch][i] = Q[i] + Q[i + s < 64 ? i + s : i];
                }
                for (uint64_t j = 0; j < L; ++j) C[ch][j % 64] += (double)(ch ? x[j].imag() : x[j].real());   // the contract
                for (int s = 32; s >= 1; s >>= 1) {
                    memcpy(Q, C[ch], sizeof Q);
                    for (int i = 0; i < s; ++i) C[ch][i] = Q[i] + Q[i + s];
                }
                REQUIRE(memcmp(&P[ch][0], &C[ch][0], sizeof(double)) == 0, "L %" PRIu64 " trial %d channel %d: %a != %a", L, trial, ch, P[ch][0], C[ch][0]);
            }
        }
    }
}

int main()
{
    char buf[1000];
    long row_replays = 0, pass_replays = 0;
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 12, 24);
    replay_mean_order();
    const uint64_t xa = 0x10000000ull, ya = 0x100000000000ull;
    double worst_share = 0.0;
    for (uint32_t lg = kCfftMinLog; lg <= kCfftMaxLog; ++lg) {
        const uint64_t n = 1ull << lg;
        // the passes in float against a direct binary64 DFT of the float32 row: relative l2 error within 2^-24 * log2 n
        for (int trial = 0; trial < 3; ++trial) {
            bhw_stft s = desc_of(1, n, 1, 1, n, 0, 0, 0);
            const BhwStftCfftPlan pl = bhwp_stft_cfft_plan(&p, n, &s, 0, false);
            std::vector<cf> row(n);
            for (uint64_t j = 0; j < n; ++j)
                row[j] = cf((float)(uniform() * 1000.0 + (trial == 1 ? 250.0 : 0.0)), (float)(uniform() * 1000.0 + cos(0.7 * (double)j) * (trial == 2 ? 1e3 : 0.0)));
            const std::vector<cf> Y = replay_passes(pl, row);
            double ne = 0, nr = 0;
            std::vector<std::complex<double>> e(n);
            for (uint64_t j = 0; j < n; ++j) e[j] = std::polar(1.0, -2.0 * M_PI * (double)j / (double)n);
            for (uint64_t k = 0; k < n; ++k) {
                std::complex<double> d(0, 0);
                for (uint64_t j = 0; j < n; ++j) d += std::complex<double>(row[j].real(), row[j].imag()) * e[(j * k) % n];
                ne += std::norm(d - std::complex<double>(Y[k].real(), Y[k].imag()));
                nr += std::norm(d);
            }
            const double err = sqrt(ne / nr), cap = ldexp((double)lg, -24);
            REQUIRE(err <= cap, "n %" PRIu64 " trial %d: relative l2 error %.3e above the cap %.3e", n, trial, err, cap);
            if (err / cap > worst_share) worst_share = err / cap;
            ++pass_replays;
        }
        for (uint64_t L : {(uint64_t)1, (uint64_t)13, n / 2 + 1, n - 1, n})
            for (uint64_t hop : {(uint64_t)1, (uint64_t)7, n, n + 5})
                for (uint64_t B : {1ull, 3ull, 64ull})
                    for (uint64_t F : {1ull, 2ull, 63ull, 64ull, 65ull, 257ull, 2049ull})
                        for (int framing = 0; framing < 4; ++framing)           // 0 Welch + detrend, 1 Welch, 2 centred reflect, 3 centred constant
                            for (int padded = 0; padded <= 1; ++padded)
                                for (uint32_t form = 0; form < 4; ++form) {     // bit 0: power, bit 1: shifted bins
                                    const bool centred = framing >= 2;
                                    const uint64_t pad = centred ? n / 2 : 0, col0 = centred ? (n - L) / 2 : 0;
                                    const uint64_t reach = centred ? n : L;
                                    uint64_t T = (F - 1) * hop + reach;
                                    T = T > 2 * pad ? T - 2 * pad : 1;
                                    if (centred && T + 2 * pad < (F - 1) * hop + n) continue;       // fewer frames than asked: not this shape
                                    if (framing == 2 && pad > T - 1) continue;                      // reflect needs pad <= T - 1
                                    const uint32_t flags = (framing == 0 ? BHW_WELCH_DETREND_CONSTANT : 0u) | ((form & 1) ? BHW_CFFT_POWER : 0u) |
                                                           ((form & 2) ? BHW_CFFT_SHIFT : 0u);
                                    const bool power = (form & 1) != 0;
                                    const uint64_t W = power ? n : 2 * n;
                                    bhw_stft s = desc_of(B, T, F, hop, n, col0, pad, framing == 2 ? BHW_PAD_REFLECT : BHW_PAD_CONSTANT);
                                    if (padded) {
                                        s.x_stride = 2 * T + 3;                                     // odd: the 4-byte loads
                                        s.y_stride = W + (power ? 5 : 6);
                                        s.y_batch_stride = F * s.y_stride + (power ? 7 : 10);
                                    }
                                    int rc = bhwp_stft_cfft_checks(&p, L, &s, flags, nullptr, nullptr, false);
                                    REQUIRE(rc == BHW_OK, "checks rc %d: n %" PRIu64 " L %" PRIu64 " hop %" PRIu64 " B %" PRIu64 " F %" PRIu64 " framing %d form %u", rc, n, L, hop, B, F, framing, form);
                                    rc = bhwp_stft_cfft_checks(&p, L, &s, flags, (const void *)xa, (const void *)ya);
                                    REQUIRE(rc == BHW_OK, "pointer checks rc %d", rc);
                                    rc = bhwp_stft_cfft_checks(&p, L, &s, flags, (const void *)(xa + 4), (const void *)(ya + 4));
                                    REQUIRE(rc == (power ? BHW_OK : BHW_ERR_BADARG), "Y at 4 bytes: rc %d", rc);
                                    REQUIRE(bhwp_stft_cfft_checks(&p, L, &s, flags, (const void *)xa, (const void *)(ya + 2)) == BHW_ERR_BADARG, "misaligned Y");
                                    REQUIRE(bhwp_stft_cfft_checks(&p, L, &s, flags, (const void *)ya, (const void *)ya) == BHW_ERR_BADARG, "overlap");
                                    REQUIRE(bhwp_stft_cfft_checks(&p, L, &s, flags | 8u, nullptr, nullptr, false) == BHW_ERR_BADARG, "flags");
                                    const BhwStftCfftPlan pl = bhwp_stft_cfft_plan(&p, L, &s, flags, (B + F) % 2 == 0);
                                    plan_invariants(p, pl, s, flags);
                                    REQUIRE(bhwp_describe_stft_cfft(&p, nullptr, L, &s, flags, buf, sizeof buf) == BHW_OK && strlen(buf) > 40, "describe");
                                    if (B * F * n <= 40000 || (B == 1 && F == 2049 && n <= 512 && L == n && hop == 1 && (form == 0 || form == 3))) {
                                        replay_rows(pl, s, L);
                                        ++row_replays;
                                    }
                                    // one frame more than the signal holds; short and odd strides; one channel; frames 0
                                    bhw_stft bad = s;
                                    bad.frames = F + 1;
                                    if (!padded && (F * hop + reach > T + 2 * pad)) REQUIRE(bhwp_stft_cfft_checks(&p, L, &bad, flags, nullptr, nullptr, false) == BHW_ERR_BADARG, "extent");
                                    bad = s;
                                    bad.y_stride = W - 1;
                                    REQUIRE(bhwp_stft_cfft_checks(&p, L, &bad, flags, nullptr, nullptr, false) == BHW_ERR_BADARG, "short y_stride");
                                    bad.y_stride = W + 3;
                                    bad.y_batch_stride = 0;
                                    REQUIRE(bhwp_stft_cfft_checks(&p, L, &bad, flags, nullptr, nullptr, false) == (power ? BHW_OK : BHW_ERR_BADARG), "odd y_stride");
                                    bad = s;
                                    bad.channels = 1;
                                    bad.x_stride = 0;
                                    REQUIRE(bhwp_stft_cfft_checks(&p, L, &bad, flags, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED, "channels");
                                    bad = s;
                                    bad.frames = 0;
                                    REQUIRE(bhwp_stft_cfft_checks(&p, L, &bad, flags, nullptr, nullptr) == BHW_OK, "frames 0");
                                    REQUIRE(bhwp_describe_stft_cfft(&p, nullptr, L, &bad, flags, buf, sizeof buf) == BHW_OK, "describe frames 0");
                                }
    }
    // sizes the kernel does not have
    for (uint64_t n : {1ull, 2ull, 8ull, 15ull, 17ull, 48ull, 100ull, 1000ull, 2049ull, 4096ull, 8192ull, 1ull << 20, 1ull << 31}) {
        bhw_stft s = desc_of(1, 1ull << 33, 2, 1, n, 0, 0, 0);
        for (uint32_t flags = 0; flags < 8; ++flags)
            REQUIRE(bhwp_stft_cfft_checks(&p, 1, &s, flags, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED, "n_fft %" PRIu64, n);
    }
    // the element cap: batch * frames * n_fft above 2^34
    {
        bhw_stft s = desc_of(1ull << 20, 16 + 2047 * 16, 2048, 16, 16, 0, 0, 0);            // 2^31 rows x 16 columns = 2^35 > 2^34
        REQUIRE(bhwp_stft_cfft_checks(&p, 16, &s, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "cap");
    }
    REQUIRE(bhwp_stft_cfft_checks(&p, 16, nullptr, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "NULL descriptor");
    REQUIRE(row_replays > 2000 && pass_replays == 24, "replays %ld %ld", row_replays, pass_replays);
    printf("ok %ld checks, %ld row replays, %ld pass replays, worst error %.3f of the cap\n", g_checks, row_replays, pass_replays, worst_share);
    return 0;
}
