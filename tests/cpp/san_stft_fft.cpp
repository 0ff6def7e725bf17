// san_stft_fft.cpp -- the planner's part of the fused window + FFT calls (bhw_plan.cpp: bhwp_stft_fft_checks / bhwp_stft_fft_plan /
// bhwp_describe_stft_fft) swept under AddressSanitizer + UBSan over every supported n_fft against L, hop, batch and frames at the
// edges, padded and packed, centred and Welch framing.  Besides "no report" it asserts the plan's invariants -- LDS within 64 KiB,
// lanes x rows = the workgroup, lanes x columns = n_fft, the window staged inside the first buffer, grid within its bound -- and replays
// on the host the kernel's index arithmetic (bhw_stft_fft.hip):
//   - ownership: every row (b, f) of the pool is taken by exactly one (workgroup, trip of the group loop, slot);
//   - the loads: every window column of every row reads a sample inside its signal (the reflect map and the constant mode included);
//   - the mean: one wave per row, lane i over j = i, i + 64, ..., then the shuffle butterfly, against the order bhw.h writes down,
//     bit for bit on binary64 sums of float32 data;
//   - the passes: every butterfly reads and writes inside its row's M points, every point of the destination is written exactly once
//     per pass, every twiddle index is inside the table after folding, and the passes compose to the transform (against a direct
//     binary64 DFT at small sizes);
//   - the stores: every (b, f, k) of the spectrum written once, inside Y's extent, never in a gap.
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

static void plan_invariants(const BhwStftFftPlan &pl, const bhw_stft &s)
{
    const uint64_t n = s.n_fft;
    REQUIRE((1ull << pl.log2n) == n && pl.m == n / 2, "log2n %u m %u", pl.log2n, pl.m);
    REQUIRE(pl.lpf * pl.fy == kFftBlock && (uint64_t)pl.lpf * pl.cpl == n && pl.cpl <= kFftMaxCpl && pl.cpl >= 4, "lanes %u x %u, %u columns", pl.lpf, pl.fy, pl.cpl);
    REQUIRE(pl.lpf >= 4 && (pl.lpf >= pl.m / 4 || pl.lpf == kFftBlock), "lanes per row %u", pl.lpf);
    REQUIRE(2 * pl.radix4 + pl.radix2 == pl.log2n - 1 && pl.radix2 <= 1, "schedule %u x 4, %u x 2", pl.radix4, pl.radix2);
    REQUIRE(pl.lds_bytes == 2u * pl.fy * pl.m * 8u + pl.m * 8u + pl.fy * 4u && pl.lds_bytes <= 64u * 1024u, "LDS %u", pl.lds_bytes);
    REQUIRE(n * 4u <= (uint64_t)pl.fy * pl.m * 8u, "the staged window (%" PRIu64 " floats) inside the first buffer", n);
    REQUIRE(pl.rows == s.batch * s.frames && pl.groups == (pl.rows + pl.fy - 1) / pl.fy, "rows %" PRIu64 " groups %" PRIu64, pl.rows, pl.groups);
    REQUIRE(pl.grid >= 1 && pl.grid <= kFftMaxGrid && pl.grid <= pl.groups && (pl.grid == pl.groups || pl.grid == kFftMaxGrid), "grid %" PRIu64, pl.grid);
    REQUIRE(pl.y_stride >= n + 2 && pl.y_stride % 2 == 0 && pl.y_bstride % 2 == 0, "strides");
    char sched[48];
    bhwp_stft_fft_schedule(pl, sched, sizeof sched);
    REQUIRE(strlen(sched) == 2 * (pl.radix4 + pl.radix2) - 1, "schedule text %s", sched);
}

// the group loop, the loads and the stores of every lane
static void replay_rows(const BhwStftFftPlan &pl, const bhw_stft &s, uint64_t L)
{
    const uint64_t F = s.frames, B = s.batch, T = s.samples, K = s.n_fft / 2 + 1;
    std::vector<int> owned(pl.rows, 0), written(pl.rows * K, 0);
    const uint64_t yext = (B - 1) * pl.y_bstride + (F - 1) * pl.y_stride + 2 * K, xext = (B - 1) * pl.x_stride + T;
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
                    REQUIRE(j < s.n_fft, "column %u", j);
                    if ((uint32_t)(j - (uint32_t)s.col0) >= L) continue;
                    uint64_t t = f * s.hop + j - s.pad;
                    if (t >= T) {
                        const int64_t ts = (int64_t)t;
                        if (s.pad_mode == BHW_PAD_REFLECT) t = ts < 0 ? (uint64_t)(-ts) : 2 * (T - 1) - t;
                        else t = 0;
                    }
                    REQUIRE(t < T && b * pl.x_stride + t < xext, "frame %" PRIu64 " column %u reads sample %" PRIu64 " of %" PRIu64, f, j, t, T);
                }
                for (uint64_t k = l; k <= pl.m; k += pl.lpf) {
                    const uint64_t yi = b * pl.y_bstride + f * pl.y_stride + 2 * k;
                    REQUIRE(yi + 2 <= yext && 2 * k + 2 <= pl.y_stride, "Y index %" PRIu64, yi);
                    ++written[r * K + k];
                }
            }
    for (uint64_t r = 0; r < pl.rows; ++r) REQUIRE(owned[r] == 1, "row %" PRIu64 " owned %d times", r, owned[r]);
    for (uint64_t i = 0; i < written.size(); ++i) REQUIRE(written[i] == 1, "bin %" PRIu64 " written %d times", i, written[i]);
}

// the passes of one row in binary64, with the kernel's indices; returns the spectrum
static std::vector<std::complex<double>> replay_passes(const BhwStftFftPlan &pl, const std::vector<double> &row)
{
    typedef std::complex<double> cd;
    const uint32_t M = pl.m, n = 2 * M, Q = M / 4;
    std::vector<cd> tw(M), a(M), b(M);
    for (uint32_t k = 0; k < M; ++k) tw[k] = cd(cos(2.0 * M_PI * k / n), -sin(2.0 * M_PI * k / n));
    auto W = [&](uint32_t idx) {
        REQUIRE(idx < n, "twiddle index %u of %u", idx, n);
        const cd w = tw[idx & (M - 1)];
        return (idx & M) ? -w : w;
    };
    for (uint32_t i = 0; i < M; ++i) a[i] = cd(row[2 * i], row[2 * i + 1]);
    cd *src = a.data(), *dst = b.data();
    uint32_t Ns = 1;
    std::vector<int> hit(M);
    for (uint32_t p = 0; p < pl.radix4; ++p) {
        const uint32_t ts = M / (2 * Ns);
        std::fill(hit.begin(), hit.end(), 0);
        for (uint32_t l = 0; l < pl.lpf; ++l)
            for (uint32_t i = l; i < Q; i += pl.lpf) {
                const uint32_t k = i & (Ns - 1);
                REQUIRE(i + 3 * Q < M, "read %u", i + 3 * Q);
                cd a0 = src[i], a1 = src[i + Q], a2 = src[i + 2 * Q], a3 = src[i + 3 * Q];
                if (Ns > 1) {
                    a1 *= W(k * ts);
                    a2 *= W(2 * k * ts);
                    a3 *= W(3 * k * ts);
                }
                const cd t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, t3 = cd(0, -1) * (a1 - a3);
                const uint32_t o = ((i - k) << 2) + k;
                REQUIRE(o + 3 * Ns < M, "write %u", o + 3 * Ns);
                dst[o] = t0 + t2;
                dst[o + Ns] = t1 + t3;
                dst[o + 2 * Ns] = t0 - t2;
                dst[o + 3 * Ns] = t1 - t3;
                for (uint32_t q = 0; q < 4; ++q) ++hit[o + q * Ns];
            }
        for (uint32_t i = 0; i < M; ++i) REQUIRE(hit[i] == 1, "pass %u: point %u written %d times", p, i, hit[i]);
        std::swap(src, dst);
        Ns *= 4;
    }
    if (pl.radix2) {
        const uint32_t H = M / 2;
        REQUIRE(Ns == H, "the radix-2 pass is the last: Ns %u", Ns);
        std::fill(hit.begin(), hit.end(), 0);
        for (uint32_t l = 0; l < pl.lpf; ++l)
            for (uint32_t i = l; i < H; i += pl.lpf) {
                REQUIRE(2 * i < M, "twiddle %u", 2 * i);
                const cd a0 = src[i], a1 = src[i + H] * tw[2 * i];
                dst[i] = a0 + a1;
                dst[i + H] = a0 - a1;
                ++hit[i];
                ++hit[i + H];
            }
        for (uint32_t i = 0; i < M; ++i) REQUIRE(hit[i] == 1, "radix-2 pass: point %u written %d times", i, hit[i]);
        std::swap(src, dst);
        Ns *= 2;
    }
    REQUIRE(Ns == M, "the passes end at Ns = M: %u", Ns);
    std::vector<cd> Y(M + 1);
    for (uint32_t k = 0; k <= M; ++k) {
        if (k == 0 || k == M) {
            Y[k] = cd(k ? src[0].real() - src[0].imag() : src[0].real() + src[0].imag(), 0.0);
            continue;
        }
        const cd A = src[k], Bz = src[M - k];
        const cd E(0.5 * (A.real() + Bz.real()), 0.5 * (A.imag() - Bz.imag())), O(0.5 * (A.imag() + Bz.imag()), 0.5 * (Bz.real() - A.real()));
        Y[k] = E + O * tw[k];
    }
    return Y;
}

// the mean of the kernel (one wave per row over the raw row in LDS) against the order of include/bhw.h
static void replay_mean_order()
{
    for (uint64_t L : {1ull, 2ull, 13ull, 63ull, 64ull, 65ull, 100ull, 400ull, 1000ull, 4096ull}) {
        std::vector<float> x(L);
        for (int trial = 0; trial < 3; ++trial) {
            for (uint64_t j = 0; j < L; ++j) {
                const double u = (double)(rnd() >> 11) / 9007199254740992.0 - 0.5;
                x[j] = (float)(trial == 1 ? 1e6 + u : trial == 2 ? u * 1e30 : u * 1000.0);
            }
            double P[64], Q[64], C[64];
            for (int i = 0; i < 64; ++i) P[i] = C[i] = 0.0;
            for (uint32_t lane = 0; lane < 64; ++lane)
                for (uint64_t j = lane; j < L; j += 64) P[lane] += (double)x[j];             // the kernel's lane loop
            for (int s = 32; s >= 1; s >>= 1) {                                              // __shfl_down: lane i adds lane i + s (its own past 63)
                memcpy(Q, P, sizeof Q);
                for (int i = 0; i < 64; ++i) P[i] = Q[i] + Q[i + s < 64 ? i + s : i];
            }
            for (uint64_t j = 0; j < L; ++j) C[j % 64] += (double)x[j];                      // the contract
            for (int s = 32; s >= 1; s >>= 1) {
                memcpy(Q, C, sizeof Q);
                for (int i = 0; i < s; ++i) C[i] = Q[i] + Q[i + s];
            }
            REQUIRE(memcmp(&P[0], &C[0], sizeof(double)) == 0, "L %" PRIu64 " trial %d: %a != %a", L, trial, P[0], C[0]);
        }
    }
}

int main()
{
    char buf[900];
    long row_replays = 0, pass_replays = 0;
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 12, 24);
    replay_mean_order();
    const uint64_t xa = 0x10000000ull, ya = 0x100000000000ull;
    for (uint32_t lg = kFftMinLog; lg <= kFftMaxLog; ++lg) {
        const uint64_t n = 1ull << lg;
        // the passes compose to the transform: against a direct DFT where that is cheap, every size against Parseval and bin 0
        {
            bhw_stft s = desc_of(1, n, 1, 1, n, 0, 0, 0);
            const BhwStftFftPlan pl = bhwp_stft_fft_plan(&p, n, &s, 0, false);
            std::vector<double> row(n);
            double sum = 0, energy = 0;
            for (uint64_t j = 0; j < n; ++j) {
                row[j] = (double)(rnd() >> 11) / 9007199254740992.0 - 0.5;
                sum += row[j];
                energy += row[j] * row[j];
            }
            const std::vector<std::complex<double>> Y = replay_passes(pl, row);
            double spec = 0;
            for (uint64_t k = 0; k <= n / 2; ++k) spec += std::norm(Y[k]) * ((k == 0 || k == n / 2) ? 1.0 : 2.0);
            REQUIRE(fabs(Y[0].real() - sum) < 1e-9 && fabs(spec / (double)n - energy) < 1e-9 * energy, "n %" PRIu64 ": bin 0 / Parseval", n);
            if (n <= 512)
                for (uint64_t k = 0; k <= n / 2; ++k) {
                    std::complex<double> d(0, 0);
                    for (uint64_t j = 0; j < n; ++j) d += row[j] * std::polar(1.0, -2.0 * M_PI * (double)((j * k) % n) / (double)n);
                    REQUIRE(std::abs(d - Y[k]) < 1e-9, "n %" PRIu64 " bin %" PRIu64, n, k);
                }
            ++pass_replays;
        }
        for (uint64_t L : {(uint64_t)1, (uint64_t)13, n / 2 + 1, n - 1, n})
            for (uint64_t hop : {(uint64_t)1, (uint64_t)7, n, n + 5})
                for (uint64_t B : {1ull, 3ull, 64ull})
                    for (uint64_t F : {1ull, 2ull, 63ull, 64ull, 65ull, 257ull, 2049ull})
                        for (int framing = 0; framing < 4; ++framing)           // 0 Welch + detrend, 1 Welch, 2 centred reflect, 3 centred constant
                            for (int padded = 0; padded <= 1; ++padded) {
                                if (L > 4096) continue;
                                const bool centred = framing >= 2;
                                const uint64_t pad = centred ? n / 2 : 0, col0 = centred ? (n - L) / 2 : 0;
                                const uint64_t reach = centred ? n : L;
                                uint64_t T = (F - 1) * hop + reach;
                                T = T > 2 * pad ? T - 2 * pad : 1;
                                if (centred && T + 2 * pad < (F - 1) * hop + n) continue;       // fewer frames than asked: not this shape
                                if (framing == 2 && pad > T - 1) continue;                      // reflect needs pad <= T - 1
                                const uint32_t flags = framing == 0 ? BHW_WELCH_DETREND_CONSTANT : 0u;
                                bhw_stft s = desc_of(B, T, F, hop, n, col0, pad, framing == 2 ? BHW_PAD_REFLECT : BHW_PAD_CONSTANT);
                                if (padded) {
                                    s.x_stride = T + 3;
                                    s.y_stride = n + 2 + 6;
                                    s.y_batch_stride = F * s.y_stride + 10;
                                }
                                int rc = bhwp_stft_fft_checks(&p, L, &s, flags, nullptr, nullptr, false);
                                REQUIRE(rc == BHW_OK, "checks rc %d: n %" PRIu64 " L %" PRIu64 " hop %" PRIu64 " B %" PRIu64 " F %" PRIu64 " framing %d", rc, n, L, hop, B, F, framing);
                                rc = bhwp_stft_fft_checks(&p, L, &s, flags, (const void *)xa, (const void *)ya);
                                REQUIRE(rc == BHW_OK, "pointer checks rc %d", rc);
                                REQUIRE(bhwp_stft_fft_checks(&p, L, &s, flags, (const void *)xa, (const void *)(ya + 4)) == BHW_ERR_BADARG, "misaligned Y");
                                REQUIRE(bhwp_stft_fft_checks(&p, L, &s, flags, (const void *)ya, (const void *)ya) == BHW_ERR_BADARG, "overlap");
                                REQUIRE(bhwp_stft_fft_checks(&p, L, &s, flags | 2u, nullptr, nullptr, false) == BHW_ERR_BADARG, "flags");
                                const BhwStftFftPlan pl = bhwp_stft_fft_plan(&p, L, &s, flags, (B + F) % 2 == 0);
                                plan_invariants(pl, s);
                                REQUIRE(pl.detrend == (flags != 0), "detrend");
                                REQUIRE(bhwp_describe_stft_fft(&p, nullptr, L, &s, flags, buf, sizeof buf) == BHW_OK && strlen(buf) > 40, "describe");
                                if (B * F * n <= 600000 || (B == 1 && F == 2049 && n <= 1024 && L == n && hop == 1)) {
                                    replay_rows(pl, s, L);
                                    ++row_replays;
                                }
                                // one frame more than the signal holds; odd and short strides; another channel count
                                bhw_stft bad = s;
                                bad.frames = F + 1;
                                if (!padded && (F * hop + reach > T + 2 * pad)) REQUIRE(bhwp_stft_fft_checks(&p, L, &bad, flags, nullptr, nullptr, false) == BHW_ERR_BADARG, "extent");
                                bad = s;
                                bad.y_stride = n + 1;
                                REQUIRE(bhwp_stft_fft_checks(&p, L, &bad, flags, nullptr, nullptr, false) == BHW_ERR_BADARG, "short y_stride");
                                bad.y_stride = n + 3;
                                REQUIRE(bhwp_stft_fft_checks(&p, L, &bad, flags, nullptr, nullptr, false) == BHW_ERR_BADARG, "odd y_stride");
                                bad = s;
                                bad.channels = 2;
                                bad.x_stride = 0;
                                REQUIRE(bhwp_stft_fft_checks(&p, L, &bad, flags, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED, "channels");
                                bad = s;
                                bad.frames = 0;
                                REQUIRE(bhwp_stft_fft_checks(&p, L, &bad, flags, nullptr, nullptr) == BHW_OK, "frames 0");
                                REQUIRE(bhwp_describe_stft_fft(&p, nullptr, L, &bad, flags, buf, sizeof buf) == BHW_OK, "describe frames 0");
                            }
    }
    // sizes the kernel does not have
    for (uint64_t n : {1ull, 2ull, 8ull, 15ull, 17ull, 48ull, 100ull, 1000ull, 4097ull, 8192ull, 1ull << 20, 1ull << 31}) {
        bhw_stft s = desc_of(1, 1ull << 33, 2, 1, n, 0, 0, 0);
        REQUIRE(bhwp_stft_fft_checks(&p, 1, &s, 0, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED, "n_fft %" PRIu64, n);
    }
    // the element cap: batch * frames * K above 2^34 (n_fft 16: K = 9)
    {
        bhw_stft s = desc_of(1ull << 20, 16 + 2047 * 16, 2048, 16, 16, 0, 0, 0);            // 2^31 rows x 16 columns = 2^35 > 2^34
        REQUIRE(bhwp_stft_fft_checks(&p, 16, &s, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "cap");
    }
    REQUIRE(bhwp_stft_fft_checks(&p, 16, nullptr, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "NULL descriptor");
    REQUIRE(row_replays > 2000 && pass_replays == 9, "replays %ld %ld", row_replays, pass_replays);
    printf("ok %ld checks, %ld row replays, %ld pass replays\n", g_checks, row_replays, pass_replays);
    return 0;
}
