// san_welch.cpp -- the planner's part of Welch's method around the FFT (bhw_plan.cpp: bhwp_sums_checks / bhwp_sums_plan,
// bhwp_welch_checks / bhwp_welch_plan, bhwp_psd_checks / bhwp_psd_plan, bhwp_describe_welch) swept under AddressSanitizer + UBSan over
// batch, T, L, nfft, hop and channels, with the frame count at 1, BLOCK - 1, BLOCK, BLOCK + 1 and many.  Besides "no report", it replays
// on the host
//   - the mean order: k_welch_mean's lane loop and shuffle butterfly (bhw_welch.h) against the order bhw.h writes down, bit for bit on
//     binary64 sums of float32 data, and every x index inside its signal;
//   - the lane and row ownership of the segments kernel (welch_loop): every (b, f, j) written exactly once, the window columns read
//     the sample f * hop + j < T and the mean of their own row;
//   - the block cut of the periodogram (k_welch_psd / k_welch_psd_join): the passes of four waves through LDS, every (b, f, k) added once,
//     in ascending f inside its block, every load (clamped past the block's end, idle lanes at the last bin) inside Y,
//     the block sums at distinct workspace slots inside the workspace, joined in ascending block order;
//   - the lanes of the window sums (every k < L once) and the join of the split sum-of-squares counters, at its bound L = 2^30,
//     |u| = 2^31.
#include <cinttypes>
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

static bhw_stft seg_of(uint64_t B, uint64_t T, uint64_t frames, uint64_t hop, uint64_t n_fft, uint32_t C)
{
    bhw_stft s;
    memset(&s, 0, sizeof s);
    s.struct_size = sizeof s;
    s.channels = C;
    s.batch = B;
    s.samples = T;
    s.frames = frames;
    s.hop = hop;
    s.n_fft = n_fft;
    s.shift = 15;
    return s;
}

// the order of include/bhw.h: 64 partial sums over j = i (mod 64) in ascending j, then the butterfly s = 32 .. 1 on a snapshot
static double mean_sum_contract(const float *x, uint64_t L)
{
    double P[64];
    for (int i = 0; i < 64; ++i) P[i] = 0.0;
    for (uint64_t j = 0; j < L; ++j) P[j % 64] += (double)x[j];
    for (int s = 32; s >= 1; s >>= 1) {
        double Q[64];
        memcpy(Q, P, sizeof Q);
        for (int i = 0; i < s; ++i) P[i] = Q[i] + Q[i + s];
    }
    return P[0];
}

// welch_mean_rows: lane i walks j = i, i + 64 * U, ... with U loads in flight added in order; then the wave's __shfl_down butterfly,
// in which every lane adds the value of lane i + s (its own when i + s >= 64)
static double mean_sum_kernel(const float *x, uint64_t L, std::vector<int> &seen)
{
    const uint32_t U = 4;
    double P[64];
    for (uint32_t lane = 0; lane < 64; ++lane) {
        P[lane] = 0.0;
        for (uint64_t j = lane; j < L; j += 64u * U)
            for (uint32_t u = 0; u < U; ++u)
                if (j + 64u * u < L) {
                    P[lane] += (double)x[j + 64u * u];
                    ++seen[j + 64u * u];
                }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        double Q[64];
        memcpy(Q, P, sizeof Q);
        for (int i = 0; i < 64; ++i) P[i] = Q[i] + Q[i + s < 64 ? i + s : i];
    }
    return P[0];
}

static void replay_mean_order()
{
    for (uint64_t L : {1ull, 2ull, 63ull, 64ull, 65ull, 127ull, 128ull, 255ull, 256ull, 257ull, 400ull, 1000ull, 4096ull, 5003ull}) {
        std::vector<float> x(L);
        for (int trial = 0; trial < 4; ++trial) {
            for (uint64_t j = 0; j < L; ++j) {
                const double u = (double)(rnd() >> 11) / 9007199254740992.0 - 0.5;
                x[j] = (float)(trial == 1 ? 1e6 + u : trial == 2 ? u * 1e30 : u * 1000.0);
            }
            if (trial == 3) x[L / 2] = 1e-40f;
            std::vector<int> seen(L, 0);
            const double a = mean_sum_contract(x.data(), L), b = mean_sum_kernel(x.data(), L, seen);
            REQUIRE(memcmp(&a, &b, sizeof a) == 0, "L %" PRIu64 " trial %d: %a != %a", L, trial, a, b);
            for (uint64_t j = 0; j < L; ++j) REQUIRE(seen[j] == 1, "L %" PRIu64 ": sample %" PRIu64 " added %d times", L, j, seen[j]);
        }
    }
}

// the mean pass: the rows of the grid-stride loop, one wave each, and the x range a row reads
static void replay_mean_rows(const BhwWelchPlan &wp, const bhw_stft &s, uint64_t L)
{
    const BhwStftPlan &pl = wp.frames;
    const uint64_t per_wg = kWelchMeanBlock / 64u, C = s.channels, F = s.frames;
    std::vector<int> rows(pl.rows, 0);
    REQUIRE(wp.mean_grid >= 1 && wp.mean_grid <= kWelchMeanMaxGrid, "mean grid %" PRIu64, wp.mean_grid);
    for (uint64_t wg = 0; wg < wp.mean_grid; ++wg)
        for (uint64_t wave = 0; wave < per_wg; ++wave)
            for (uint64_t r = wg * per_wg + wave; r < pl.rows; r += wp.mean_grid * per_wg) {
                const uint64_t b = r / F, f = r - b * F;
                REQUIRE(b < s.batch, "row %" PRIu64, r);
                const uint64_t lo = b * pl.x_stride + f * s.hop * C, hi = lo + L * C;           // elements [lo, hi)
                REQUIRE(lo >= b * pl.x_stride && hi <= b * pl.x_stride + s.samples * C, "row %" PRIu64 " reads [%" PRIu64 ", %" PRIu64 ")", r, lo, hi);
                REQUIRE((r * C + C) * 4u <= wp.ws_bytes, "mean slot of row %" PRIu64, r);
                ++rows[r];
            }
    for (uint64_t r = 0; r < pl.rows; ++r) REQUIRE(rows[r] == 1, "row %" PRIu64 " averaged %d times", r, rows[r]);
}

// welch_loop: every lane of the grid, every row of its row blocks, in the kernel's order
static void replay_segments(const BhwWelchPlan &wp, const bhw_stft &s, uint64_t L)
{
    const BhwStftPlan &pl = wp.frames;
    const uint64_t F = s.frames, B = s.batch, N = s.n_fft, C = s.channels;
    std::vector<int> writes(B * F * N, 0);
    const uint64_t span = pl.group * pl.fy;
    for (uint64_t bx = 0; bx < pl.grid_x; ++bx)
        for (uint64_t gy = 0; gy < pl.grid_y; ++gy)
            for (uint32_t tid = 0; tid < kFramesBlock; ++tid) {
                const uint64_t j = bx * pl.kx + (tid & (pl.kx - 1u));
                const uint32_t ty = tid / pl.kx;
                if (j >= N) continue;
                const bool in = j < L;
                for (uint64_t by = gy; by < pl.row_blocks; by += pl.grid_y) {
                    const uint64_t r_beg = by * span + ty, r_end = (by + 1) * span < pl.rows ? (by + 1) * span : pl.rows;
                    if (r_beg >= r_end) continue;
                    uint64_t b = r_beg / F, f = r_beg - b * F;
                    for (uint64_t r = r_beg; r < r_end; r += pl.fy) {
                        REQUIRE(b * F + f == r && f < F && b < B, "row %" PRIu64 " -> (%" PRIu64 ", %" PRIu64 ")", r, b, f);   // the mean at r * C + c is this row's
                        ++writes[(b * F + f) * N + j];
                        if (in) {
                            const uint64_t t = f * s.hop + j;
                            REQUIRE(t < s.samples, "segment %" PRIu64 " column %" PRIu64 " reads sample %" PRIu64, f, j, t);
                            REQUIRE(b * pl.x_stride + t * C + C <= (B - 1) * pl.x_stride + s.samples * C, "x index");
                        }
                        const uint64_t yi = b * pl.y_bstride + f * pl.y_stride + j * C;
                        REQUIRE(yi + C <= (B - 1) * pl.y_bstride + (F - 1) * pl.y_stride + N * C, "y index %" PRIu64, yi);
                        f += pl.step_f;                             // welch_step
                        b += pl.step_b;
                        if (f >= F) {
                            f -= F;
                            ++b;
                        }
                    }
                }
            }
    for (uint64_t i = 0; i < writes.size(); ++i) REQUIRE(writes[i] == 1, "element %" PRIu64 " written %d times", i, writes[i]);
}

static bhw_psd psd_of(uint64_t B, uint64_t F, uint64_t K, uint64_t n_fft, uint32_t flags, uint64_t ys, uint64_t ybs, uint64_t ps)
{
    bhw_psd d;
    memset(&d, 0, sizeof d);
    d.struct_size = sizeof d;
    d.flags = flags;
    d.batch = B;
    d.frames = F;
    d.bins = K;
    d.n_fft = n_fft;
    d.y_stride = ys;
    d.y_batch_stride = ybs;
    d.p_stride = ps;
    d.scale = 0.25;
    return d;
}

// k_welch_psd over its grid, then k_welch_psd_join
static void replay_psd(const BhwPsdPlan &pl, const bhw_psd &d)
{
    const uint64_t B = d.batch, F = d.frames, K = d.bins;
    std::vector<int> reads(B * F * K, 0), slots(B * pl.blocks * K, 0), outs(B * K, 0);
    REQUIRE(pl.blocks == (F + BHW_WELCH_BLOCK - 1) / BHW_WELCH_BLOCK && pl.grid == B * pl.blocks * pl.tiles, "plan");
    REQUIRE((pl.blocks == 1) == (pl.ws_bytes == 0) && (pl.blocks == 1 || pl.ws_bytes == B * pl.blocks * K * 8), "workspace %" PRIu64, pl.ws_bytes);
    const uint64_t yext = (B - 1) * pl.y_bstride + (F - 1) * pl.y_stride + K;
    for (uint64_t unit = 0; unit < pl.grid; ++unit)
        for (uint32_t lane = 0; lane < kPsdLanes; ++lane) {
            const uint64_t tile = unit % pl.tiles, rest = unit / pl.tiles, blk = rest % pl.blocks, b = rest / pl.blocks;
            const uint64_t k = tile * kPsdLanes + lane;
            const bool active = k < K;
            const uint64_t kk = active ? k : K - 1;                                     // an idle lane loads the last bin
            REQUIRE(b < B, "unit %" PRIu64, unit);
            const uint64_t f0 = blk * BHW_WELCH_BLOCK, f1 = f0 + BHW_WELCH_BLOCK < F ? f0 + BHW_WELCH_BLOCK : F;
            REQUIRE(f0 < f1 && f1 - f0 <= BHW_WELCH_BLOCK, "block %" PRIu64, blk);
            int64_t last = -1;
            const uint32_t U = pl.unroll, pass = kPsdWaves * U;
            REQUIRE((U == kPsdUnrollMax || U == kPsdUnrollMin) && (U == kPsdUnrollMax) == (pl.grid <= kPsdSmallGrid), "unroll %u", U);
            for (uint64_t p0 = f0; p0 < f1; p0 += pass) {
                // the loads of the pass: wave w, slot u -> LDS row w * U + u holds frame p0 + row (clamped past the end)
                uint64_t row_frame[kPsdWaves * kPsdUnrollMax];
                for (uint32_t wave = 0; wave < kPsdWaves; ++wave)
                    for (uint32_t u = 0; u < U; ++u) {
                        const uint64_t fr = p0 + wave * U + u, frc = fr < f1 ? fr : f1 - 1;
                        const uint64_t yi = b * pl.y_bstride + frc * pl.y_stride + kk;
                        REQUIRE(yi < yext, "Y index %" PRIu64, yi);
                        row_frame[wave * U + u] = fr;
                    }
                // wave 0 adds rows 0 .. n - 1 in ascending order
                const uint32_t n = f1 - p0 < pass ? (uint32_t)(f1 - p0) : pass;
                for (uint32_t i = 0; i < n; ++i) {
                    const uint64_t f = row_frame[i];
                    REQUIRE(f == p0 + i && f < f1 && (int64_t)f > last, "frame order: row %u holds %" PRIu64, i, f);
                    last = (int64_t)f;
                    if (active) ++reads[(b * F + f) * K + k];
                }
            }
            if (!active) continue;
            if (pl.blocks > 1) {
                const uint64_t wi = (b * pl.blocks + blk) * K + k;
                REQUIRE((wi + 1) * 8 <= pl.ws_bytes, "workspace slot %" PRIu64, wi);
                ++slots[wi];
            } else {
                REQUIRE(b * pl.p_stride + k < (B - 1) * pl.p_stride + K, "P index");
                ++outs[b * K + k];
            }
        }
    if (pl.blocks > 1) {
        REQUIRE(pl.join_grid * 256u >= B * K && (pl.join_grid - 1) * 256u < B * K, "join grid");
        for (uint64_t i = 0; i < pl.join_grid * 256u; ++i) {
            if (i >= B * K) continue;
            const uint64_t b = i / K, k = i - b * K;
            uint64_t prev = 0;
            for (uint64_t blk = 0; blk < pl.blocks; ++blk) {
                const uint64_t wi = b * pl.blocks * K + k + blk * K;
                REQUIRE(wi == (b * pl.blocks + blk) * K + k && (blk == 0 || wi > prev) && slots[wi] == 1, "join slot %" PRIu64, wi);
                prev = wi;
            }
            ++outs[b * K + k];
        }
    }
    for (uint64_t i = 0; i < reads.size(); ++i) REQUIRE(reads[i] == 1, "Y element %" PRIu64 " read %d times", i, reads[i]);
    for (uint64_t i = 0; i < outs.size(); ++i) REQUIRE(outs[i] == 1, "P element %" PRIu64 " written %d times", i, outs[i]);
}

static void sums_section(const bhw_params &p)
{
    char buf[640];
    // the lanes of the reduction: every k < L exactly once, the same trip count in every lane
    for (uint64_t L : {1ull, 2ull, 63ull, 64ull, 65ull, 400ull, 2047ull, 2048ull, 2049ull, 4096ull, 65537ull, 1ull << 20, (1ull << 20) + 1}) {
        const BhwSumsPlan pl = bhwp_sums_plan(L);
        REQUIRE(pl.grid >= 1 && pl.grid <= kSumsMaxGrid && pl.trips >= 1, "L %" PRIu64, L);
        const uint64_t lanes = (uint64_t)pl.grid * kSumsBlock;
        REQUIRE(lanes * pl.trips >= L && lanes * (pl.trips - 1) < L, "L %" PRIu64 ": %" PRIu64 " lanes x %u", L, lanes, pl.trips);
        std::vector<uint8_t> seen(L, 0);
        for (uint64_t g = 0; g < lanes; ++g)
            for (uint32_t n = 0; n < pl.trips; ++n) {
                const uint64_t k = g + (uint64_t)n * lanes;
                if (k < L) ++seen[k];
            }
        for (uint64_t k = 0; k < L; ++k) REQUIRE(seen[k] == 1, "coefficient %" PRIu64, k);
    }
    for (uint32_t pw = 4; pw <= 30; ++pw) {
        const BhwSumsPlan pl = bhwp_sums_plan(1ull << pw);
        REQUIRE((uint64_t)pl.grid * kSumsBlock * pl.trips >= (1ull << pw), "2^%u", pw);
    }
    REQUIRE(bhwp_sums_checks(&p, 400, 0, (const void *)0x1000) == BHW_OK && bhwp_sums_checks(&p, 400, BHW_SUMS_F32, (const void *)0x1000) == BHW_OK, "checks");
    REQUIRE(bhwp_sums_checks(&p, 400, 2, (const void *)0x1000) == BHW_ERR_BADARG && bhwp_sums_checks(&p, 400, 0, (const void *)0x1004) == BHW_ERR_BADARG, "checks");
    REQUIRE(bhwp_sums_checks(&p, 0, 0, (const void *)0x1000) == BHW_ERR_BADARG && bhwp_sums_checks(&p, 400, 0, nullptr) == BHW_ERR_BADARG, "checks");
    REQUIRE(bhwp_describe_welch(&p, nullptr, 400, nullptr, BHW_SUMS_F32, nullptr, buf, sizeof buf) == BHW_OK, "describe");
    // the split counters: per coefficient the low and the high 32 bits of u^2, joined as lo + hi * 2^32
    for (int trial = 0; trial < 2000; ++trial) {
        unsigned __int128 want = 0;
        uint64_t lo = 0, hi = 0;
        int64_t s1 = 0;
        const int n = 1 + (int)(rnd() % 64);
        for (int i = 0; i < n; ++i) {
            int64_t u = (int64_t)(rnd() % ((1ull << 32) + 1)) - (1ll << 31);           // -2^31 .. 2^31, both ends included
            if (i == 0 && trial % 7 == 0) u = 1ll << 31;
            if (i == 1 && trial % 5 == 0) u = -(1ll << 31);
            const uint64_t q = (uint64_t)(u * u);
            REQUIRE(q <= (1ull << 62), "u^2");
            lo += q & 0xFFFFFFFFull;
            hi += q >> 32;
            s1 += u;
            want += (unsigned __int128)q;
        }
        REQUIRE(bhwp_sums_join(lo, hi) == want, "join, trial %d", trial);
    }
    // the bound: L = 2^30 coefficients of |u| = 2^31.  lo = 0, hi = 2^30 * 2^30 = 2^60 < 2^62; s2 = 2^92; s1 = -2^61 in two's complement
    const uint64_t L = 1ull << 30, q = 1ull << 62;
    const uint64_t lo = L * (q & 0xFFFFFFFFull), hi = L * (q >> 32);
    REQUIRE(lo == 0 && hi == (1ull << 60), "bound counters");
    REQUIRE(bhwp_sums_join(lo, hi) == ((unsigned __int128)1 << 92), "bound join");
    const uint64_t lo_max = L * 0xFFFFFFFFull;                                          // the low counter's own bound: below 2^62
    REQUIRE(lo_max < (1ull << 62) && bhwp_sums_join(lo_max, hi) == ((unsigned __int128)1 << 92) + lo_max, "low counter bound");
    const uint64_t s1w = (uint64_t)0 - (L << 31);                                       // wrapping adds of -2^31
    REQUIRE((int64_t)s1w == -(1ll << 61), "s1 bound");
}

int main()
{
    char buf[900];
    long seg_replays = 0, psd_replays = 0;
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 12, 24);
    replay_mean_order();
    sums_section(p);
    const unsigned long long BL = BHW_WELCH_BLOCK;
    REQUIRE(BL == 256, "BHW_WELCH_BLOCK %llu", BL);
    // the segments: batch, L, nfft, hop, channels, and T chosen for F = 1, BLOCK - 1, BLOCK, BLOCK + 1 and many
    for (uint64_t B : {1ull, 3ull, 64ull})
        for (uint64_t L : {1ull, 13ull, 64ull, 100ull, 400ull})
            for (uint64_t extra : {0ull, 1ull, 112ull})                                  // nfft - L
                for (uint64_t hop : {1ull, 5ull, 100ull, 450ull})
                    for (uint64_t F : {1ull, BL - 1, BL, BL + 1, 3 * BL + 7})
                        for (uint32_t C = 1; C <= 2; ++C)
                            for (uint64_t slack : {0ull, 3ull}) {
                                const uint64_t n_fft = L + extra;
                                const uint64_t T = (F - 1) * hop + L + (slack < hop ? slack : hop - 1);   // scipy's count stays F
                                REQUIRE(1 + (T - L) / hop == F, "frame count");
                                bhw_stft s = seg_of(B, T, F, hop, n_fft, C);
                                for (uint32_t flags = 0; flags <= 1; ++flags) {
                                    int rc = bhwp_welch_checks(&p, L, &s, flags, nullptr, nullptr, nullptr, 0, false);
                                    REQUIRE(rc == BHW_OK, "checks rc %d: B %" PRIu64 " T %" PRIu64 " L %" PRIu64 " n_fft %" PRIu64, rc, B, T, L, n_fft);
                                    const uint64_t need = bhwp_welch_workspace_bytes(&s, flags);
                                    REQUIRE(need == (flags ? B * F * C * 4 : 0), "workspace %" PRIu64, need);
                                    // with pointers: far apart passes; a workspace one byte short or at y does not
                                    const uint64_t xa = 0x10000000ull, ya = 0x100000000000ull, wa = 0x200000000000ull;
                                    rc = bhwp_welch_checks(&p, L, &s, flags, (const void *)xa, (const void *)ya, (const void *)wa, need);
                                    REQUIRE(rc == BHW_OK, "pointer checks rc %d", rc);
                                    if (flags) {
                                        REQUIRE(bhwp_welch_checks(&p, L, &s, flags, (const void *)xa, (const void *)ya, (const void *)wa, need - 1) == BHW_ERR_WORKSPACE, "short");
                                        REQUIRE(bhwp_welch_checks(&p, L, &s, flags, (const void *)xa, (const void *)ya, (const void *)ya, need) == BHW_ERR_BADARG, "overlap");
                                        REQUIRE(bhwp_welch_checks(&p, L, &s, flags, (const void *)xa, (const void *)ya, nullptr, need) == BHW_ERR_BADARG, "NULL");
                                    }
                                    REQUIRE(bhwp_describe_welch(&p, nullptr, L, &s, flags, nullptr, buf, sizeof buf) == BHW_OK, "describe");
                                    const BhwWelchPlan wp = bhwp_welch_plan(&p, L, &s, flags, (B + F) % 2 == 0);
                                    REQUIRE(wp.detrend == (flags != 0) && wp.ws_bytes == need && wp.frames.rows == B * F, "plan");
                                    if (flags && B * F * n_fft <= 300000) {
                                        replay_mean_rows(wp, s, L);
                                        replay_segments(wp, s, L);
                                        ++seg_replays;
                                    }
                                }
                                // one segment more than the signal holds, padding, an offset window: refused
                                bhw_stft bad = seg_of(B, T, F + 1, hop, n_fft, C);
                                if (T < F * hop + L) REQUIRE(bhwp_welch_checks(&p, L, &bad, 1, nullptr, nullptr, nullptr, 0, false) == BHW_ERR_BADARG, "extent");
                                bad = s;
                                bad.pad = 1;
                                REQUIRE(bhwp_welch_checks(&p, L, &bad, 0, nullptr, nullptr, nullptr, 0, false) == BHW_ERR_BADARG, "pad");
                                bad = s;
                                bad.pad_mode = 1;
                                REQUIRE(bhwp_welch_checks(&p, L, &bad, 0, nullptr, nullptr, nullptr, 0, false) == BHW_ERR_BADARG, "pad_mode");
                                if (extra) {
                                    bad = s;
                                    bad.col0 = 1;
                                    REQUIRE(bhwp_welch_checks(&p, L, &bad, 1, nullptr, nullptr, nullptr, 0, false) == BHW_ERR_BADARG, "col0");
                                }
                                REQUIRE(bhwp_welch_checks(&p, L, &s, 2, nullptr, nullptr, nullptr, 0, false) == BHW_ERR_BADARG, "flags");
                            }
    // the periodogram: F around the block size, K around the lane count, packed and strided
    for (uint64_t B : {1ull, 3ull, 64ull})
        for (uint64_t F : {1ull, 2ull, BL - 1, BL, BL + 1, 3 * BL + 7})
            for (uint64_t n_fft : {1ull, 64ull, 65ull, 512ull, 1024ull})
                for (uint32_t flags = 0; flags <= 1; ++flags)
                    for (int strided = 0; strided <= 1; ++strided) {
                        const uint64_t K = flags ? n_fft / 2 + 1 : n_fft;
                        const uint64_t ys = strided ? K + 3 : 0, ybs = strided ? (F - 1) * (K + 3) + K + 5 : 0, ps = strided ? K + 2 : 0;
                        bhw_psd d = psd_of(B, F, K, n_fft, flags, ys, ybs, ps);
                        int rc = bhwp_psd_checks(&d, nullptr, nullptr, nullptr, 0, false);
                        REQUIRE(rc == BHW_OK, "psd checks rc %d", rc);
                        const BhwPsdPlan pl = bhwp_psd_plan(&d);
                        const uint64_t Ya = 0x10000000ull, Pa = 0x100000000000ull, Wa = 0x200000000000ull;
                        rc = bhwp_psd_checks(&d, (const void *)Ya, (const void *)Pa, (const void *)Wa, pl.ws_bytes);
                        REQUIRE(rc == BHW_OK, "psd pointer checks rc %d", rc);
                        if (pl.ws_bytes) {
                            REQUIRE(bhwp_psd_checks(&d, (const void *)Ya, (const void *)Pa, (const void *)Wa, pl.ws_bytes - 1) == BHW_ERR_WORKSPACE, "short");
                            REQUIRE(bhwp_psd_checks(&d, (const void *)Ya, (const void *)Pa, nullptr, 0) == BHW_ERR_BADARG, "NULL");
                            REQUIRE(bhwp_psd_checks(&d, (const void *)Ya, (const void *)Pa, (const void *)Ya, pl.ws_bytes) == BHW_ERR_BADARG, "overlap");
                        }
                        REQUIRE(bhwp_psd_checks(&d, (const void *)Ya, (const void *)Ya, (const void *)Wa, pl.ws_bytes) == BHW_ERR_BADARG, "P in Y");
                        REQUIRE(bhwp_describe_welch(nullptr, nullptr, 0, nullptr, 0, &d, buf, sizeof buf) == BHW_OK, "describe");
                        for (uint64_t k = 0; k < K; ++k) {
                            const bool want = flags && k != 0 && !(n_fft % 2 == 0 && k == n_fft / 2);
                            REQUIRE(bhw_psd_doubled(flags, k, K, n_fft) == want, "doubled(%" PRIu64 ")", k);
                        }
                        if (B * F * K <= 400000) {
                            replay_psd(pl, d);
                            ++psd_replays;
                        }
                    }
    REQUIRE(seg_replays > 100 && psd_replays > 100, "replays %ld %ld", seg_replays, psd_replays);
    printf("ok %ld checks, %ld segment replays, %ld periodogram replays\n", g_checks, seg_replays, psd_replays);
    return 0;
}
