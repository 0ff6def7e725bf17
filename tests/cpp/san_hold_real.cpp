// san_hold_real.cpp -- the planner's part of the fused max-hold / min-hold calls for real input, both families (bhw_plan.cpp:
// bhwp_hold_fft_* and bhwp_hold_mfft_*: checks, plan, workspace bytes, describe) swept under AddressSanitizer + UBSan over every
// supported n_fft (9 powers of two, 95 mixed-radix sizes), and a host replay, lane by lane, of what bhw_hold_real.h, bhw_hold_fft.hip,
// bhw_hold_mfft.hip and the join of bhw_hold_cfft.hip do with the plan:
//   - run ownership and the padded frame map: workgroup w walks the groups first(w), next(...) of the row function under an epilogue
//     that owns runs; every group of the padded pool is visited exactly once, by the workgroup that owns its run, a run's groups in
//     ascending order and never across a signal;
//   - the live-slot mask and the reduce step, both regimes, with bin M = n_fft / 2 aside on lane 0 where the Welch sibling takes it
//     aside (M >= 256 for a power of two, M a multiple of 256 for a mixed size), on an h array of exactly B * F * K words and a
//     workspace of exactly the plan's bytes: every chunk pair is written exactly once and none outside the workspace, every
//     (b, f < F, k <= M) is reduced exactly once -- bin M by one owner, aside or not -- and no f >= F at all (a dead slot is a zero
//     row: one read of it and the minimum is 0), and what a lane carries out of a run is the identities, not zero;
//   - the join: both launches lane by lane over the same workspace, every block pair and every requested trace written once, a row
//     inside p_stride, the trace that is not asked for untouched, the one-sided factor s_k of bhw_psd_doubled;
//   - the traces equal a plain loop over the frames with float compares and the NaN rule of include/bhw.h, bit for bit, NaN and
//     infinite powers among the words.
// The arrays the replay indexes are std::vectors of exactly the sizes the contract states, so an index the asserts missed is ASan's.
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

constexpr uint32_t CH = BHW_WELCH_FFT_CHUNK, BLK = BHW_WELCH_BLOCK;
constexpr uint32_t ID_MAX = 0u, ID_MIN = 0xFFFFFFFFu;                  // the identities of the two word reductions
struct Pair { uint32_t hi, lo; };
static_assert(sizeof(Pair) == 8, "a pair is the 8 bytes of a chunk sum");

static float as_float(uint32_t w)
{
    float f;
    memcpy(&f, &w, 4);
    return f;
}
static uint32_t as_word(float f)
{
    uint32_t w;
    memcpy(&w, &f, 4);
    return w;
}

// a power as the forward call may store it: a non-negative float32 word; now and then +0.0, +inf, a NaN of either sign
static uint32_t power_word()
{
    const uint64_t r = rnd();
    switch (r % 97) {
    case 0: return 0u;
    case 1: return 0x7F800000u;
    case 2: return 0x7FC00000u;
    case 3: return 0xFFC00001u;
    default: return as_word(ldexpf((float)((r >> 20) & 0xFFFFFF) + 1.0f, (int)((r >> 50) % 60) - 40));
    }
}

// k_hold_join<GROUPED, FINAL> as bhwk_hold_join launches it, every lane of every workgroup
static void replay_join(bool grouped, bool final, const std::vector<Pair> &in, std::vector<Pair> *out, std::vector<int> *out_hit,
                        std::vector<float> *pmax, std::vector<float> *pmin, std::vector<int> &P_hit, uint64_t batch, uint64_t bins,
                        uint64_t n_fft, uint64_t n_in, uint64_t n_out, uint64_t p_stride, double scale, uint32_t psd_flags, uint64_t grid)
{
    constexpr uint32_t U = BLK / CH;
    REQUIRE(grid * 256u >= batch * n_out * bins && (grid - 1) * 256u < batch * n_out * bins, "join grid %" PRIu64, grid);
    for (uint64_t wg = 0; wg < grid; ++wg)
        for (uint32_t t = 0; t < 256; ++t) {
            const uint64_t i = wg * 256u + t;
            if (i >= batch * n_out * bins) continue;
            const uint64_t j = i % bins, rest = i / bins;
            const uint64_t o = rest % n_out, b = rest / n_out;
            const uint64_t base = b * n_in * bins + j;
            const uint64_t i0 = grouped ? o * U : 0, i1 = grouped ? (i0 + U < n_in ? i0 + U : n_in) : n_in;
            REQUIRE(i0 < i1, "an output with no input");
            uint32_t H = ID_MAX, L = ID_MIN;
            for (uint64_t c = i0; c < i1; c += U) {
                Pair v[U];
                for (uint32_t u = 0; u < U; ++u) v[u] = in.at(base + (c + u < i1 ? c + u : i1 - 1u) * bins);
                for (uint32_t u = 0; u < U; ++u) {
                    H = v[u].hi > H ? v[u].hi : H;
                    L = v[u].lo < L ? v[u].lo : L;
                }
            }
            if (final) {
                REQUIRE(j < p_stride, "a trace's row inside p_stride");
                if (H > 0x7F800000u) L = H;
                const double sk = bhw_psd_doubled(psd_flags, j, bins, n_fft) ? scale * 2.0 : scale;
                if (pmax) pmax->at(b * p_stride + j) = (float)((double)as_float(H) * sk);
                if (pmin) pmin->at(b * p_stride + j) = (float)((double)as_float(L) * sk);
                ++P_hit.at(b * p_stride + j);
            } else {
                out->at((b * n_out + o) * bins + j) = Pair{H, L};
                ++out_hit->at((b * n_out + o) * bins + j);
            }
        }
}

// One call, lane by lane.  WP: BhwWelchFftPlan or BhwWelchMfftPlan (the plan a hold plan wraps); POW2 and NACC: the template
// arguments of HoldRealAccumulate; traces: what is stored.
template <bool POW2, uint32_t NACC, class WP>
static void replay_call(const WP &wp, const bhw_stft &s, double scale, uint32_t psd_flags, uint32_t traces)
{
    const auto &pl = wp.fft;
    const uint64_t B = s.batch, F = s.frames, K = wp.bins;
    const uint32_t fy = pl.fy, M = pl.m;
    REQUIRE(K == M + 1u && 2u * M == s.n_fft && wp.fpad % wp.run == 0 && wp.run % fy == 0 && wp.run % CH == 0 && wp.fpad >= F && wp.fpad - F < wp.run, "the padded axis");
    REQUIRE(wp.gpr == wp.run / fy && (wp.gpr & (wp.gpr - 1)) == 0, "groups per run: a power of two");
    REQUIRE(pl.groups == B * wp.fpad / fy && wp.runs == B * wp.fpad / wp.run && pl.grid == (wp.runs < kFftMaxGrid ? wp.runs : kFftMaxGrid), "groups, runs, grid");
    REQUIRE(wp.chunks == (F + CH - 1) / CH && wp.blocks == (F + BLK - 1) / BLK, "chunks, blocks");
    REQUIRE(wp.ws_bytes == 8u * B * K * (wp.chunks + (wp.blocks > 1 ? wp.blocks : 0)), "workspace bytes");
    REQUIRE(wp.acc == (fy >= CH ? 0u : (uint32_t)((K + kFftBlock - 1) / kFftBlock)) && wp.acc <= NACC, "pairs carried per lane");
    REQUIRE(wp.run == (fy > CH ? fy : CH) && wp.gpr == (fy >= CH ? 1u : CH / fy), "run = max(16, fy), gpr = max(1, 16 / fy)");
    const bool aside = POW2 ? M >= kFftBlock : (M & (kFftBlock - 1u)) == 0u;
    if (fy < CH && aside) REQUIRE(POW2 || M / kFftBlock < NACC - 1u, "the last pair is free where bin M is aside (M = %u)", M);
    std::vector<uint32_t> h(B * F * K);                                                      // the powers: live frames only
    for (auto &v : h) v = power_word();
    std::vector<Pair> ws(wp.ws_bytes / 8, Pair{0x12345678u, 0x12345678u});                   // exactly the plan's bytes
    std::vector<int> ws_hit(ws.size(), 0), h_hit(h.size(), 0), group_hit(pl.groups, 0);
    const uint64_t n_chunk_ws = B * wp.chunks * K;
    for (uint64_t w = 0; w < pl.grid; ++w) {
        std::vector<Pair> acc((size_t)kFftBlock * NACC, Pair{ID_MAX, ID_MIN});               // the lanes' registers
        uint64_t prev = UINT64_MAX;
        // fft_first_group / fft_next_group (and their mfft twins) under an epilogue that owns runs
        for (uint64_t g = w * wp.gpr; g < pl.groups; g = ((g + 1u) & (wp.gpr - 1u)) ? g + 1u : g + 1u + (pl.grid - 1u) * wp.gpr) {
            ++group_hit.at(g);
            const uint64_t r0 = g * fy, b = r0 / wp.fpad, f0 = r0 - b * wp.fpad;
            REQUIRE(b < B && f0 + fy <= wp.fpad, "a group inside one signal");
            if (prev != UINT64_MAX && (g & (wp.gpr - 1u))) REQUIRE(g == prev + 1, "a run's groups in ascending order");
            REQUIRE((g / wp.gpr) % pl.grid == w, "run %" PRIu64 " belongs to workgroup %" PRIu64, g / wp.gpr, w);
            prev = g;
            if (fy >= CH) {
                const uint32_t pairs = (fy / CH) * (uint32_t)K;
                for (uint32_t tid = 0; tid < kFftBlock; ++tid)
                    for (uint32_t i = tid; i < pairs; i += kFftBlock) {
                        const uint32_t c = i / (uint32_t)K, k = i - c * (uint32_t)K;
                        const uint64_t fc = f0 + (uint64_t)c * CH;
                        if (fc >= F) continue;                                               // a padding chunk is never stored
                        const uint32_t m = F - fc < CH ? (uint32_t)(F - fc) : CH;
                        REQUIRE(m >= 1, "a stored chunk has a live frame");
                        uint32_t H = ID_MAX, L = ID_MIN;
                        for (uint32_t sl = 0; sl < m; ++sl) {
                            const uint32_t slot = c * CH + sl;
                            REQUIRE(slot < fy && k <= M && f0 + slot < F, "the slot read is live");
                            const uint64_t hi = (b * F + f0 + slot) * K + k;
                            const uint32_t v = h.at(hi);
                            ++h_hit[hi];
                            H = v > H ? v : H;
                            L = v < L ? v : L;
                        }
                        const uint64_t wi = (b * wp.chunks + fc / CH) * K + k;
                        REQUIRE(wi < n_chunk_ws, "chunk pair %" PRIu64 " of %" PRIu64, wi, n_chunk_ws);
                        ws.at(wi) = Pair{H, L};
                        ++ws_hit.at(wi);
                    }
            } else {
                const uint32_t m = f0 >= F ? 0u : F - f0 < fy ? (uint32_t)(F - f0) : fy;
                const bool last = ((g + 1u) & (wp.gpr - 1u)) == 0u;
                REQUIRE(f0 / CH < wp.chunks && (b * wp.chunks + f0 / CH + 1) * K <= n_chunk_ws, "the pointer every group of the run forms stays inside");
                // one lane's step for one of its pairs: slot `i` of its registers, bin k
                auto step = [&](uint32_t tid, uint32_t i, uint32_t k) {
                    REQUIRE(i < NACC && k <= M, "pair %u, bin %u", i, k);
                    Pair A = acc.at((size_t)tid * NACC + i);
                    for (uint32_t sl = 0; sl < m; ++sl) {
                        REQUIRE(sl < fy && f0 + sl < F, "a live slot of the group");
                        const uint64_t hi = (b * F + f0 + sl) * K + k;
                        const uint32_t v = h.at(hi);
                        ++h_hit[hi];
                        A.hi = v > A.hi ? v : A.hi;
                        A.lo = v < A.lo ? v : A.lo;
                    }
                    if (last) {
                        REQUIRE((f0 + fy) % CH == 0 && f0 / CH * CH < F, "the run's chunk exists and its first frame is live");
                        const uint64_t wi = (b * wp.chunks + f0 / CH) * K + k;
                        REQUIRE(wi < n_chunk_ws, "chunk pair %" PRIu64 " of %" PRIu64, wi, n_chunk_ws);
                        ws.at(wi) = A;
                        ++ws_hit.at(wi);
                        A = Pair{ID_MAX, ID_MIN};
                    }
                    acc.at((size_t)tid * NACC + i) = A;
                };
                for (uint32_t tid = 0; tid < kFftBlock; ++tid) {
                    for (uint32_t i = 0; i < (POW2 ? NACC - 1u : NACC); ++i) {
                        const uint32_t k = tid + i * kFftBlock;
                        if (aside ? k < M : k <= M) {
                            REQUIRE(!(aside && tid == 0u && i == NACC - 1u), "lane 0's last pair is bin M's alone");
                            step(tid, i, k);
                        }
                    }
                    if (aside && tid == 0u) step(0u, NACC - 1u, M);
                }
            }
        }
        for (const Pair &a : acc) REQUIRE(a.hi == ID_MAX && a.lo == ID_MIN, "a lane leaves its last run with the identities");
    }
    for (uint64_t g = 0; g < pl.groups; ++g) REQUIRE(group_hit[g] == 1, "group %" PRIu64 " visited %d times", g, group_hit[g]);
    for (size_t i = 0; i < h.size(); ++i) REQUIRE(h_hit[i] == 1, "power %zu (bin %zu of %u) reduced %d times", i, i % (size_t)K, M, h_hit[i]);
    for (uint64_t i = 0; i < n_chunk_ws; ++i) REQUIRE(ws_hit[i] == 1, "chunk pair %" PRIu64 " written %d times", i, ws_hit[i]);
    for (uint64_t i = n_chunk_ws; i < ws.size(); ++i) REQUIRE(ws_hit[i] == 0, "the reducing kernel writes chunk pairs only");
    // the join
    const uint64_t ps = wp.p_stride;
    std::vector<float> pmax((B - 1) * ps + K, -1.0f), pmin((B - 1) * ps + K, -1.0f);
    std::vector<float> *dmax = (traces & BHW_HOLD_MAX) ? &pmax : nullptr, *dmin = (traces & BHW_HOLD_MIN) ? &pmin : nullptr;
    std::vector<int> P_hit(pmax.size(), 0);
    std::vector<Pair> chunk_in(ws.begin(), ws.begin() + n_chunk_ws);
    if (wp.blocks == 1) {
        REQUIRE(wp.join_grid == 0, "one launch");
        replay_join(true, true, chunk_in, nullptr, nullptr, dmax, dmin, P_hit, B, K, s.n_fft, wp.chunks, 1, ps, scale, psd_flags, wp.blocks_grid);
    } else {
        std::vector<Pair> blk(ws.size() - n_chunk_ws);                                          // what follows the chunk pairs, exactly
        std::vector<int> blk_hit(blk.size(), 0);
        REQUIRE(blk.size() == B * wp.blocks * K, "the block pairs follow the chunk pairs");
        replay_join(true, false, chunk_in, &blk, &blk_hit, nullptr, nullptr, P_hit, B, K, s.n_fft, wp.chunks, wp.blocks, ps, scale, psd_flags,
                    wp.blocks_grid);
        for (size_t i = 0; i < blk.size(); ++i) REQUIRE(blk_hit[i] == 1, "block pair %zu written %d times", i, blk_hit[i]);
        replay_join(false, true, blk, nullptr, nullptr, dmax, dmin, P_hit, B, K, s.n_fft, wp.blocks, 1, ps, scale, psd_flags, wp.join_grid);
    }
    // the traces against a plain loop over the frames: float compares, and a NaN in any frame makes both traces NaN
    for (uint64_t b = 0; b < B; ++b)
        for (uint64_t j = 0; j < ps && b * ps + j < pmax.size(); ++j) {
            REQUIRE(P_hit[b * ps + j] == (j < K ? 1 : 0), "trace (%" PRIu64 ", %" PRIu64 ") written %d times", b, j, P_hit[b * ps + j]);
            if (j >= K) {
                REQUIRE(pmax[b * ps + j] == -1.0f && pmin[b * ps + j] == -1.0f, "the gap of a padded p_stride is left alone");
                continue;
            }
            float mx = -INFINITY, mn = INFINITY;
            bool nan = false;
            for (uint64_t f = 0; f < F; ++f) {
                const float v = as_float(h[(b * F + f) * K + j]);
                if (v != v) nan = true;
                else {
                    mx = v > mx ? v : mx;
                    mn = v < mn ? v : mn;
                }
            }
            // the contract's factor: doubled for every bin but 0 and, n_fft being even, M
            const double sk = ((psd_flags & BHW_PSD_ONESIDED) && j != 0 && j != M) ? scale * 2.0 : scale;
            const float wmax = (float)((double)mx * sk), wmin = (float)((double)mn * sk);
            const float gmax = pmax[b * ps + j], gmin = pmin[b * ps + j];
            if (!(traces & BHW_HOLD_MAX)) REQUIRE(gmax == -1.0f, "the maximum is not asked for and not written");
            else if (nan) REQUIRE(gmax != gmax, "a NaN power makes the maximum NaN");
            else REQUIRE(memcmp(&wmax, &gmax, 4) == 0, "max (%" PRIu64 ", %" PRIu64 "): %a != %a", b, j, gmax, wmax);
            if (!(traces & BHW_HOLD_MIN)) REQUIRE(gmin == -1.0f, "the minimum is not asked for and not written");
            else if (nan) REQUIRE(gmin != gmin, "a NaN power makes the minimum NaN");
            else REQUIRE(memcmp(&wmin, &gmin, 4) == 0, "min (%" PRIu64 ", %" PRIu64 "): %a != %a", b, j, gmin, wmin);
        }
}

static bool pow2_supported(uint64_t n) { return n >= 16 && n <= 4096 && !(n & (n - 1)); }
static bool mixed_supported(uint64_t n)
{
    if (n < 16 || n > 4095 || (n & 1) || !(n & (n - 1))) return false;
    for (const uint64_t r : {2ull, 3ull, 5ull})
        while (n % r == 0) n /= r;
    return n == 1;
}

struct Fft {
    static constexpr const char *name = "fft";
    static constexpr bool kPow2 = true;
    static constexpr uint32_t kAcc = kHoldFftMaxAcc;
    using Hold = BhwHoldFftPlan;
    static bool supported(uint64_t n) { return pow2_supported(n); }
    static int checks(const bhw_params *p, uint64_t L, const bhw_stft *s, uint32_t fl, double sc, uint32_t psd, uint64_t ps, const void *x,
                      const void *a, const void *b, const void *w, uint64_t wb, bool ptr = true)
    { return bhwp_hold_fft_checks(p, L, s, fl, sc, psd, ps, x, a, b, w, wb, ptr); }
    static int welch_checks(const bhw_params *p, uint64_t L, const bhw_stft *s, uint32_t fl, double sc, uint32_t psd, uint64_t ps)
    { return bhwp_welch_fft_checks(p, L, s, fl, sc, psd, ps, nullptr, nullptr, nullptr, 0, false); }
    static uint64_t ws(const bhw_stft *s) { return bhwp_hold_fft_workspace_bytes(s); }
    static uint64_t welch_ws(const bhw_stft *s) { return bhwp_welch_fft_workspace_bytes(s); }
    static Hold plan(const bhw_params *p, uint64_t L, const bhw_stft *s, uint32_t fl, uint64_t ps, uint32_t tr, bool tab) { return bhwp_hold_fft_plan(p, L, s, fl, ps, tr, tab); }
    static auto welch_plan(const bhw_params *p, uint64_t L, const bhw_stft *s, uint32_t fl, uint64_t ps, bool tab) { return bhwp_welch_fft_plan(p, L, s, fl, ps, tab); }
    static int describe(const bhw_params *p, uint64_t L, const bhw_stft *s, uint32_t fl, uint32_t tr, char *buf, uint64_t len) { return bhwp_describe_hold_fft(p, nullptr, L, s, fl, tr, buf, len); }
};
struct Mfft {
    static constexpr const char *name = "mfft";
    static constexpr bool kPow2 = false;
    static constexpr uint32_t kAcc = kHoldMfftMaxAcc;
    using Hold = BhwHoldMfftPlan;
    static bool supported(uint64_t n) { return mixed_supported(n); }
    static int checks(const bhw_params *p, uint64_t L, const bhw_stft *s, uint32_t fl, double sc, uint32_t psd, uint64_t ps, const void *x,
                      const void *a, const void *b, const void *w, uint64_t wb, bool ptr = true)
    { return bhwp_hold_mfft_checks(p, L, s, fl, sc, psd, ps, x, a, b, w, wb, ptr); }
    static int welch_checks(const bhw_params *p, uint64_t L, const bhw_stft *s, uint32_t fl, double sc, uint32_t psd, uint64_t ps)
    { return bhwp_welch_mfft_checks(p, L, s, fl, sc, psd, ps, nullptr, nullptr, nullptr, 0, false); }
    static uint64_t ws(const bhw_stft *s) { return bhwp_hold_mfft_workspace_bytes(s); }
    static uint64_t welch_ws(const bhw_stft *s) { return bhwp_welch_mfft_workspace_bytes(s); }
    static Hold plan(const bhw_params *p, uint64_t L, const bhw_stft *s, uint32_t fl, uint64_t ps, uint32_t tr, bool tab) { return bhwp_hold_mfft_plan(p, L, s, fl, ps, tr, tab); }
    static auto welch_plan(const bhw_params *p, uint64_t L, const bhw_stft *s, uint32_t fl, uint64_t ps, bool tab) { return bhwp_welch_mfft_plan(p, L, s, fl, ps, tab); }
    static int describe(const bhw_params *p, uint64_t L, const bhw_stft *s, uint32_t fl, uint32_t tr, char *buf, uint64_t len) { return bhwp_describe_hold_mfft(p, nullptr, L, s, fl, tr, buf, len); }
};

static long g_replays = 0, g_aside = 0;

template <class Fam>
static long sweep(const bhw_params &p)
{
    char buf[1400];
    long sizes = 0;
    const uint64_t xa = 0x10000000ull, ma = 0x100000000000ull, na = 0x180000000000ull, wa = 0x200000000000ull;
    for (uint64_t n = 1; n <= 4200; ++n) {
        if (!Fam::supported(n)) {
            bhw_stft s = desc_of(1, 1ull << 20, 2, 1, n, 0, 0, 0);
            const int rc = Fam::checks(&p, 1, &s, 0, 1.0, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, false);
            REQUIRE(rc != BHW_OK && rc == Fam::welch_checks(&p, 1, &s, 0, 1.0, 0, 0), "%s n_fft %" PRIu64 ": the sibling's refusal", Fam::name, n);
            continue;
        }
        ++sizes;
        const uint64_t K = n / 2 + 1;
        for (uint64_t L : {(uint64_t)13, n})
            for (uint64_t hop : {(uint64_t)7, n + 5})
                for (uint64_t B : {1ull, 3ull})
                    // the edges of a chunk (16), of runs of two and four chunks (32, 64) and of a block (256)
                    for (uint64_t F : {1ull, 15ull, 16ull, 17ull, 31ull, 32ull, 33ull, 63ull, 65ull, 256ull, 257ull, 531ull})
                        for (int framing = 0; framing < 3; ++framing) {                   // 0 Welch + detrend, 1 Welch, 2 centred reflect
                            const bool centred = framing >= 2;
                            const uint64_t pad = centred ? n / 2 : 0, col0 = centred ? (n - L) / 2 : 0;
                            const uint64_t reach = centred ? n : L;
                            uint64_t T = (F - 1) * hop + reach;
                            T = T > 2 * pad ? T - 2 * pad : 1;
                            if (centred && (T + 2 * pad < (F - 1) * hop + n || pad > T - 1)) continue;
                            const uint32_t flags = framing == 0 ? BHW_WELCH_DETREND_CONSTANT : 0u;
                            const uint32_t psd = (B + F + framing) % 2 ? BHW_PSD_ONESIDED : 0u;
                            const uint32_t traces = 1u + (uint32_t)((B + F + framing + n) % 3);   // max, min, both
                            bhw_stft s = desc_of(B, T, F, hop, n, col0, pad, framing == 2 ? BHW_PAD_REFLECT : BHW_PAD_CONSTANT);
                            const uint64_t ps = (B + F) % 3 == 0 ? K + 5 : 0;
                            const uint64_t need = Fam::ws(&s);
                            REQUIRE(need == Fam::welch_ws(&s) && need > 0, "the workspace is the sibling's");
                            int rc = Fam::checks(&p, L, &s, flags, 0.5, psd, ps, nullptr, nullptr, nullptr, nullptr, 0, false);
                            REQUIRE(rc == BHW_OK, "%s checks rc %d: n %" PRIu64 " L %" PRIu64 " hop %" PRIu64 " B %" PRIu64 " F %" PRIu64 " framing %d: %s", Fam::name, rc, n, L, hop, B, F, framing, bhw_last_error());
                            auto full = [&](const bhw_stft &d, uint32_t fl, double scale, uint64_t pstr, uint64_t x, uint64_t a, uint64_t b, uint64_t w, uint64_t wb) {
                                return Fam::checks(&p, L, &d, fl, scale, psd, pstr, (const void *)x, (const void *)a, (const void *)b, (const void *)w, wb);
                            };
                            REQUIRE(full(s, flags, 0.5, ps, xa, ma, na, wa, need) == BHW_OK, "pointer checks: %s", bhw_last_error());
                            REQUIRE(full(s, flags, 0.5, ps, xa, ma, 0, wa, need) == BHW_OK && full(s, flags, 0.5, ps, xa, 0, na, wa, need) == BHW_OK, "one trace alone");
                            REQUIRE(full(s, flags, 0.5, ps, xa, 0, 0, wa, need) == BHW_ERR_BADARG, "no trace");
                            REQUIRE(full(s, flags, 0.5, ps, 0, ma, na, wa, need) == BHW_ERR_BADARG, "NULL x");
                            REQUIRE(full(s, flags, 0.5, ps, xa + 4, ma + 4, na + 4, wa, need + 8) == BHW_OK, "4-byte aligned x and traces");
                            REQUIRE(full(s, flags, 0.5, ps, xa, ma + 2, na, wa, need) == BHW_ERR_BADARG && full(s, flags, 0.5, ps, xa, ma, na + 2, wa, need) == BHW_ERR_BADARG, "misaligned trace");
                            REQUIRE(full(s, flags, 0.5, ps, xa + 1, ma, na, wa, need) == BHW_ERR_BADARG, "misaligned x");
                            REQUIRE(full(s, flags, 0.5, ps, xa, ma, na, wa + 4, need) == BHW_ERR_BADARG, "misaligned workspace");
                            REQUIRE(full(s, flags, 0.5, ps, xa, ma, na, 0, need) == BHW_ERR_BADARG, "NULL workspace");
                            REQUIRE(full(s, flags, 0.5, ps, xa, ma, na, wa, need - 1) == BHW_ERR_WORKSPACE, "short workspace");
                            REQUIRE(full(s, flags, 0.5, ps, ma, ma, na, wa, need) == BHW_ERR_BADARG && full(s, flags, 0.5, ps, na, ma, na, wa, need) == BHW_ERR_BADARG, "x on a trace");
                            REQUIRE(full(s, flags, 0.5, ps, xa, ma, ma, wa, need) == BHW_ERR_BADARG && full(s, flags, 0.5, ps, xa, ma, ma + 4, wa, need) == BHW_ERR_BADARG, "max on min");
                            const uint64_t pe = ((B - 1) * (ps ? ps : K) + K) * 4;
                            REQUIRE(full(s, flags, 0.5, ps, xa, ma, ma + pe, wa, need) == BHW_OK && full(s, flags, 0.5, ps, xa, ma, ma + pe - 4, wa, need) == BHW_ERR_BADARG, "min behind max");
                            const uint64_t xe = ((B - 1) * T + T) * 4;                            // T floats of a signal: real input
                            REQUIRE(full(s, flags, 0.5, ps, xa, xa + xe, na, wa, need) == BHW_OK && full(s, flags, 0.5, ps, xa, xa + xe - 4, na, wa, need) == BHW_ERR_BADARG, "max behind x");
                            REQUIRE(full(s, flags, 0.5, ps, xa, ma, na, xa, need) == BHW_ERR_BADARG, "workspace on x");
                            REQUIRE(full(s, flags, 0.5, ps, xa, wa + need - 4, na, wa, need) == BHW_ERR_BADARG && full(s, flags, 0.5, ps, xa, ma, wa + need - 4, wa, need) == BHW_ERR_BADARG, "a trace on the workspace's end");
                            REQUIRE(full(s, flags, 0.5, ps, xa, wa + need, na, wa, need) == BHW_OK, "a trace behind the workspace");
                            REQUIRE(full(s, flags | 8u, 0.5, ps, xa, ma, na, wa, need) == BHW_ERR_BADARG, "unknown flags");
                            REQUIRE(full(s, flags, INFINITY, ps, xa, ma, na, wa, need) == BHW_ERR_BADARG && full(s, flags, NAN, ps, xa, ma, na, wa, need) == BHW_ERR_BADARG, "scale");
                            REQUIRE(Fam::checks(&p, L, &s, flags, 0.5, 2u, ps, (const void *)xa, (const void *)ma, (const void *)na, (const void *)wa, need) == BHW_ERR_BADARG, "psd_flags");
                            REQUIRE(full(s, flags, 0.5, K - 1, xa, ma, na, wa, need) == BHW_ERR_BADARG, "short p_stride");
                            bhw_stft bad = s;
                            bad.y_stride = 2 * n + 2;
                            REQUIRE(full(bad, flags, 0.5, ps, xa, ma, na, wa, need) == BHW_ERR_BADARG, "y_stride");
                            bad = s;
                            bad.channels = 2;
                            REQUIRE(full(bad, flags, 0.5, ps, xa, ma, na, wa, need) == BHW_ERR_UNSUPPORTED, "channels");
                            bad = s;
                            bad.frames = 0;
                            REQUIRE(Fam::checks(&p, L, &bad, flags, 0.5, psd, ps, nullptr, nullptr, nullptr, nullptr, 0) == BHW_OK, "frames 0");
                            REQUIRE(Fam::ws(&bad) == 0, "frames 0 needs no workspace");
                            REQUIRE(Fam::describe(&p, L, &bad, flags, traces, buf, sizeof buf) == BHW_OK && strstr(buf, "nothing (frames 0); traces: "), "describe frames 0");
                            const bool tab = (B + F) % 2 == 0;
                            const typename Fam::Hold hp = Fam::plan(&p, L, &s, flags, ps, traces, tab);
                            const auto wp = Fam::welch_plan(&p, L, &s, flags, ps, tab);
                            const auto &hw = hp.welch;
                            REQUIRE(hp.traces == traces && hw.bins == wp.bins && hw.run == wp.run && hw.gpr == wp.gpr && hw.acc == wp.acc && hw.fpad == wp.fpad &&
                                    hw.chunks == wp.chunks && hw.blocks == wp.blocks && hw.runs == wp.runs && hw.blocks_grid == wp.blocks_grid &&
                                    hw.join_grid == wp.join_grid && hw.p_stride == wp.p_stride && hw.ws_bytes == wp.ws_bytes && hw.fft.m == wp.fft.m &&
                                    hw.fft.lpf == wp.fft.lpf && hw.fft.fy == wp.fft.fy && hw.fft.cpl == wp.fft.cpl && hw.fft.lds_bytes == wp.fft.lds_bytes &&
                                    hw.fft.rows == wp.fft.rows && hw.fft.groups == wp.fft.groups && hw.fft.grid == wp.fft.grid &&
                                    hw.fft.x_stride == wp.fft.x_stride && hw.fft.route == wp.fft.route && hw.fft.detrend == wp.fft.detrend &&
                                    hw.fft.len == wp.fft.len,
                                    "the hold plan is the sibling's plan, field for field, and the traces");
                            REQUIRE(hp.welch.ws_bytes == need && hp.welch.p_stride == (ps ? ps : K), "workspace and p_stride");
                            REQUIRE(Fam::describe(&p, L, &s, flags, traces, buf, sizeof buf) == BHW_OK && strlen(buf) > 80 && strlen(buf) < sizeof buf - 1, "describe");
                            REQUIRE(strstr(buf, "k_hold_join") && strstr(buf, "chunk 16 frames") && strstr(buf, "workspace") && !strstr(buf, "welch") &&
                                    strstr(buf, traces == 3 ? "; traces: max, min" : traces == 1 ? "; traces: max" : "; traces: min"),
                                    "the line's own fields in %s", buf);
                            // every size is replayed at the edges of a chunk and a run, with one signal and with three, doubled and not, each
                            // selection of traces; the edges of a block at the sizes up to 512, where the h array stays small
                            if (hop == 7 && L == n && framing == (int)((B + F) % 2) && (F <= 65 || n <= 512)) {
                                replay_call<Fam::kPow2, Fam::kAcc>(hp.welch, s, 1.0 / (3.7 * (double)F), psd, traces);
                                ++g_replays;
                                const uint32_t M = hp.welch.fft.m;
                                if (hp.welch.fft.fy < CH && (Fam::kPow2 ? M >= kFftBlock : M % kFftBlock == 0)) ++g_aside;
                            }
                        }
    }
    return sizes;
}

int main()
{
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 12, 24);
    const long pow2 = sweep<Fft>(p);
    const long aside_pow2 = g_aside;
    const long mixed = sweep<Mfft>(p);
    REQUIRE(pow2 == 9 && mixed == 95, "supported sizes %ld + %ld", pow2, mixed);
    REQUIRE(aside_pow2 > 0 && g_aside > aside_pow2, "bin M aside was replayed in both families (%ld, %ld)", aside_pow2, g_aside - aside_pow2);
    for (uint32_t psd : {0u, (uint32_t)BHW_PSD_ONESIDED}) {   // more runs than workgroups, 513 blocks through the join: 131 142 frames
        bhw_stft s = desc_of(1, 262300, 131142, 2, 18, 1, 0, 0);
        REQUIRE(bhwp_hold_mfft_checks(&p, 16, &s, 0, 1.0, psd, 0, nullptr, nullptr, nullptr, nullptr, 0, false) == BHW_OK, "the long case: %s", bhw_last_error());
        const BhwHoldMfftPlan hp = bhwp_hold_mfft_plan(&p, 16, &s, 0, 0, BHW_HOLD_MAX | BHW_HOLD_MIN, false);
        REQUIRE(hp.welch.runs > kFftMaxGrid && hp.welch.fft.grid == kFftMaxGrid && hp.welch.blocks == 513 && hp.welch.fft.fy == 64, "the long mixed case");
        replay_call<false, kHoldMfftMaxAcc>(hp.welch, s, 0.25, psd, hp.traces);
        ++g_replays;
        bhw_stft t = desc_of(1, 262298, 131142, 2, 16, 0, 0, 0);
        REQUIRE(bhwp_hold_fft_checks(&p, 16, &t, 0, 1.0, psd, 0, nullptr, nullptr, nullptr, nullptr, 0, false) == BHW_OK, "the long case: %s", bhw_last_error());
        const BhwHoldFftPlan hq = bhwp_hold_fft_plan(&p, 16, &t, 0, 0, BHW_HOLD_MIN, false);
        REQUIRE(hq.welch.runs > kFftMaxGrid && hq.welch.fft.grid == kFftMaxGrid && hq.welch.blocks == 513 && hq.welch.fft.fy == 64, "the long power-of-two case");
        replay_call<true, kHoldFftMaxAcc>(hq.welch, t, 0.25, psd, hq.traces);
        ++g_replays;
    }
    REQUIRE(bhwp_hold_fft_checks(&p, 16, nullptr, 0, 1.0, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, false) == BHW_ERR_BADARG, "NULL descriptor");
    REQUIRE(bhwp_hold_fft_workspace_bytes(nullptr) == 0 && bhwp_hold_mfft_workspace_bytes(nullptr) == 0, "NULL descriptor needs nothing");
    REQUIRE(g_replays >= 104 * 8, "replays %ld", g_replays);
    printf("ok %ld checks, %ld call replays over %ld + %ld sizes\n", g_checks, g_replays, pow2, mixed);
    return 0;
}
