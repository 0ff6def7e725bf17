// san_logspec.cpp -- the planner's part of the fused log spectrogram / MFCC calls (bhw_plan.cpp: bhwp_logspec_checks, bhwp_logspec_plan,
// bhwp_logspec_mfft_plan, bhwp_describe_logspec) swept under AddressSanitizer + UBSan for both radix families, and a host replay, lane
// by lane, of log_row of bhw_logspec.h:
//   - power rows: every output column k < K of a live row is written exactly once;
//   - bank rows: every power of the slot is staged exactly once before the first barrier; between the barriers every filter m is
//     written exactly once -- to the output row (coeffs 0) or to the slot's log row g, which lives in the buffer the split pass read
//     (src): g is never written before the first barrier (a power may still be formed from src) and never read before the second;
//     every power read lies inside the slot's K floats and every weight read inside [0, weights);
//   - DCT: after the second barrier every output column j < coeffs is written exactly once, every read of g lies inside n_fft floats
//     and below `filters`, every read of the matrix inside filters * coeffs floats; with consistent banks the result is compared with
//     the contract's plain binary64 sums bit for bit.
// Consistent banks and deliberately inconsistent ones (offsets not ascending or past `weights`, `first` at or past K or at the top of
// uint32); the inconsistent ones never run on a GPU.  The arrays the replay indexes are std::vectors of exactly K, `weights`, n_fft
// and filters * coeffs elements, so an index the asserts missed is ASan's.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
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
static double unit() { return (double)(rnd() >> 11) / 9007199254740992.0; }

static bhw_stft desc_of(uint64_t B, uint64_t T, uint64_t frames, uint64_t hop, uint64_t n_fft)
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
    s.shift = 15;
    return s;
}

struct Bank {
    std::vector<uint32_t> first, offset;
    std::vector<float> weight;
    uint32_t filters, weights;          // what the descriptor says
};

static const uint64_t kFirst = 0x200000000000ull, kOffset = 0x200000100000ull, kWeight = 0x200000200000ull, kDct = 0x200010000000ull;

static bhw_fbank fbank_of(const Bank &bk, uint32_t bins)
{
    bhw_fbank fb;
    memset(&fb, 0, sizeof fb);
    fb.struct_size = sizeof fb;
    fb.filters = bk.filters;
    fb.bins = bins;
    fb.weights = bk.weights;
    fb.d_first = (const uint32_t *)kFirst;                       // never dereferenced by the planner
    fb.d_offset = (const uint32_t *)kOffset;
    fb.d_weight = (const float *)kWeight;
    return fb;
}

static bhw_logspec log_of(uint32_t mode, double floor, double mult, uint32_t coeffs, uint32_t rows)
{
    bhw_logspec ls;
    memset(&ls, 0, sizeof ls);
    ls.struct_size = sizeof ls;
    ls.mode = mode;
    ls.floor = floor;
    ls.mult = mult;
    ls.coeffs = coeffs;
    ls.dct_rows = rows;
    ls.d_dct = coeffs ? (const float *)kDct : nullptr;
    return ls;
}

static Bank consistent_bank(uint32_t K, uint32_t filters)
{
    Bank bk;
    bk.filters = filters;
    bk.first.resize(filters);
    bk.offset.assign(filters + 1, 0);
    for (uint32_t m = 0; m < filters; ++m) {
        const uint32_t kind = (uint32_t)(rnd() % 8);
        uint32_t k0 = (uint32_t)(rnd() % K), c = (uint32_t)(rnd() % (K - k0 + 1));
        if (kind == 0) c = 0;
        if (kind == 1) k0 = 0, c = K;
        if (kind == 2) k0 = K - 1, c = 1;
        bk.first[m] = k0;
        bk.offset[m + 1] = bk.offset[m] + c;
        for (uint32_t i = 0; i < c; ++i) bk.weight.push_back((float)(unit() - 0.25));
    }
    bk.weights = bk.offset[filters];
    return bk;
}

static float log_word(const bhw_logspec &ls, float q)
{
    const double d = (double)q;
    const double t = ls.mode == BHW_LOG_ADD ? d + ls.floor : (d < ls.floor ? ls.floor : d);
    return (float)(ls.mult * log(t));
}

// log_row for one live slot, every lane in the kernel's order.  M, lpf: the plan's; n = n_fft.
static void replay_row(uint32_t M, uint32_t lpf, uint32_t n, const Bank *bk, const bhw_logspec &ls, bool consistent)
{
    const uint32_t K = M + 1;
    REQUIRE(K <= n, "K powers inside the idle buffer's n_fft floats");
    std::vector<float> power(K);
    for (uint32_t k = 0; k < K; ++k) power[k] = (float)(unit() * 100.0);
    if (!bk) {
        std::vector<int> hit(K, 0);
        std::vector<float> out(K);
        for (uint32_t l = 0; l < lpf; ++l)
            for (uint32_t k = l; k <= M; k += lpf) {
                out.at(k) = log_word(ls, power[k]);
                ++hit[k];
            }
        for (uint32_t k = 0; k < K; ++k) REQUIRE(hit[k] == 1 && !std::isnan(out[k]), "log column %u written %d times", k, hit[k]);
        return;
    }
    int phase = 0;                                                    // 0: before the first barrier, 1: between, 2: after the second
    std::vector<float> pw(K), gs(n), out(ls.coeffs ? ls.coeffs : bk->filters, -1.0f);   // exactly K and n_fft: ASan guards the rest
    std::vector<int> pw_hit(K, 0), g_hit(n, 0), out_hit(out.size(), 0);
    for (uint32_t l = 0; l < lpf; ++l)
        for (uint32_t k = l; k <= M; k += lpf) {
            REQUIRE(phase == 0, "src is read by the split pass");
            pw.at(k) = power[k];
            ++pw_hit[k];
        }
    for (uint32_t k = 0; k < K; ++k) REQUIRE(pw_hit[k] == 1, "power %u staged %d times", k, pw_hit[k]);
    phase = 1;                                                        // -- the first barrier: every split pass is done, src is dead --
    const uint32_t W = bk->weights;
    REQUIRE(bk->weight.size() == W, "the weight array holds `weights` floats");
    if (ls.coeffs) REQUIRE(bk->filters <= n, "the host check: filters <= n_fft under a DCT");
    const float *pwp = pw.data(), *wp = bk->weight.data();
    for (uint32_t l = 0; l < lpf; ++l)
        for (uint32_t m = l; m < bk->filters; m += lpf) {
            uint32_t o0 = bk->offset.at(m), o1 = bk->offset.at(m + 1u);
            o0 = o0 < W ? o0 : W;
            o1 = o1 < W ? o1 : W;
            o1 = o1 < o0 ? o0 : o1;
            const uint32_t k0 = bk->first.at(m);
            uint32_t c = o1 - o0;
            const uint32_t room = k0 < K ? K - k0 : 0u;
            c = c < room ? c : room;
            double acc = 0.0;
            for (uint32_t i = 0; i < c; ++i) {
                REQUIRE((uint64_t)k0 + i < K, "filter %u reads power %" PRIu64 " of %u", m, (uint64_t)k0 + i, K);
                REQUIRE((uint64_t)o0 + i < W, "filter %u reads weight %" PRIu64 " of %u", m, (uint64_t)o0 + i, W);
                acc = fma((double)pwp[k0 + i], (double)wp[o0 + i], acc);
            }
            const float g = log_word(ls, (float)acc);
            if (ls.coeffs) {
                REQUIRE(phase == 1 && m < n, "g[%u] is written between the barriers, inside n_fft = %u floats", m, n);
                gs.at(m) = g;
                ++g_hit[m];
            } else {
                out.at(m) = g;
                ++out_hit[m];
            }
        }
    if (!ls.coeffs) {
        for (uint32_t m = 0; m < bk->filters; ++m) REQUIRE(out_hit[m] == 1, "log-bank column %u written %d times", m, out_hit[m]);
        if (consistent)
            for (uint32_t m = 0; m < bk->filters; ++m) {
                double acc = 0.0;
                for (uint32_t i = bk->offset[m]; i < bk->offset[m + 1]; ++i) acc += (double)pw[bk->first[m] + (i - bk->offset[m])] * (double)bk->weight[i];
                const float want = log_word(ls, (float)acc);
                REQUIRE(memcmp(&want, &out[m], 4) == 0 || (std::isnan(want) && std::isnan(out[m])), "filter %u: %a != %a", m, out[m], want);
            }
        return;
    }
    for (uint32_t m = 0; m < n; ++m) REQUIRE(g_hit[m] == (m < bk->filters ? 1 : 0), "g[%u] written %d times", m, g_hit[m]);
    phase = 2;                                                        // -- the second barrier: every g of the slot is in place --
    std::vector<float> dct((size_t)bk->filters * ls.coeffs);          // exactly filters * coeffs
    for (float &v : dct) v = (float)(unit() - 0.4);
    const float *gp = gs.data(), *dp = dct.data();
    for (uint32_t l = 0; l < lpf; ++l)
        for (uint32_t j = l; j < ls.coeffs; j += lpf) {
            double acc = 0.0;
            for (uint32_t m = 0; m < bk->filters; ++m) {
                const size_t at = (size_t)m * ls.coeffs + j;
                REQUIRE(phase == 2 && m < n && g_hit[m] == 1 && at < dct.size(), "coefficient %u reads g[%u], matrix word %zu of %zu", j, m, at, dct.size());
                acc = fma((double)gp[m], (double)dp[at], acc);
            }
            out.at(j) = (float)acc;
            ++out_hit[j];
        }
    for (uint32_t j = 0; j < ls.coeffs; ++j) REQUIRE(out_hit[j] == 1, "coefficient %u written %d times", j, out_hit[j]);
    for (uint32_t j = 0; j < ls.coeffs; ++j) {
        double acc = 0.0;                                             // the contract: ascending m, binary64, from +0.0
        for (uint32_t m = 0; m < bk->filters; ++m) acc += (double)gs[m] * (double)dct[(size_t)m * ls.coeffs + j];
        const float want = (float)acc;
        REQUIRE(memcmp(&want, &out[j], 4) == 0 || (std::isnan(want) && std::isnan(out[j])), "coefficient %u: %a != %a", j, out[j], want);
    }
}

template <class Plan, class Parent>
static void same_plan(const Plan &pl, const Parent &pa)
{
    REQUIRE(pl.m == pa.m && pl.lpf == pa.lpf && pl.fy == pa.fy && pl.cpl == pa.cpl && pl.groups == pa.groups && pl.grid == pa.grid &&
            pl.lds_bytes == pa.lds_bytes && pl.rows == pa.rows && pl.x_stride == pa.x_stride && pl.detrend == pa.detrend, "the parent's plan");
}

int main()
{
    char buf[1400];
    long replays = 0, bad_banks = 0, sizes = 0;
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 12, 24);
    const void *xa = (const void *)0x10000000ull, *ya = (const void *)0x100000000000ull;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (uint64_t n = 16; n <= 4096; ++n) {
        const bool pow2 = !(n & (n - 1)), mix = bhwp_mfft_supported(n);
        if (!pow2 && !mix) continue;
        ++sizes;
        const bool mixed = mix;
        const uint32_t K = (uint32_t)(n / 2 + 1);
        // every size runs a few banks; the whole sweep runs at the powers of two and a handful of mixed sizes
        const bool full = pow2 || n == 18 || n == 400 || n == 1200 || n == 4050;
        std::vector<uint32_t> filter_counts = {0u, 10u, (uint32_t)n};
        if (full) filter_counts = {0u, 1u, 3u, 10u, 80u, K - 1u, K, (uint32_t)n - 1u, (uint32_t)n};
        for (uint32_t filters : filter_counts) {
            if (filters > kSpecMaxFilters) continue;
            Bank bk;
            if (filters) bk = consistent_bank(K, filters);
            const Bank *bp = filters ? &bk : nullptr;
            bhw_fbank fb = fbank_of(bk, K);
            const bhw_fbank *f = filters ? &fb : nullptr;
            std::vector<uint32_t> coeff_counts = {0u};
            if (filters) coeff_counts = full ? std::vector<uint32_t>{0u, 1u, 13u, filters <= 512u ? filters : 512u, 300u} : std::vector<uint32_t>{0u, 13u};
            for (uint32_t coeffs : coeff_counts)
                for (uint32_t mode : {BHW_LOG_CLAMP, BHW_LOG_ADD}) {
                    if (coeffs && filters > n) continue;               // refused: swept below
                    const bhw_logspec ls = log_of(mode, mode ? 1.0 : 1e-10, mode ? -2.5 : 1.0, coeffs, coeffs ? filters : 0u);
                    const uint64_t W = coeffs ? coeffs : filters ? filters : K;
                    for (int padded = 0; padded <= 1; ++padded)
                        for (uint32_t flags : {0u, (uint32_t)BHW_WELCH_DETREND_CONSTANT}) {
                            const uint64_t B = 3, F = 65, hop = 7, L = n;
                            bhw_stft s = desc_of(B, (F - 1) * hop + L, F, hop, n);
                            if (padded) {
                                s.x_stride = s.samples + 3;
                                s.y_stride = W + 5;
                                s.y_batch_stride = F * s.y_stride + 9;
                            }
                            int rc = bhwp_logspec_checks(mixed, &p, L, &s, flags, f, &ls, nullptr, nullptr, false);
                            REQUIRE(rc == BHW_OK, "checks rc %d: n %" PRIu64 " filters %u coeffs %u: %s", rc, n, filters, coeffs, bhw_last_error());
                            REQUIRE(bhwp_logspec_checks(mixed, &p, L, &s, flags, f, &ls, xa, ya) == BHW_OK, "pointer checks: %s", bhw_last_error());
                            REQUIRE(bhwp_logspec_checks(!mixed, &p, L, &s, flags, f, &ls, xa, ya) == BHW_ERR_UNSUPPORTED, "the other family");
                            REQUIRE(strstr(bhw_last_error(), mixed ? "bhw_logspec_mfft_f32_*" : "bhw_logspec_f32_*") != nullptr, "names the call: %s", bhw_last_error());
                            REQUIRE(bhwp_logspec_checks(mixed, &p, L, &s, flags, f, &ls, xa, (const char *)ya + 2) == BHW_ERR_BADARG, "misaligned output");
                            REQUIRE(bhwp_logspec_checks(mixed, &p, L, &s, flags, f, &ls, ya, ya) == BHW_ERR_BADARG, "overlap");
                            REQUIRE(bhwp_logspec_checks(mixed, &p, L, &s, flags | BHW_MFFT_POWER, f, &ls, nullptr, nullptr, false) == BHW_ERR_BADARG, "flags");
                            bhw_stft bad = s;
                            bad.y_stride = W - 1;
                            if (W > 1) REQUIRE(bhwp_logspec_checks(mixed, &p, L, &bad, flags, f, &ls, nullptr, nullptr, false) == BHW_ERR_BADARG, "short y_stride");
                            bad = s;
                            bad.y_batch_stride = (F - 1) * (s.y_stride ? s.y_stride : W) + W - 1;
                            REQUIRE(bhwp_logspec_checks(mixed, &p, L, &bad, flags, f, &ls, nullptr, nullptr, false) == BHW_ERR_BADARG, "short y_batch_stride");
                            bad = s;
                            bad.frames = 0;
                            REQUIRE(bhwp_logspec_checks(mixed, &p, L, &bad, flags, f, &ls, nullptr, nullptr) == BHW_OK, "frames 0");
                            REQUIRE(bhwp_describe_logspec(mixed, &p, nullptr, L, &bad, flags, f, &ls, buf, sizeof buf) == BHW_OK && strstr(buf, "frames 0"), "describe frames 0");
                            REQUIRE(bhwp_describe_logspec(mixed, &p, nullptr, L, &s, flags, f, &ls, buf, sizeof buf) == BHW_OK && strlen(buf) > 60, "describe");
                            REQUIRE(strstr(buf, " signals x ") && strstr(buf, "bytes of LDS") && strstr(buf, mode ? "log add" : "log clamp"), "line %s", buf);
                            uint32_t M, lpf;
                            if (mixed) {
                                const BhwStftMfftPlan pl = bhwp_logspec_mfft_plan(&p, L, &s, flags, f, &ls, padded != 0);
                                same_plan(pl, bhwp_stft_mfft_plan(&p, L, &s, flags | BHW_MFFT_POWER, f, padded != 0));
                                REQUIRE(pl.y_stride == (padded ? W + 5 : W) && pl.y_bstride == (padded ? F * (W + 5) + 9 : F * W), "strides");
                                REQUIRE(pl.form == (f ? BHWP_MFFT_BANK : BHWP_MFFT_POWER), "form");
                                M = pl.m, lpf = pl.lpf;
                            } else {
                                const BhwStftFftPlan pl = bhwp_logspec_plan(&p, L, &s, flags, f, &ls, padded != 0);
                                same_plan(pl, bhwp_spectrogram_plan(&p, L, &s, flags, f, padded != 0));
                                REQUIRE(pl.y_stride == (padded ? W + 5 : W) && pl.y_bstride == (padded ? F * (W + 5) + 9 : F * W), "strides");
                                M = pl.m, lpf = pl.lpf;
                            }
                            if (padded || flags) continue;
                            replay_row(M, lpf, (uint32_t)n, bp, ls, true);
                            ++replays;
                            if (!filters || !full || coeffs > 13u) continue;
                            for (int kind = 0; kind < 6; ++kind) {     // deliberately inconsistent banks: the replay alone (never a GPU)
                                Bank wrong = bk;
                                for (uint32_t m = 0; m < filters; ++m) {
                                    if (kind == 0) wrong.offset[m + 1] = (uint32_t)rnd();
                                    if (kind == 1 && m % 2) std::swap(wrong.offset[m], wrong.offset[m + 1]);
                                    if (kind == 2) wrong.offset[m + 1] = wrong.offset[m + 1] + bk.weights + 1u;
                                    if (kind == 3) wrong.first[m] = K + (uint32_t)(rnd() % 5);
                                    if (kind == 4) wrong.first[m] = 0xFFFFFFFFu - (uint32_t)(rnd() % 3);
                                    if (kind == 5) wrong.first[m] = K - 1, wrong.offset[m] = 0, wrong.offset[m + 1] = bk.weights;
                                }
                                replay_row(M, lpf, (uint32_t)n, &wrong, ls, false);
                                ++bad_banks;
                            }
                            Bank half = bk;                            // a descriptor that claims fewer weights than the offsets reach
                            half.weights = bk.weights / 2;
                            half.weight.resize(half.weights);
                            replay_row(M, lpf, (uint32_t)n, &half, ls, false);
                            ++bad_banks;
                        }
                }
            if (!filters || !full || filters > n) continue;
            // the refusals of the log descriptor, in the header's order: each fails at its own check with every later one wrong too
            bhw_stft s = desc_of(2, 20 * n, 3, n, n);
            const uint32_t rows = filters;
            auto refused = [&](const bhw_fbank *bank, const bhw_logspec *l, const char *word) {
                const int rc = bhwp_logspec_checks(mixed, &p, n, &s, 0, bank, l, xa, ya);
                REQUIRE(rc == BHW_ERR_BADARG && strstr(bhw_last_error(), word), "wanted '%s', got %d: %s", word, rc, bhw_last_error());
            };
            bhw_logspec l2 = log_of(7, -1.0, 0.0, 5000, rows + 1);
            refused(f, nullptr, "log descriptor is NULL");
            l2.struct_size = 40, l2.reserved = 1;
            refused(f, &l2, "struct_size");
            l2.struct_size = sizeof l2;
            refused(f, &l2, "reserved");
            l2.reserved = 0;
            refused(f, &l2, "mode");
            l2.mode = BHW_LOG_ADD;
            for (double v : {-1.0, 0.0, inf, -inf, nan}) {
                l2.floor = v;
                refused(f, &l2, "floor");
            }
            l2.floor = 1e-300;
            for (double v : {0.0, -0.0, inf, -inf, nan}) {
                l2.mult = v;
                refused(f, &l2, "mult");
            }
            l2.mult = -1e300;
            refused(f, &l2, "coeffs 5000");
            l2.coeffs = 4096;
            refused(nullptr, &l2, "without a filter bank");
            refused(f, &l2, "dct_rows");
            l2.dct_rows = rows;
            bhw_fbank wide = fb;
            wide.filters = (uint32_t)n + 1;
            l2.dct_rows = (uint32_t)n + 1;
            if (n + 1 <= kSpecMaxFilters) refused(&wide, &l2, "above n_fft");
            l2.dct_rows = rows;
            l2.d_dct = nullptr;
            refused(f, &l2, "d_dct is NULL");
            l2.d_dct = (const float *)(kDct + 2);
            refused(f, &l2, "d_dct is not 4-byte aligned");
            const uint64_t obytes = 2ull * 3 * 4096 * 4, dbytes = (uint64_t)rows * 4096 * 4;
            l2.d_dct = (const float *)((const char *)ya + obytes - 4);
            refused(f, &l2, "d_dct and d_out overlap");
            l2.d_dct = (const float *)((const char *)ya - dbytes + 4);
            refused(f, &l2, "d_dct and d_out overlap");
            l2.d_dct = (const float *)((const char *)ya + obytes);
            REQUIRE(bhwp_logspec_checks(mixed, &p, n, &s, 0, f, &l2, xa, ya) == BHW_OK, "matrix behind the output: %s", bhw_last_error());
            l2.d_dct = (const float *)((const char *)ya - dbytes);
            REQUIRE(bhwp_logspec_checks(mixed, &p, n, &s, 0, f, &l2, xa, ya) == BHW_OK, "matrix ends at the output: %s", bhw_last_error());
            l2.d_dct = (const float *)(kFirst - dbytes + 4);
            refused(f, &l2, "d_dct and bhw_fbank.d_first overlap");
            l2.d_dct = (const float *)(kOffset + 4ull * filters);
            refused(f, &l2, "d_dct and bhw_fbank.d_offset overlap");
            if (fb.weights) {
                l2.d_dct = (const float *)(kWeight + 4ull * fb.weights - 4);
                refused(f, &l2, "d_dct and bhw_fbank.d_weight overlap");
            }
            l2.d_dct = (const float *)(kWeight + 4ull * fb.weights);
            REQUIRE(bhwp_logspec_checks(mixed, &p, n, &s, 0, f, &l2, xa, ya) == BHW_OK, "matrix behind the weights: %s", bhw_last_error());
            // the parent's refusals of the bank come first, in its words
            bhw_fbank b2 = fb;
            b2.bins = K - 1;
            refused(&b2, nullptr, "bhw_fbank.bins");
            b2 = fb, b2.d_first = nullptr;
            l2.d_dct = nullptr;
            refused(&b2, &l2, "d_first / d_offset is NULL");
        }
    }
    bhw_logspec ls = log_of(BHW_LOG_CLAMP, 1e-10, 1.0, 0, 0);
    REQUIRE(bhwp_logspec_checks(false, &p, 16, nullptr, 0, nullptr, &ls, nullptr, nullptr, false) == BHW_ERR_BADARG, "NULL descriptor");
    REQUIRE(bhwp_logspec_checks(true, &p, 16, nullptr, 0, nullptr, &ls, nullptr, nullptr, false) == BHW_ERR_BADARG, "NULL descriptor");
    for (uint64_t n : {8ull, 14ull, 442ull, 4098ull, 8192ull})
        for (bool mixed : {false, true}) {
            bhw_stft s = desc_of(1, 1ull << 33, 2, 1, n);
            REQUIRE(bhwp_logspec_checks(mixed, &p, 1, &s, 0, nullptr, &ls, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED, "n_fft %" PRIu64, n);
        }
    {
        bhw_stft s = desc_of(2, 4000, 3, 16, 16);
        s.channels = 2;
        for (bool mixed : {false, true}) {
            s.n_fft = mixed ? 18 : 16;
            REQUIRE(bhwp_logspec_checks(mixed, &p, 16, &s, 0, nullptr, &ls, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED && strstr(bhw_last_error(), "real input"), "channels 2: %s", bhw_last_error());
        }
    }
    REQUIRE(sizes == 9 + 95 && replays >= 1000 && bad_banks >= 1000, "sizes %ld replays %ld bad banks %ld", sizes, replays, bad_banks);
    printf("ok %ld checks, %ld sizes, %ld epilogue replays, %ld inconsistent banks\n", g_checks, sizes, replays, bad_banks);
    return 0;
}
