// san_cmask.cpp -- the planner's part of the fused STFT + complex gain + inverse STFT calls of both families (bhw_plan.cpp:
// bhwp_cmask_fft_checks / bhwp_cmask_mfft_checks, the real-gain plans they run, bhwp_describe_cmask_fft / _mfft) swept under
// AddressSanitizer + UBSan over all 8 + 73 supported n_fft against L, hop, batch, frames and the output length at the edges, both padding
// rules, centred and not, packed and padded strides and every gain stride form.  Besides "no report" it asserts that
//   - the checks pass what the real-gain checks pass, and the plan used is the real-gain plan for the same arguments (the strides in
//     pairs), at most 8 columns per lane and 40 960 / 40 000 bytes of LDS;
//   - the describe line names k_cmask_*_direct and "complex gains", and is the real-gain line otherwise;
//   - a 4-byte aligned d_g is refused, and a d_out that begins in the second half of the gain array is refused (8-byte elements);
// and it replays, lane by lane, the gain-pair reads of MaskSourceT<fft_v2f>::frame / MaskMfftSourceT<fft_v2f>::frame (step c.: the lane
// of k <= floor(M / 2) loads the pairs of k, ascending, and of M - k, descending) on a FLOAT array of exactly the contract's size --
// 2 * ((B - 1) * g_batch_stride + (frames - 1) * g_stride + K) floats -- under every stride form: every float index 2 * (...) and
// 2 * (...) + 1 inside the extent and never in a gap, every pair 0..M of a row read, with M odd and M even.  The other index arithmetic of
// the kernels is the real-gain kernels' text, which tests/cpp/san_mask_fft.cpp and san_mask_mfft.cpp replay.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "bhw_plan.h"

static long g_checks = 0, g_replays = 0, g_odd = 0, g_even = 0;
#define REQUIRE(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static bhw_stft desc_of(uint64_t B, uint64_t T, uint64_t frames, uint64_t hop, uint64_t n_fft, uint64_t col0, uint64_t pad, uint32_t pad_mode,
                        uint64_t x_stride)
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
    s.pad_mode = pad_mode;
    s.x_stride = x_stride;
    s.shift = 15;
    return s;
}

// The gain-pair reads of one call: g is a float array of exactly the contract's extent; ASan holds the accesses to it.
static void replay_gain_reads(uint32_t M, uint32_t lpf, uint64_t Bn, uint64_t F, uint64_t gs, uint64_t gbs)
{
    const uint64_t K = (uint64_t)M + 1;
    const uint32_t H = M >> 1;
    const uint64_t pairs = (Bn - 1) * gbs + (F - 1) * gs + K;
    std::vector<float> g(2 * pairs, 1.0f);
    std::vector<uint8_t> gap(2 * pairs, 1), seen(K);
    const uint64_t nb_rows = gbs ? Bn : 1, f_rows = gs ? F : 1;
    for (uint64_t b = 0; b < nb_rows; ++b)
        for (uint64_t f = 0; f < f_rows; ++f)
            for (uint64_t k = 0; k < 2 * K; ++k) gap[2 * (b * gbs + f * gs) + k] = 0;
    ++(M & 1u ? g_odd : g_even);
    float sum = 0.0f;
    for (uint64_t b = 0; b < Bn; ++b)
        for (uint64_t f = 0; f < F; ++f) {
            std::fill(seen.begin(), seen.end(), 0);
            const uint64_t row = b * gbs + f * gs;                       // const G *gp = g + b * g_bstride + f * g_stride, G a pair
            for (uint32_t l = 0; l < lpf; ++l) {
                uint64_t up = 0, down = 0;
                bool first = true;
                for (uint32_t k = l; k <= H; k += lpf) {
                    const uint64_t qa = k, qb = M - k;                   // gp[k], gp[M - k]
                    REQUIRE(first || (qa > up && qb < down), "pairs of lane %u not ascending / descending", l);
                    first = false;
                    up = qa;
                    down = qb;
                    for (uint64_t q : {qa, qb})
                        for (uint64_t part = 0; part < 2; ++part) {
                            const uint64_t at = 2 * (row + q) + part;
                            REQUIRE(at < g.size() && !gap.at(at), "float %" PRIu64 " of pair %" PRIu64 " of frame %" PRIu64 " outside its row", at, q, f);
                            sum += g.at(at);
                        }
                    REQUIRE((2 * (row + qa)) % 2 == 0, "a pair begins at an even float");
                    seen.at(qa) = 1;
                    seen.at(qb) = 1;
                }
            }
            for (uint64_t k = 0; k < K; ++k) REQUIRE(seen[k] == 1, "pair %" PRIu64 " not read", k);
        }
    REQUIRE(sum > 0.0f, "reads");
    ++g_replays;
}

template <typename Checks, typename RealChecks, typename Plan, typename Describe, typename RealDescribe>
static void family(const char *fam, const std::vector<uint64_t> &sizes, uint32_t max_lds, Checks checks, RealChecks real_checks, Plan plan,
                   Describe describe, RealDescribe real_describe)
{
    bhw_params p;
    REQUIRE(bhw_params_init(&p, BHW_WIN_BH4, 12, 16) == BHW_OK, "params");
    char line[1280], real[1280], kname[64], rname[64];
    snprintf(kname, sizeof kname, "k_cmask_%s_direct", fam);
    snprintf(rname, sizeof rname, "k_mask_%s_direct", fam);
    // addresses that are never dereferenced: the checks only compare them
    const char *X = (const char *)0x10000000, *G = (const char *)0x4000000000ull, *O = (const char *)0x8000000000ull;
    uint64_t combo = 0;
    for (uint64_t n : sizes) {
        const uint64_t K = n / 2 + 1;
        for (uint64_t L : {(uint64_t)1, (uint64_t)13, n / 2 + 1, n})
            for (uint64_t hop : {(uint64_t)1, n / 4 + 3, n + 5})
                for (uint64_t nb : {1, 3})
                    for (uint64_t F : {1, 2, 65})
                        for (int center = 0; center < 2; ++center)
                            for (uint32_t mode : {(uint32_t)BHW_PAD_REFLECT, (uint32_t)BHW_PAD_CONSTANT})
                                for (int extra : {0, -1, 1}) {
                                    if (L > n || (!center && L < n)) continue;
                                    const uint64_t pad = center ? n / 2 : 0, col0 = (n - L) / 2;
                                    const uint64_t Tin = n + hop * (F - 1) - 2 * pad;
                                    if (Tin < 1 || (mode == BHW_PAD_REFLECT && pad > Tin - 1)) continue;
                                    const int64_t Ts = (int64_t)Tin + (extra < 0 ? -1 : extra > 0 ? (int64_t)(n + 2 * hop + 3) : 0);
                                    if (Ts < 1) continue;
                                    const uint64_t T = (uint64_t)Ts;
                                    const bool padded = (n / 2 + F + nb) % 2 == 0;
                                    const bhw_stft sa = desc_of(nb, Tin, F, hop, n, col0, pad, mode, padded ? Tin + 3 : 0);
                                    const bhw_stft ss = desc_of(nb, T, F, hop, n, col0, pad, 0, padded ? T + 5 : 0);
                                    const uint64_t forms[5][2] = {{K, F * K}, {0, 0}, {K, 0}, {0, K}, {K + 7, F * (K + 7) + 11}};
                                    const uint32_t flags = (n / 2 + hop) % 2 ? BHW_OLA_NORMALIZE : 0;
                                    ++combo;
                                    for (const auto &gf : forms) {
                                        const int rc = checks(&p, L, &sa, &ss, flags, X, G, gf[0], gf[1], O, true);
                                        REQUIRE(rc == BHW_OK, "checks %d n %" PRIu64 " L %" PRIu64 " hop %" PRIu64 " F %" PRIu64, rc, n, L, hop, F);
                                        REQUIRE(real_checks(&p, L, &sa, &ss, flags, X, G, gf[0], gf[1], O, true) == BHW_OK, "the real-gain checks");
                                        const auto pl = plan(&p, L, &sa, &ss, flags, gf[0], gf[1], false);
                                        REQUIRE(pl.g_stride == gf[0] && pl.g_bstride == gf[1], "gain strides");
                                        REQUIRE(pl.cpl <= 8u && pl.lds_bytes <= max_lds && pl.m == n / 2 && pl.lpf >= 1u, "plan of n_fft %" PRIu64, n);
                                        REQUIRE(describe(&p, nullptr, L, &sa, &ss, flags, gf[0], gf[1], line, sizeof line) == BHW_OK, "describe");
                                        REQUIRE(real_describe(&p, nullptr, L, &sa, &ss, flags, gf[0], gf[1], real, sizeof real) == BHW_OK, "describe");
                                        REQUIRE(line[0] == 'c' && strstr(line, kname) && strstr(line, ", complex gains: ") && strlen(line) < sizeof line - 1, "line");
                                        REQUIRE(!strstr(real, "complex gains") && strstr(real, rname) && strlen(line) == strlen(real) + 1 + 1 + 8, "the real line");
                                        REQUIRE(describe(&p, nullptr, L, &sa, &ss, flags, gf[0], gf[1], line, 40) == BHW_OK, "short buffer");
                                        // the replay, where the call is small enough to walk lane by lane
                                        const uint64_t work = nb * F * n;
                                        if (work <= (1u << 8) || (work <= (1u << 15) && (size_t)(&gf - forms) == combo % 5))
                                            replay_gain_reads(pl.m, pl.lpf, nb, F, gf[0], gf[1]);
                                    }
                                    // a gain stride below its bound in pairs; the alignment; out inside x or g, in 8-byte elements
                                    REQUIRE(checks(&p, L, &sa, &ss, flags, X, G, K - 1, 0, O, true) == BHW_ERR_BADARG, "g_stride");
                                    if (F > 1) REQUIRE(checks(&p, L, &sa, &ss, flags, X, G, K, F * K - 1, O, true) == BHW_ERR_BADARG, "g_batch_stride");
                                    REQUIRE(checks(&p, L, &sa, &ss, flags, X, G + 4, 0, 0, O, true) == BHW_ERR_BADARG, "a 4-byte aligned d_g");
                                    REQUIRE(real_checks(&p, L, &sa, &ss, flags, X, G + 4, 0, 0, O, true) == BHW_OK, "the real call takes it");
                                    REQUIRE(checks(&p, L, &sa, &ss, flags, X, G, 0, 0, X + 4 * (Tin - 1), true) == BHW_ERR_BADARG, "x overlap");
                                    REQUIRE(checks(&p, L, &sa, &ss, flags, X, G, 0, 0, G + 4 * K, true) == BHW_ERR_BADARG, "the second half of a gain row");
                                    REQUIRE(real_checks(&p, L, &sa, &ss, flags, X, G, 0, 0, G + 4 * K, true) == BHW_OK, "behind one real gain row");
                                    REQUIRE(checks(&p, L, &sa, &ss, flags, X, G, 0, 0, G + 8 * K - 4, true) == BHW_ERR_BADARG, "the last float of a gain row");
                                    REQUIRE(checks(&p, L, &sa, &ss, flags, X, G, 0, 0, G + 8 * K, true) == BHW_OK, "behind one gain row");
                                    const uint64_t pairs = (nb - 1) * (F * K) + (F - 1) * K + K;
                                    REQUIRE(checks(&p, L, &sa, &ss, flags, X, G, K, F * K, G + 4 * pairs, true) == BHW_ERR_BADARG, "the second half of the gains");
                                    REQUIRE(checks(&p, L, &sa, &ss, flags, X, G, K, F * K, G + 8 * pairs, true) == BHW_OK, "behind the gains");
                                }
    }
}

int main()
{
    std::vector<uint64_t> pow2, mixed;
    for (uint64_t n = 1u << kFftMinLog; n <= (1u << kMaskFftMaxLog); n <<= 1) pow2.push_back(n);
    for (uint64_t n = 1; n <= kMaskMfftMaxN; ++n)
        if (bhwp_mfft_supported(n)) mixed.push_back(n);
    REQUIRE(pow2.size() == 8 && mixed.size() == 73, "%zu + %zu sizes", pow2.size(), mixed.size());
    family("fft", pow2, 40960u, bhwp_cmask_fft_checks, bhwp_mask_fft_checks, bhwp_mask_fft_plan, bhwp_describe_cmask_fft, bhwp_describe_mask_fft);
    family("mfft", mixed, 40000u, bhwp_cmask_mfft_checks, bhwp_mask_mfft_checks, bhwp_mask_mfft_plan, bhwp_describe_cmask_mfft,
           bhwp_describe_mask_mfft);
    REQUIRE(g_odd > 0 && g_even > 0, "M odd %ld, even %ld", g_odd, g_even);
    // the sizes the calls do not take, each naming the other family's complex-gain call where one exists
    bhw_params p;
    REQUIRE(bhw_params_init(&p, BHW_WIN_BH4, 12, 16) == BHW_OK, "params");
    const void *X = (const void *)0x10000000, *G = (const void *)0x4000000000ull, *O = (const void *)0x8000000000ull;
    for (uint64_t n : {8ull, 14ull, 22ull, 400ull, 2000ull, 2160ull, 4050ull, 4096ull, 8192ull}) {
        const bhw_stft s = desc_of(1, 100000, 3, 7, n, 0, n / 2, 0, 0);
        const int rc = bhwp_cmask_fft_checks(&p, 8, &s, &s, 0, X, G, 0, 0, O);
        REQUIRE(rc == BHW_ERR_UNSUPPORTED || (n == 8 && rc != BHW_OK), "n_fft %" PRIu64, n);
        if (n == 400 || n == 2000) REQUIRE(strstr(bhw_last_error(), "bhw_cmask_mfft_f32_*") != nullptr, "%s", bhw_last_error());
    }
    for (uint64_t n : {8ull, 14ull, 22ull, 16ull, 512ull, 2048ull, 2160ull, 2560ull, 4050ull, 4096ull, 8192ull}) {
        const bhw_stft s = desc_of(1, 100000, 3, 7, n, 0, n / 2, 0, 0);
        REQUIRE(bhwp_cmask_mfft_checks(&p, 8, &s, &s, 0, X, G, 0, 0, O) == BHW_ERR_UNSUPPORTED, "n_fft %" PRIu64, n);
        if (n == 16 || n == 512 || n == 2048) REQUIRE(strstr(bhw_last_error(), "bhw_cmask_fft_f32_*") != nullptr, "%s", bhw_last_error());
    }
    printf("ok %ld checks, %ld gain replays\n", g_checks, g_replays);
    return 0;
}
