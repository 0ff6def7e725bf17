// san_beam.cpp -- the planner's part of the fused multichannel filter-and-sum calls of both families (bhw_plan.cpp:
// bhwp_beam_fft_checks / bhwp_beam_mfft_checks, bhwp_beam_fft_plan / _mfft_plan, bhwp_describe_beam_fft / _mfft) swept under
// AddressSanitizer + UBSan over all 8 + 73 supported n_fft against L, hop, batch, frames, the output length and n_ch at the edges (1, 2,
// 3 and BHW_BEAM_MAX_CH channels), both padding rules, centred and not, packed and padded strides and every gain stride form.  Besides
// "no report" it asserts that
//   - the checks pass, and the plan is the complex-gain call's plan for the B output signals, field for field, with the channel axis
//     resolved beside it; at most 8 columns per lane, 40 960 / 40 000 bytes of LDS, and at most 3 values of k <= floor(M / 2) per lane
//     (what the kernels' register sums hold);
//   - the describe line begins "beam", names k_beam_*_direct and says "channels C";
//   - n_ch 0 and BHW_BEAM_MAX_CH + 1, a channel stride below its bound, a zero gain channel stride with two channels, batch strides
//     that do not hold the channels, and a d_out that begins inside the LAST channel of d_x or of d_g are refused;
// and it replays, lane by lane and channel by channel, the sample reads of step a. (mask_fft_row / mask_mfft_row: t = f * hop + j - pad
// under the padding rule, from x + b * x_stride + c * x_ch_stride) and the gain-pair reads of step c. (gp = g + b * g_batch_stride +
// c * g_ch_stride + f * g_stride; pairs k ascending and M - k descending) of BeamSource::frame / BeamMfftSource::frame on float arrays
// of exactly the contract's extents under every stride form: every index inside the extent and never in a gap, every sample under a
// frame's window and every pair 0..M of every channel's row read, with M odd and M even.
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

// The sample reads (step a.) and the gain-pair reads (step c.) of one call, from the plan's resolved strides: x and g are float arrays
// of exactly the contract's extents; ASan holds the accesses to them.
template <typename Plan>
static void replay_reads(const Plan &pl, const bhw_stft &sa, uint64_t L, uint64_t Bn, uint64_t F)
{
    const uint32_t M = pl.m, lpf = pl.lpf, H = M >> 1, n = (uint32_t)sa.n_fft, C = pl.n_ch;
    const uint64_t K = (uint64_t)M + 1, T = sa.samples, gs = pl.g_stride, gcs = pl.g_cstride, gbs = pl.g_bstride;
    const uint64_t xs = pl.in_stride, xcs = pl.x_cstride;
    ++(M & 1u ? g_odd : g_even);
    // the samples
    const uint64_t floats = (Bn - 1) * xs + (C - 1) * xcs + T;
    std::vector<float> x(floats, 1.0f);
    std::vector<uint8_t> xgap(floats, 1), hit(floats, 0);
    for (uint64_t b = 0; b < Bn; ++b)
        for (uint32_t c = 0; c < C; ++c)
            for (uint64_t t = 0; t < T; ++t) xgap[b * xs + c * xcs + t] = 0;
    float sum = 0.0f;
    const bool reflect = sa.pad_mode == BHW_PAD_REFLECT;
    for (uint64_t b = 0; b < Bn; ++b)
        for (uint64_t f = 0; f < F; ++f)
            for (uint32_t c = 0; c < C; ++c) {
                const uint64_t xb = b * xs + c * xcs;                     // x + b * x_stride + c * x_cstride
                const uint64_t t0 = f * sa.hop - sa.pad;                  // the (wrapped) time of column 0
                for (uint32_t l = 0; l < lpf; ++l)
                    for (uint32_t j = l; j < n; j += lpf) {
                        const uint32_t k = j - (uint32_t)sa.col0;
                        if (k >= L) continue;
                        uint64_t t = t0 + j;
                        if (t >= T) {
                            const int64_t ts = (int64_t)t;
                            if (reflect) t = ts < 0 ? (uint64_t)(-ts) : 2 * (T - 1) - t;
                            else t = 0;
                        }
                        REQUIRE(t < T && xb + t < floats && !xgap.at(xb + t), "sample %" PRIu64 " of channel %u of frame %" PRIu64 " outside its channel", t, c, f);
                        sum += x.at(xb + t);
                        hit.at(xb + t) = 1;
                    }
            }
    for (uint64_t i = 0; i < floats; ++i) REQUIRE(!(xgap[i] && hit[i]), "a gap of x was read");
    // the gain pairs
    const uint64_t pairs = (Bn - 1) * gbs + (C - 1) * gcs + (F - 1) * gs + K;
    std::vector<float> g(2 * pairs, 1.0f);
    std::vector<uint8_t> gap(2 * pairs, 1), seen(K);
    const uint64_t nb_rows = gbs ? Bn : 1, f_rows = gs ? F : 1;
    for (uint64_t b = 0; b < nb_rows; ++b)
        for (uint32_t c = 0; c < C; ++c)
            for (uint64_t f = 0; f < f_rows; ++f)
                for (uint64_t k = 0; k < 2 * K; ++k) gap[2 * (b * gbs + c * gcs + f * gs) + k] = 0;
    for (uint64_t b = 0; b < Bn; ++b)
        for (uint64_t f = 0; f < F; ++f)
            for (uint32_t c = 0; c < C; ++c) {
                std::fill(seen.begin(), seen.end(), 0);
                const uint64_t row = b * gbs + c * gcs + f * gs;          // g + b * g_bstride + c * g_cstride + f * g_stride, in pairs
                for (uint32_t l = 0; l < lpf; ++l) {
                    uint32_t owned = 0;
                    for (uint32_t i = 0; i < 3u; ++i) {                   // kMaxK register sums: k = l + i * lpf
                        const uint32_t k = l + i * lpf;
                        if (k > H) continue;
                        ++owned;
                        for (uint64_t q : {(uint64_t)k, (uint64_t)(M - k)})
                            for (uint64_t part = 0; part < 2; ++part) {
                                const uint64_t at = 2 * (row + q) + part;
                                REQUIRE(at < g.size() && !gap.at(at), "float %" PRIu64 " of pair %" PRIu64 " of channel %u of frame %" PRIu64 " outside its row", at, q, c, f);
                                sum += g.at(at);
                            }
                        seen.at(k) = 1;
                        seen.at(M - k) = 1;
                    }
                    uint32_t all = 0;
                    for (uint32_t k = l; k <= H; k += lpf) ++all;
                    REQUIRE(owned == all, "lane %u owns %u values of k, its sums hold %u", l, all, owned);
                }
                for (uint64_t k = 0; k < K; ++k) REQUIRE(seen[k] == 1, "pair %" PRIu64 " not read", k);
            }
    REQUIRE(sum > 0.0f, "reads");
    ++g_replays;
}

template <typename Checks, typename Plan, typename CPlan, typename Describe>
static void family(const char *fam, const std::vector<uint64_t> &sizes, uint32_t max_lds, Checks checks, Plan plan, CPlan cmask_plan,
                   Describe describe)
{
    bhw_params p;
    REQUIRE(bhw_params_init(&p, BHW_WIN_BH4, 12, 16) == BHW_OK, "params");
    char line[1280], kname[64], chans[32];
    snprintf(kname, sizeof kname, "k_beam_%s_direct", fam);
    // addresses that are never dereferenced: the checks only compare them
    const char *X = (const char *)0x10000000, *G = (const char *)0x4000000000ull, *O = (const char *)0x8000000000ull;
    const uint32_t chan_counts[4] = {1u, 2u, 3u, BHW_BEAM_MAX_CH};
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
                                    ++combo;
                                    const uint32_t C = chan_counts[combo % 4];
                                    const bool padded = (n / 2 + F + nb) % 2 == 0;
                                    const uint64_t xcs = padded ? Tin + 3 : 0, xc = xcs ? xcs : Tin;
                                    const bhw_stft sa = desc_of(nb, Tin, F, hop, n, col0, pad, mode, padded ? C * xcs + 2 : 0);
                                    const bhw_stft ss = desc_of(nb, T, F, hop, n, col0, pad, 0, padded ? T + 5 : 0);
                                    bhw_stft sc = sa;                     // the complex-gain call's analysis descriptor: one channel a signal
                                    sc.x_stride = 0;
                                    const uint64_t prow = (F - 1) * (K + 7) + K;
                                    // (g_stride, g_ch_stride, g_batch_stride): full, (C, K), (C, F, K), (B, C, 1, K), padded
                                    const uint64_t forms[5][3] = {{K, F * K, C * F * K}, {0, K, 0}, {K, F * K, 0}, {0, K, C * K},
                                                                  {K + 7, prow + 5, (C - 1) * (prow + 5) + prow + 11}};
                                    const uint32_t flags = (n / 2 + hop) % 2 ? BHW_OLA_NORMALIZE : 0;
                                    snprintf(chans, sizeof chans, ", complex gains: channels %u, ", C);
                                    for (const auto &gf : forms) {
                                        const BhwBeamAxis ch{C, xcs, gf[1]};
                                        const int rc = checks(&p, L, &sa, &ss, flags, X, ch, G, gf[0], gf[2], O, true);
                                        REQUIRE(rc == BHW_OK, "checks %d (%s) n %" PRIu64 " L %" PRIu64 " hop %" PRIu64 " F %" PRIu64 " C %u", rc,
                                                bhw_last_error(), n, L, hop, F, C);
                                        const auto pl = plan(&p, L, &sa, &ss, flags, ch, gf[0], gf[2], false);
                                        const auto cp = cmask_plan(&p, L, &sc, &ss, flags, gf[0], gf[2], false);
                                        REQUIRE(pl.g_stride == gf[0] && pl.g_cstride == gf[1] && pl.g_bstride == gf[2] && pl.n_ch == C, "gain strides");
                                        REQUIRE(pl.x_cstride == xc && pl.in_stride == (padded ? C * xcs + 2 : C * Tin), "input strides");
                                        REQUIRE(pl.cpl <= 8u && pl.lds_bytes <= max_lds && pl.m == n / 2 && pl.lpf >= 1u, "plan of n_fft %" PRIu64, n);
                                        REQUIRE((pl.m >> 1) / pl.lpf + 1u <= 3u, "%u values of k per lane at n_fft %" PRIu64, (pl.m >> 1) / pl.lpf + 1u, n);
                                        REQUIRE(pl.m == cp.m && pl.lpf == cp.lpf && pl.fy == cp.fy && pl.cpl == cp.cpl && pl.lds_bytes == cp.lds_bytes &&
                                                pl.grid == cp.grid && pl.span == cp.span && pl.spans == cp.spans && pl.groups == cp.groups &&
                                                pl.trips == cp.trips && pl.t0 == cp.t0, "the complex-gain plan");
                                        REQUIRE(describe(&p, nullptr, L, &sa, &ss, flags, ch, gf[0], gf[2], line, sizeof line) == BHW_OK, "describe");
                                        REQUIRE(!strncmp(line, "beam ", 5) && strstr(line, kname) && strstr(line, chans) && strlen(line) < sizeof line - 1, "line");
                                        REQUIRE(describe(&p, nullptr, L, &sa, &ss, flags, ch, gf[0], gf[2], line, 40) == BHW_OK, "short buffer");
                                        // the replay, where the call is small enough to walk lane by lane
                                        const uint64_t work = nb * F * n * C;
                                        if (work <= (1u << 9) || (work <= (1u << 16) && (size_t)(&gf - forms) == combo % 5))
                                            replay_reads(pl, sa, L, nb, F);
                                    }
                                    // the channel axis at its bounds
                                    const uint64_t rows = (F - 1) * K + K;
                                    const BhwBeamAxis ok{C, xcs, rows};
                                    REQUIRE(checks(&p, L, &sa, &ss, flags, X, ok, G, K, 0, O, true) == BHW_OK, "%s", bhw_last_error());
                                    for (uint32_t bad : {0u, BHW_BEAM_MAX_CH + 1u})
                                        REQUIRE(checks(&p, L, &sa, &ss, flags, X, BhwBeamAxis{bad, 0, rows}, G, K, 0, O, true) == BHW_ERR_BADARG, "n_ch %u", bad);
                                    REQUIRE(checks(&p, L, &sa, &ss, flags, X, BhwBeamAxis{C, Tin - 1, rows}, G, K, 0, O, true) == BHW_ERR_BADARG || Tin == 1, "x_ch_stride");
                                    if (C > 1) {
                                        REQUIRE(checks(&p, L, &sa, &ss, flags, X, BhwBeamAxis{C, xcs, 0}, G, K, 0, O, true) == BHW_ERR_BADARG, "g_ch_stride 0");
                                        REQUIRE(strstr(bhw_last_error(), "sum of the channels") != nullptr, "%s", bhw_last_error());
                                        REQUIRE(checks(&p, L, &sa, &ss, flags, X, BhwBeamAxis{C, xcs, rows - 1}, G, K, 0, O, true) == BHW_ERR_BADARG, "g_ch_stride");
                                        REQUIRE(checks(&p, L, &sa, &ss, flags, X, ok, G, K, C * rows - 1, O, true) == BHW_ERR_BADARG, "g_batch_stride");
                                        bhw_stft sb = sa;
                                        sb.x_stride = (C - 1) * xc + Tin - 1;
                                        REQUIRE(checks(&p, L, &sb, &ss, flags, X, ok, G, K, 0, O, true) != BHW_OK, "x_stride below the channels");
                                    }
                                    REQUIRE(checks(&p, L, &sa, &ss, flags, X, ok, G + 4, K, 0, O, true) == BHW_ERR_BADARG, "a 4-byte aligned d_g");
                                    // d_out inside the last channel of the last signal of x, and inside the last channel's gains
                                    const uint64_t xlast = (nb - 1) * (sa.x_stride ? sa.x_stride : C * xc) + (C - 1) * xc + Tin - 1;
                                    REQUIRE(checks(&p, L, &sa, &ss, flags, X, ok, G, K, 0, X + 4 * xlast, true) == BHW_ERR_BADARG, "x overlap");
                                    REQUIRE(checks(&p, L, &sa, &ss, flags, X, ok, G, K, 0, X + 4 * (xlast + 1), true) == BHW_OK, "behind x: %s", bhw_last_error());
                                    const uint64_t glast = (C - 1) * rows + rows;
                                    REQUIRE(checks(&p, L, &sa, &ss, flags, X, ok, G, K, 0, G + 8 * glast - 4, true) == BHW_ERR_BADARG, "the last float of the gains");
                                    REQUIRE(checks(&p, L, &sa, &ss, flags, X, ok, G, K, 0, G + 8 * glast, true) == BHW_OK, "behind the gains");
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
    family("fft", pow2, 40960u, bhwp_beam_fft_checks, bhwp_beam_fft_plan, bhwp_mask_fft_plan, bhwp_describe_beam_fft);
    family("mfft", mixed, 40000u, bhwp_beam_mfft_checks, bhwp_beam_mfft_plan, bhwp_mask_mfft_plan, bhwp_describe_beam_mfft);
    REQUIRE(g_odd > 0 && g_even > 0, "M odd %ld, even %ld", g_odd, g_even);
    // the sizes the calls do not take, each naming the other family's call where one exists
    bhw_params p;
    REQUIRE(bhw_params_init(&p, BHW_WIN_BH4, 12, 16) == BHW_OK, "params");
    const void *X = (const void *)0x10000000, *G = (const void *)0x4000000000ull, *O = (const void *)0x8000000000ull;
    const BhwBeamAxis ch{2, 0, 100000};
    for (uint64_t n : {8ull, 14ull, 22ull, 400ull, 2000ull, 2160ull, 4050ull, 4096ull, 8192ull}) {
        const bhw_stft s = desc_of(1, 100000, 3, 7, n, 0, n / 2, 0, 0);
        const int rc = bhwp_beam_fft_checks(&p, 8, &s, &s, 0, X, ch, G, 0, 0, O);
        REQUIRE(rc == BHW_ERR_UNSUPPORTED || (n == 8 && rc != BHW_OK), "n_fft %" PRIu64, n);
        if (n == 400 || n == 2000) REQUIRE(strstr(bhw_last_error(), "bhw_beam_mfft_f32_*") != nullptr, "%s", bhw_last_error());
    }
    for (uint64_t n : {8ull, 14ull, 22ull, 16ull, 512ull, 2048ull, 2160ull, 2560ull, 4050ull, 4096ull, 8192ull}) {
        const bhw_stft s = desc_of(1, 100000, 3, 7, n, 0, n / 2, 0, 0);
        REQUIRE(bhwp_beam_mfft_checks(&p, 8, &s, &s, 0, X, ch, G, 0, 0, O) == BHW_ERR_UNSUPPORTED, "n_fft %" PRIu64, n);
        if (n == 16 || n == 512 || n == 2048) REQUIRE(strstr(bhw_last_error(), "bhw_beam_fft_f32_*") != nullptr, "%s", bhw_last_error());
    }
    printf("ok %ld checks, %ld read replays\n", g_checks, g_replays);
    return 0;
}
