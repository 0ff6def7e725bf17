// san_spectrogram.cpp -- the planner's part of the fused spectrogram calls (bhw_plan.cpp: bhwp_spectrogram_checks /
// bhwp_spectrogram_plan / bhwp_describe_spectrogram) swept under AddressSanitizer + UBSan, and a host replay, lane by lane, of the
// epilogue of bhw_spectrogram.hip:
//   - the idle buffer: after the plan's passes the buffer the epilogue writes the powers to is not the one that holds the
//     transformed points, and the slot's K floats lie inside it and inside the plan's LDS bytes;
//   - power mode: every output column k < K of a live row is written exactly once, inside the row's W floats;
//   - bank mode: every power of the slot is written exactly once before the barrier; after it every output column m < filters is
//     written exactly once, every power read lies inside the slot's K floats and every weight read inside [0, weights) -- for
//     consistent banks (where the sum is also compared with the dense product, bit for bit in binary64) and for deliberately
//     inconsistent ones: offsets that are not ascending or lie past `weights`, `first` at or past K or at the top of uint32.
// The arrays the replay indexes are std::vectors of exactly K and `weights` elements, so an index the asserts missed is ASan's.
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

struct Bank {
    std::vector<uint32_t> first, offset;
    std::vector<float> weight;
    uint32_t filters, weights;          // what the descriptor says
};

static bhw_fbank fbank_of(const Bank &bk, uint32_t bins)
{
    bhw_fbank fb;
    memset(&fb, 0, sizeof fb);
    fb.struct_size = sizeof fb;
    fb.filters = bk.filters;
    fb.bins = bins;
    fb.weights = bk.weights;
    fb.d_first = (const uint32_t *)0x200000000000ull;            // never dereferenced by the planner
    fb.d_offset = (const uint32_t *)0x200000100000ull;
    fb.d_weight = (const float *)0x200000200000ull;
    return fb;
}

// a consistent random bank: bands inside [0, K), some empty, some over all K bins, negative weights too
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
        for (uint32_t i = 0; i < c; ++i) bk.weight.push_back((float)((double)(rnd() >> 11) / 9007199254740992.0 - 0.25));
    }
    bk.weights = bk.offset[filters];
    return bk;
}

// the epilogue of one live slot, every lane in the kernel's order; out has W columns
static void replay_epilogue(const BhwStftFftPlan &pl, const Bank *bk, bool consistent)
{
    const uint32_t M = pl.m, K = M + 1, lpf = pl.lpf, n = 2 * M;
    // the idle buffer of every slot: not src, inside the Stockham buffers
    const uint32_t passes = pl.radix4 + pl.radix2;
    for (uint32_t slot = 0; slot < pl.fy; ++slot) {
        uint64_t src = (uint64_t)slot * M, dst = ((uint64_t)pl.fy + slot) * M;          // in complex64 elements from fft_lds
        for (uint32_t i = 0; i < passes; ++i) std::swap(src, dst);
        const uint64_t idle = ((uint64_t)((passes & 1u) ? 0u : pl.fy) + slot) * M;      // fft_idle_buffer
        REQUIRE(idle == dst && idle != src, "slot %u: idle %" PRIu64 " src %" PRIu64, slot, idle, src);
        REQUIRE(idle * 8u + (uint64_t)K * 4u <= (idle + M) * 8u && (idle + M) * 8u <= 2ull * pl.fy * M * 8u && K <= n, "slot %u: K floats inside", slot);
        REQUIRE(2ull * pl.fy * M * 8u < pl.lds_bytes, "buffers inside the plan's LDS");
    }
    std::vector<double> src_pow(K);
    for (uint32_t k = 0; k < K; ++k) src_pow[k] = (double)(float)((double)(rnd() >> 11) / 9007199254740992.0 * 100.0);
    if (!bk) {
        std::vector<int> hit(K, 0);
        for (uint32_t l = 0; l < lpf; ++l)
            for (uint32_t k = l; k <= M; k += lpf) ++hit.at(k);
        for (uint32_t k = 0; k < K; ++k) REQUIRE(hit[k] == 1, "power column %u written %d times", k, hit[k]);
        return;
    }
    std::vector<float> pw(K);                                                              // exactly K: ASan guards the rest
    std::vector<int> pw_hit(K, 0);
    for (uint32_t l = 0; l < lpf; ++l)
        for (uint32_t k = l; k <= M; k += lpf) {
            pw.at(k) = (float)src_pow[k];
            ++pw_hit[k];
        }
    for (uint32_t k = 0; k < K; ++k) REQUIRE(pw_hit[k] == 1, "power %u staged %d times", k, pw_hit[k]);
    // -- the barrier --
    const uint32_t W = bk->weights;
    REQUIRE(bk->weight.size() == W, "the weight array holds `weights` floats");
    std::vector<int> hit(bk->filters, 0);
    std::vector<float> out(bk->filters, -1.0f);
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
            out.at(m) = (float)acc;
            ++hit[m];
        }
    for (uint32_t m = 0; m < bk->filters; ++m) REQUIRE(hit[m] == 1, "bank column %u written %d times", m, hit[m]);
    if (consistent)
        for (uint32_t m = 0; m < bk->filters; ++m) {
            double acc = 0.0;                                                             // the contract: ascending i, binary64, from +0.0
            for (uint32_t i = bk->offset[m]; i < bk->offset[m + 1]; ++i) acc += (double)pw[bk->first[m] + (i - bk->offset[m])] * (double)bk->weight[i];
            const float want = (float)acc;
            REQUIRE(memcmp(&want, &out[m], 4) == 0 && !(bk->offset[m] == bk->offset[m + 1] && (out[m] != 0.0f || std::signbit(out[m]))),
                    "filter %u: %a != %a", m, out[m], want);
        }
}

int main()
{
    char buf[1100];
    long replays = 0, bad_banks = 0;
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 12, 24);
    const uint64_t xa = 0x10000000ull, ya = 0x100000000000ull;
    for (uint32_t lg = kFftMinLog; lg <= kFftMaxLog; ++lg) {
        const uint64_t n = 1ull << lg;
        const uint32_t K = (uint32_t)(n / 2 + 1);
        for (uint32_t filters : {0u, 1u, 3u, 10u, 80u, K - 1u, K, K + 7u, 4096u}) {
            Bank bk;
            if (filters) bk = consistent_bank(K, filters);
            const Bank *bp = filters ? &bk : nullptr;
            const uint64_t W = filters ? filters : K;
            for (uint64_t L : {(uint64_t)13, n})
                for (uint64_t hop : {(uint64_t)7, n + 5})
                    for (uint64_t B : {1ull, 3ull})
                        for (uint64_t F : {1ull, 65ull, 257ull})
                            for (int framing = 0; framing < 3; ++framing)           // 0 Welch + detrend, 1 Welch, 2 centred reflect
                                for (int padded = 0; padded <= 1; ++padded) {
                                    const bool centred = framing >= 2;
                                    const uint64_t pad = centred ? n / 2 : 0, col0 = centred ? (n - L) / 2 : 0;
                                    const uint64_t reach = centred ? n : L;
                                    uint64_t T = (F - 1) * hop + reach;
                                    T = T > 2 * pad ? T - 2 * pad : 1;
                                    if (centred && (T + 2 * pad < (F - 1) * hop + n || pad > T - 1)) continue;
                                    const uint32_t flags = framing == 0 ? BHW_WELCH_DETREND_CONSTANT : 0u;
                                    bhw_stft s = desc_of(B, T, F, hop, n, col0, pad, framing == 2 ? BHW_PAD_REFLECT : BHW_PAD_CONSTANT);
                                    if (padded) {
                                        s.x_stride = T + 3;
                                        s.y_stride = W + 5;                                    // odd: no evenness rule
                                        s.y_batch_stride = F * s.y_stride + 9;
                                    }
                                    bhw_fbank fb = fbank_of(bk, K);
                                    const bhw_fbank *f = filters ? &fb : nullptr;
                                    int rc = bhwp_spectrogram_checks(&p, L, &s, flags, f, nullptr, nullptr, false);
                                    REQUIRE(rc == BHW_OK, "checks rc %d: n %" PRIu64 " L %" PRIu64 " hop %" PRIu64 " B %" PRIu64 " F %" PRIu64 " framing %d filters %u: %s", rc, n, L, hop, B, F, framing, filters, bhw_last_error());
                                    REQUIRE(bhwp_spectrogram_checks(&p, L, &s, flags, f, (const void *)xa, (const void *)ya) == BHW_OK, "pointer checks");
                                    REQUIRE(bhwp_spectrogram_checks(&p, L, &s, flags, f, (const void *)xa, (const void *)(ya + 4)) == BHW_OK, "4-byte aligned P");
                                    REQUIRE(bhwp_spectrogram_checks(&p, L, &s, flags, f, (const void *)xa, (const void *)(ya + 2)) == BHW_ERR_BADARG, "misaligned P");
                                    REQUIRE(bhwp_spectrogram_checks(&p, L, &s, flags, f, (const void *)ya, (const void *)ya) == BHW_ERR_BADARG, "overlap");
                                    REQUIRE(bhwp_spectrogram_checks(&p, L, &s, flags | 2u, f, nullptr, nullptr, false) == BHW_ERR_BADARG, "flags");
                                    const BhwStftFftPlan pl = bhwp_spectrogram_plan(&p, L, &s, flags, f, (B + F) % 2 == 0);
                                    const BhwStftFftPlan fw = bhwp_stft_fft_plan(&p, L, &s, flags, (B + F) % 2 == 0);
                                    REQUIRE(pl.lpf == fw.lpf && pl.fy == fw.fy && pl.cpl == fw.cpl && pl.radix4 == fw.radix4 && pl.radix2 == fw.radix2 &&
                                            pl.groups == fw.groups && pl.grid == fw.grid && pl.lds_bytes == fw.lds_bytes && pl.rows == fw.rows, "the forward plan");
                                    REQUIRE(pl.y_stride == (padded ? W + 5 : W) && pl.y_bstride == (padded ? F * (W + 5) + 9 : F * W), "strides");
                                    REQUIRE(bhwp_describe_spectrogram(&p, nullptr, L, &s, flags, f, buf, sizeof buf) == BHW_OK && strlen(buf) > 40, "describe");
                                    REQUIRE(strstr(buf, filters ? "bank mode" : "power mode") != nullptr, "mode in %s", buf);
                                    bhw_stft bad = s;
                                    bad.y_stride = W - 1;
                                    if (W > 1) REQUIRE(bhwp_spectrogram_checks(&p, L, &bad, flags, f, nullptr, nullptr, false) == BHW_ERR_BADARG, "short y_stride");
                                    bad = s;
                                    bad.y_batch_stride = (F - 1) * (s.y_stride ? s.y_stride : W) + W - 1;
                                    if (bad.y_batch_stride) REQUIRE(bhwp_spectrogram_checks(&p, L, &bad, flags, f, nullptr, nullptr, false) == BHW_ERR_BADARG, "short y_batch_stride");
                                    bad = s;
                                    bad.channels = 2;
                                    bad.x_stride = 0;
                                    REQUIRE(bhwp_spectrogram_checks(&p, L, &bad, flags, f, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED, "channels");
                                    bad = s;
                                    bad.frames = 0;
                                    REQUIRE(bhwp_spectrogram_checks(&p, L, &bad, flags, f, nullptr, nullptr) == BHW_OK, "frames 0");
                                    REQUIRE(bhwp_describe_spectrogram(&p, nullptr, L, &bad, flags, f, buf, sizeof buf) == BHW_OK, "describe frames 0");
                                    if (L == n && hop == 7 && B == 1 && F == 65 && !padded) {
                                        replay_epilogue(pl, bp, true);
                                        ++replays;
                                    }
                                }
            if (!filters) continue;
            // the bank's own refusals
            bhw_stft s = desc_of(2, 20 * n, 3, n, n, 0, 0, 0);
            bhw_fbank fb = fbank_of(bk, K);
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &fb, (const void *)xa, (const void *)ya) == BHW_OK, "bank accepted");
            bhw_fbank b2 = fb;
            b2.struct_size = 40;
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_ERR_BADARG, "struct_size");
            b2 = fb, b2.reserved = 1;
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_ERR_BADARG, "reserved");
            b2 = fb, b2.filters = 0;
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_ERR_BADARG, "filters 0");
            b2 = fb, b2.filters = 4097;
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_ERR_BADARG, "filters 4097");
            b2 = fb, b2.bins = K - 1;
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_ERR_BADARG, "bins");
            b2 = fb, b2.weights = (1u << 24) + 1u;
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_ERR_BADARG, "weights");
            b2 = fb, b2.weights = 1u << 24;
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_OK, "2^24 weights");
            b2 = fb, b2.d_first = nullptr;
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_ERR_BADARG, "NULL d_first");
            b2 = fb, b2.d_offset = nullptr;
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_ERR_BADARG, "NULL d_offset");
            b2 = fb, b2.d_weight = nullptr;
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == (fb.weights ? BHW_ERR_BADARG : BHW_OK), "NULL d_weight");
            b2.weights = 0;
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_OK, "NULL d_weight with no weights");
            b2 = fb, b2.d_first = (const uint32_t *)((uintptr_t)fb.d_first + 2);
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_ERR_BADARG, "misaligned d_first");
            b2 = fb, b2.d_offset = (const uint32_t *)((uintptr_t)fb.d_offset + 1);
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_ERR_BADARG, "misaligned d_offset");
            b2 = fb, b2.d_weight = (const float *)((uintptr_t)fb.d_weight + 2);
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_ERR_BADARG, "misaligned d_weight");
            // the last byte of each array on the first of P, and the first byte behind P
            const uint64_t pbytes = 2ull * 3 * filters * 4;
            b2 = fb, b2.d_first = (const uint32_t *)(ya - 4ull * filters + 4);
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_ERR_BADARG, "d_first overlaps P");
            b2.d_first = (const uint32_t *)(ya - 4ull * filters);
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_OK, "d_first ends at P");
            b2 = fb, b2.d_offset = (const uint32_t *)(ya + pbytes - 4);
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_ERR_BADARG, "d_offset overlaps P");
            b2.d_offset = (const uint32_t *)(ya + pbytes);
            REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_OK, "d_offset behind P");
            if (fb.weights) {
                b2 = fb, b2.d_weight = (const float *)(ya + 8);
                REQUIRE(bhwp_spectrogram_checks(&p, n, &s, 0, &b2, (const void *)xa, (const void *)ya) == BHW_ERR_BADARG, "d_weight overlaps P");
            }
            // the element cap with W: 2^20 signals x 4 frames x 4096 filters = 2^34 passes, one more filter column does not exist; 8 frames do not pass
            {
                bhw_stft big = desc_of(1ull << 20, 8 * n, 4, n, n, 0, 0, 0);
                bhw_fbank bf = fb;
                bf.filters = 4096;
                REQUIRE(bhwp_spectrogram_checks(&p, n, &big, 0, &bf, nullptr, nullptr, false) == BHW_OK, "cap reached: %s", bhw_last_error());
                big.frames = 8;
                REQUIRE(bhwp_spectrogram_checks(&p, n, &big, 0, &bf, nullptr, nullptr, false) == BHW_ERR_BADARG, "cap");
            }
            // deliberately inconsistent banks: the replay alone (never a GPU)
            const BhwStftFftPlan pl = bhwp_spectrogram_plan(&p, n, &s, 0, &fb, false);
            for (int kind = 0; kind < 6; ++kind) {
                Bank bad = bk;
                for (uint32_t m = 0; m < filters; ++m) {
                    if (kind == 0) bad.offset[m + 1] = (uint32_t)rnd();                              // anything
                    if (kind == 1 && m % 2) std::swap(bad.offset[m], bad.offset[m + 1]);            // not ascending
                    if (kind == 2) bad.offset[m + 1] = bad.offset[m + 1] + bk.weights + 1u;          // past weights
                    if (kind == 3) bad.first[m] = K + (uint32_t)(rnd() % 5);                         // at or past K
                    if (kind == 4) bad.first[m] = 0xFFFFFFFFu - (uint32_t)(rnd() % 3);               // the top of uint32
                    if (kind == 5) bad.first[m] = K - 1, bad.offset[m] = 0, bad.offset[m + 1] = bk.weights;   // every band runs off the row
                }
                replay_epilogue(pl, &bad, false);
                ++bad_banks;
            }
            {   // a descriptor that claims fewer weights than the offsets reach: the clamp holds the reads inside the claim
                Bank bad = bk;
                bad.weights = bk.weights / 2;
                bad.weight.resize(bad.weights);
                replay_epilogue(pl, &bad, false);
                ++bad_banks;
            }
        }
    }
    REQUIRE(bhwp_spectrogram_checks(&p, 16, nullptr, 0, nullptr, nullptr, nullptr, false) == BHW_ERR_BADARG, "NULL descriptor");
    for (uint64_t n : {8ull, 48ull, 1000ull, 8192ull}) {
        bhw_stft s = desc_of(1, 1ull << 33, 2, 1, n, 0, 0, 0);
        REQUIRE(bhwp_spectrogram_checks(&p, 1, &s, 0, nullptr, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED, "n_fft %" PRIu64, n);
    }
    REQUIRE(replays >= 9 * 9 && bad_banks >= 9 * 8 * 7, "replays %ld %ld", replays, bad_banks);
    printf("ok %ld checks, %ld epilogue replays, %ld inconsistent banks\n", g_checks, replays, bad_banks);
    return 0;
}
