// san_mask_iq.cpp -- the planner's part of the fused STFT + gain + inverse STFT calls for I/Q input (bhw_plan.cpp:
// bhwp_[c]mask_cfft_checks / bhwp_[c]mask_cmfft_checks, bhwp_mask_cfft_plan / bhwp_mask_cmfft_plan, bhwp_describe_[c]mask_c[m]fft)
// swept under AddressSanitizer + UBSan over all 8 + 91 supported n_fft against L, hop, batch, frames and the output length at the
// edges, both padding rules, centred and not, packed, padded and odd strides, both gain types, every gain stride form and both values
// of the shift flag.  Besides "no report" it asserts that
//   - the plan is the inverse I/Q parent's for the synthesis descriptor, field for field, but for the LDS (one more table of n / 2
//     entries for a power of two, the parent's bytes for a mixed-radix size), at most 8 columns per lane;
//   - the describe line names the kernel of the gain type, "forward + inverse FFT" and the state of the gain columns;
//   - a d_out that begins inside the second half of d_x's last complex sample is refused, one that begins behind it is not;
// and it replays, lane by lane, on FLOAT arrays of exactly the contract's size,
//   a. the sample reads of MaskCfftSourceT::frame / MaskCmfftSourceT::frame (step a.): floats 2 t and 2 t + 1 of signal b, as one 8-byte
//      access or as two 4-byte ones, under reflection at both ends and under zero padding (where no value is formed: nothing is
//      read), with T below the pad where the checks allow it; every float of a signal under a window is read, never one in a gap;
//   c. the gain reads (step c.): column k, or (k + n / 2) mod n under the shift (a mask for a power of two, a compare and a subtract
//      otherwise), as 4-byte words or 8-byte pairs, under every stride form, n_fft odd and even: every index inside the extent and
//      never in a gap, every column of a row read exactly once.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "bhw_plan.h"

static long g_checks = 0, g_sample_replays = 0, g_gain_replays = 0, g_odd = 0, g_even = 0, g_vec = 0, g_scalar = 0, g_reflected = 0;
#define REQUIRE(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static bhw_stft desc_of(uint64_t B, uint64_t T, uint64_t frames, uint64_t hop, uint64_t n_fft, uint64_t col0, uint64_t pad, uint32_t pad_mode,
                        uint64_t x_stride)
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
    s.pad_mode = pad_mode;
    s.x_stride = x_stride;
    s.shift = 15;
    return s;
}

static bool pow2(uint64_t n) { return n && !(n & (n - 1)); }

// a. The sample reads of every frame of every signal: x is a float array of exactly (B - 1) * x_stride + 2 * T floats.
static void replay_sample_reads(uint32_t n, uint32_t lpf, uint32_t col0, uint32_t L, const bhw_stft &sa, uint64_t in_stride, bool vec)
{
    const uint64_t T = sa.samples, Bn = sa.batch, floats = (Bn - 1) * in_stride + 2 * T;
    std::vector<float> x(floats, 1.0f);
    std::vector<uint8_t> gap(floats, 1), read(floats, 0);
    for (uint64_t b = 0; b < Bn; ++b)
        for (uint64_t t = 0; t < 2 * T; ++t) gap[b * in_stride + t] = 0;
    ++(vec ? g_vec : g_scalar);
    float sum = 0.0f;
    for (uint64_t b = 0; b < Bn; ++b)
        for (uint64_t f = 0; f < sa.frames; ++f) {
            const float *xb = x.data() + b * in_stride;
            const uint64_t t0 = f * sa.hop - sa.pad;                      // the (wrapped) time of column 0
            for (uint32_t l = 0; l < lpf; ++l)
                for (uint32_t j = l; j < n; j += lpf) {
                    const uint32_t k = j - col0;
                    if (!(k < L)) continue;                               // a value is formed only for window columns
                    uint64_t t = t0 + j;
                    bool zero = false;
                    if (t >= T) {
                        const int64_t ts = (int64_t)t;
                        if (sa.pad_mode == BHW_PAD_REFLECT) {
                            t = ts < 0 ? (uint64_t)(-ts) : 2 * (T - 1) - t;
                            ++g_reflected;
                        } else {
                            t = 0;
                            zero = true;
                        }
                    }
                    REQUIRE(t < T, "sample %" PRIu64 " of %" PRIu64 " (frame %" PRIu64 ", column %u)", t, T, f, j);
                    const float *px = xb + 2 * t;
                    const uint64_t at = (uint64_t)(px - x.data());
                    REQUIRE(at + 1 < floats && !gap[at] && !gap[at + 1], "floats %" PRIu64 ", %" PRIu64 " of %" PRIu64, at, at + 1, floats);
                    if (vec) {
                        REQUIRE(at % 2 == 0, "an 8-byte load at float %" PRIu64, at);   // (the array begins on the 8-byte grid here)
                        float pair[2];
                        memcpy(pair, px, 8);
                        sum += zero ? 0.0f : pair[0] + pair[1];
                    } else {
                        sum += zero ? 0.0f : px[0] + px[1];
                    }
                    if (!zero) read[at] = read[at + 1] = 1;
                }
        }
    // every sample under a window of some frame is read at least once: with hop <= L and frames covering the signal, all of them
    if (sa.hop <= L && sa.pad >= col0 && (sa.frames - 1) * sa.hop + col0 + L >= T + sa.pad) {
        for (uint64_t b = 0; b < Bn; ++b)
            for (uint64_t t = 0; t < 2 * T; ++t) REQUIRE(read[b * in_stride + t], "float %" PRIu64 " of signal %" PRIu64 " never read", t, b);
    }
    REQUIRE(sum == sum, "NaN");
    ++g_sample_replays;
}

// c. The gain reads of every frame: g is an array of exactly (B - 1) * gbs + (F - 1) * gs + n elements of `elem` floats.
static void replay_gain_reads(uint32_t n, uint32_t lpf, uint64_t Bn, uint64_t F, uint64_t gs, uint64_t gbs, uint32_t elem, bool shifted)
{
    const uint64_t K = n, count = (Bn - 1) * gbs + (F - 1) * gs + K;
    std::vector<float> g(elem * count, 1.0f);
    std::vector<uint8_t> gap(count, 1), seen(K);
    const uint64_t nb_rows = gbs ? Bn : 1, f_rows = gs ? F : 1;
    for (uint64_t b = 0; b < nb_rows; ++b)
        for (uint64_t f = 0; f < f_rows; ++f)
            for (uint64_t k = 0; k < K; ++k) gap[b * gbs + f * gs + k] = 0;
    ++(n & 1u ? g_odd : g_even);
    const uint32_t turn = shifted ? n >> 1 : 0u;
    float sum = 0.0f;
    for (uint64_t b = 0; b < Bn; ++b)
        for (uint64_t f = 0; f < F; ++f) {
            const uint64_t row = b * gbs + f * gs;
            std::fill(seen.begin(), seen.end(), 0);
            for (uint32_t l = 0; l < lpf; ++l)
                for (uint32_t k = l; k < n; k += lpf) {
                    uint32_t col;
                    if (pow2(n)) col = (k + turn) & (n - 1u);             // bhw_mask_cfft.hip
                    else {                                                // bhw_mask_cmfft.hip
                        col = k + turn;
                        col = col >= n ? col - n : col;
                    }
                    REQUIRE(col < n && col == (k + (shifted ? n / 2 : 0)) % n, "column %u of bin %u", col, k);
                    const uint64_t at = row + col;
                    REQUIRE(at < count && !gap[at], "gain %" PRIu64 " of %" PRIu64, at, count);
                    for (uint32_t e = 0; e < elem; ++e) sum += g[elem * at + e];
                    REQUIRE(!seen[col], "column %u read twice", col);
                    seen[col] = 1;
                }
            for (uint64_t k = 0; k < K; ++k) REQUIRE(seen[k], "column %" PRIu64 " not read", k);
        }
    REQUIRE(sum > 0.0f, "sum");
    ++g_gain_replays;
}

typedef int (*checks_fn)(const bhw_params *, uint64_t, const bhw_stft *, const bhw_stft *, uint32_t, const void *, const void *, uint64_t, uint64_t,
                         const void *, bool);
typedef int (*describe_fn)(const bhw_params *, const BhwCordicCfg *, uint64_t, const bhw_stft *, const bhw_stft *, uint32_t, uint64_t, uint64_t,
                           char *, uint64_t);

static bool supported_mixed(uint64_t n)
{
    if (n < 18 || n > 2047 || pow2(n)) return false;
    for (uint64_t r : {2ull, 3ull, 5ull})
        while (n % r == 0) n /= r;
    return n == 1;
}

int main()
{
    bhw_params p;
    REQUIRE(bhw_params_init(&p, BHW_WIN_BH4, 12, 16) == BHW_OK, "params");
    std::vector<uint32_t> sizes;
    for (uint32_t n = 16; n <= 2048; ++n)
        if ((pow2(n) && n >= 16) || supported_mixed(n)) sizes.push_back(n);
    REQUIRE(sizes.size() == 99, "%zu sizes", sizes.size());
    char line[1280], parent[1280];
    long plans = 0;
    uint32_t worst_lds[2] = {0, 0};
    for (uint32_t n : sizes) {
        const bool mixed = !pow2(n);
        for (uint32_t L : {1u, 13u, n / 2 + 1, n}) {
            if (L > n) continue;
            for (uint64_t hop : {(uint64_t)1, (uint64_t)7, (uint64_t)n / 4 + 3, (uint64_t)n + 5})
                for (int center = 0; center < 2; ++center) {
                    if (!center && L < n) continue;                       // (refused in Python; the C calls take it, the sweep stays with the users' shapes)
                    for (uint64_t F : {(uint64_t)1, (uint64_t)2, (uint64_t)9}) {
                        const uint64_t pad = center ? n / 2 : 0, col0 = (n - L) / 2, Bn = F == 9 ? 3 : 2;
                        const uint64_t Tin = n + hop * (F - 1) - 2 * pad;
                        if (Tin < 1) continue;
                        for (int64_t extra : {(int64_t)0, (int64_t)-3, (int64_t)40}) {
                            if ((int64_t)Tin + extra < 1) continue;
                            const uint64_t T = (uint64_t)((int64_t)Tin + extra);
                            for (uint32_t mode : {BHW_PAD_CONSTANT, BHW_PAD_REFLECT}) {
                                if (mode == BHW_PAD_REFLECT && pad >= Tin) continue;     // reflection needs pad < T (the checks say so below)
                                for (int stride_form = 0; stride_form < 3; ++stride_form) {
                                    const uint64_t xs = stride_form == 0 ? 0 : stride_form == 1 ? 2 * Tin + 6 : 2 * Tin + 3;
                                    const uint64_t os = stride_form == 0 ? 0 : stride_form == 1 ? 2 * T + 10 : 2 * T + 5;
                                    const bhw_stft sa = desc_of(Bn, Tin, F, hop, n, col0, pad, mode, xs);
                                    const bhw_stft ss = desc_of(Bn, T, F, hop, n, col0, pad, 0, os);
                                    const uint64_t forms[5][2] = {{n, F * n}, {0, 0}, {n, 0}, {0, n}, {n + 7ull, (F - 1) * (n + 7ull) + n + 11}};
                                    for (int pairs = 0; pairs < 2; ++pairs)
                                        for (int sh = 0; sh < 2; ++sh) {
                                            const int form = (int)((plans + pairs + sh) % 5);
                                            const uint64_t gs = forms[form][0], gbs = forms[form][1];
                                            const uint32_t flags = (uint32_t)(BHW_OLA_NORMALIZE | (sh ? BHW_CFFT_SHIFT : 0));
                                            const checks_fn checks = mixed ? (pairs ? bhwp_cmask_cmfft_checks : bhwp_mask_cmfft_checks)
                                                                           : (pairs ? bhwp_cmask_cfft_checks : bhwp_mask_cfft_checks);
                                            const describe_fn describe = mixed ? (pairs ? bhwp_describe_cmask_cmfft : bhwp_describe_mask_cmfft)
                                                                               : (pairs ? bhwp_describe_cmask_cfft : bhwp_describe_mask_cfft);
                                            int rc = checks(&p, L, &sa, &ss, flags, nullptr, nullptr, gs, gbs, nullptr, false);
                                            REQUIRE(rc == BHW_OK, "n %u L %u hop %" PRIu64 " F %" PRIu64 ": %s", n, L, hop, F, bhw_last_error());
                                            // the pointers: out inside the second half of x's last complex sample, and right behind it
                                            const uint64_t in_stride = xs ? xs : 2 * Tin, xfloats = (Bn - 1) * in_stride + 2 * Tin;
                                            const uintptr_t x0 = 0x10000000u, g0 = 0x40000000u;
                                            rc = checks(&p, L, &sa, &ss, flags, (const void *)x0, (const void *)g0, gs, gbs,
                                                        (const void *)(x0 + 4 * xfloats - 4), true);
                                            REQUIRE(rc == BHW_ERR_BADARG && strstr(bhw_last_error(), "d_x and d_out overlap"), "%s", bhw_last_error());
                                            rc = checks(&p, L, &sa, &ss, flags, (const void *)x0, (const void *)g0, gs, gbs,
                                                        (const void *)(x0 + 4 * xfloats), true);
                                            REQUIRE(rc == BHW_OK, "%s", bhw_last_error());
                                            uint32_t lpf, fy, cpl, lds, parent_lds;
                                            if (mixed) {
                                                const BhwMaskCmfftPlan pl = bhwp_mask_cmfft_plan(&p, L, &sa, &ss, flags, gs, gbs, false);
                                                const BhwIstftCmfftPlan ip = bhwp_istft_cmfft_plan(&p, L, &ss, flags, false);
                                                REQUIRE(pl.n == ip.n && pl.fold == ip.fold && pl.lpf == ip.lpf && pl.fy == ip.fy && pl.cpl == ip.cpl &&
                                                        pl.passes == ip.passes && !memcmp(pl.radix, ip.radix, sizeof ip.radix) && pl.span == ip.span &&
                                                        pl.spans == ip.spans && pl.groups == ip.groups && pl.trips == ip.trips && pl.grid == ip.grid &&
                                                        pl.t0 == ip.t0 && pl.hop == ip.hop && pl.x_stride == ip.x_stride && pl.shifted == (sh != 0),
                                                        "plan n %u", n);
                                                REQUIRE(pl.in_stride == in_stride && pl.g_stride == gs && pl.g_bstride == gbs, "strides");
                                                lpf = pl.lpf, fy = pl.fy, cpl = pl.cpl, lds = pl.lds_bytes, parent_lds = ip.lds_bytes;
                                                REQUIRE(lds == parent_lds, "lds %u %u", lds, parent_lds);
                                            } else {
                                                const BhwMaskCfftPlan pl = bhwp_mask_cfft_plan(&p, L, &sa, &ss, flags, gs, gbs, false);
                                                const BhwIstftCfftPlan ip = bhwp_istft_cfft_plan(&p, L, &ss, flags, false);
                                                REQUIRE(pl.n == ip.n && pl.lpf == ip.lpf && pl.fy == ip.fy && pl.cpl == ip.cpl && pl.radix4 == ip.radix4 &&
                                                        pl.radix2 == ip.radix2 && pl.span == ip.span && pl.spans == ip.spans && pl.groups == ip.groups &&
                                                        pl.trips == ip.trips && pl.grid == ip.grid && pl.t0 == ip.t0 && pl.hop == ip.hop &&
                                                        pl.x_stride == ip.x_stride && pl.shifted == (sh != 0), "plan n %u", n);
                                                REQUIRE(pl.in_stride == in_stride && pl.g_stride == gs && pl.g_bstride == gbs, "strides");
                                                lpf = pl.lpf, fy = pl.fy, cpl = pl.cpl, lds = pl.lds_bytes, parent_lds = ip.lds_bytes;
                                                REQUIRE(lds == parent_lds + n / 2 * 8 && lds == 2 * fy * n * 8 + n * 8 + n * 4, "lds %u %u", lds, parent_lds);
                                            }
                                            REQUIRE(cpl <= kCfftMaxCpl && lpf * fy == 256 && (uint64_t)cpl * lpf >= n && lds <= 57344, "lanes n %u", n);
                                            if (lds > worst_lds[mixed]) worst_lds[mixed] = lds;
                                            rc = describe(&p, nullptr, L, &sa, &ss, flags, gs, gbs, line, sizeof line);
                                            REQUIRE(rc == BHW_OK, "%s", bhw_last_error());
                                            const std::string kernel = std::string(pairs ? "k_cmask_" : "k_mask_") + (mixed ? "cmfft" : "cfft") + "_direct<";
                                            REQUIRE(strstr(line, kernel.c_str()) && strstr(line, ", forward + inverse FFT, ") &&
                                                    strstr(line, sh ? ", gain columns shifted, " : ", gain columns in order, ") &&
                                                    (strstr(line, ", complex gains: ") != nullptr) == (pairs != 0), "%s", line);
                                            rc = mixed ? bhwp_describe_istft_cmfft(&p, nullptr, L, &ss, flags, parent, sizeof parent)
                                                       : bhwp_describe_istft_cfft(&p, nullptr, L, &ss, flags, parent, sizeof parent);
                                            REQUIRE(rc == BHW_OK, "%s", bhw_last_error());
                                            const char *a = strstr(line, " signals x "), *b = strstr(parent, " signals x ");
                                            const char *al = a ? strstr(a, " lanes, ") : nullptr, *bl = b ? strstr(b, " lanes, ") : nullptr;
                                            REQUIRE(a && b && al && bl && (al - a) == (bl - b) && !strncmp(a, b, (size_t)(al - a)), "%s | %s", line, parent);
                                            ++plans;
                                            // the replays, on the small sizes and on each size's first shape (they are lane loops over every frame)
                                            if (n <= 100 || (L == n && hop == 7 && F == 2 && extra == 0)) {
                                                const bool vec = in_stride % 2 == 0;  // (iq_vec: an 8-byte aligned base and an even stride)
                                                replay_sample_reads(n, lpf, (uint32_t)col0, L, sa, in_stride, vec);
                                                replay_gain_reads(n, lpf, Bn, F, gs, gbs, pairs ? 2u : 1u, sh != 0);
                                            }
                                        }
                                }
                            }
                        }
                    }
                }
        }
    }
    REQUIRE(worst_lds[0] == 57344 && worst_lds[1] == 56700, "lds %u %u", worst_lds[0], worst_lds[1]);
    REQUIRE(g_odd > 100 && g_even > 100 && g_vec > 100 && g_scalar > 100 && g_reflected > 1000, "coverage %ld %ld %ld %ld %ld", g_odd, g_even,
            g_vec, g_scalar, g_reflected);
    // T below the pad under zero padding: every padded column stands for +0.0 and nothing outside the signal is read
    {
        const uint32_t n = 64;
        const bhw_stft sa = desc_of(2, 20, 6, 4, n, 0, 32, BHW_PAD_CONSTANT, 0), ss = desc_of(2, 110, 6, 4, n, 0, 32, 0, 0);
        REQUIRE(bhwp_mask_cfft_checks(&p, n, &sa, &ss, 1, nullptr, nullptr, 0, 0, nullptr, false) == BHW_OK, "%s", bhw_last_error());
        const BhwMaskCfftPlan pl = bhwp_mask_cfft_plan(&p, n, &sa, &ss, 1, 0, 0, false);
        replay_sample_reads(n, pl.lpf, 0, n, sa, pl.in_stride, true);
        const bhw_stft sr = desc_of(2, 20, 6, 4, n, 0, 32, BHW_PAD_REFLECT, 0);
        REQUIRE(bhwp_mask_cfft_checks(&p, n, &sr, &ss, 1, nullptr, nullptr, 0, 0, nullptr, false) == BHW_ERR_BADARG, "reflection with T below the pad");
    }
    printf("ok %ld checks, %ld plans, %ld sample replays (%ld 8-byte, %ld 4-byte, %ld reflected reads), %ld gain replays (%ld odd n_fft, %ld even)\n",
           g_checks, plans, g_sample_replays, g_vec, g_scalar, g_reflected, g_gain_replays, g_odd, g_even);
    return 0;
}
