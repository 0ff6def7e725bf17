// san_mask_mfft.cpp -- the planner's part of the mixed-radix fused STFT + mask + inverse STFT calls (bhw_plan.cpp:
// bhwp_mask_mfft_checks / bhwp_mask_mfft_plan / bhwp_describe_mask_mfft) swept under AddressSanitizer + UBSan over all 73 supported
// n_fft against L, hop, batch, frames and the output length at the edges, both padding rules, centred and not, packed and padded
// strides and every gain stride form.  Besides "no report" it asserts that the plan is bhwp_istft_mfft_plan of the synthesis
// descriptor field for field but for the LDS bytes (two twiddle tables, within 40 000 bytes, at most 8 columns per lane), and replays on
// the host, lane by lane, the index arithmetic that is new in bhw_mask_mfft.hip (MaskMfftSource::frame) on arrays of exactly the
// contract's sizes:
//   - the frame load: every column of the slot's row written once, by one lane; every sample index inside [0, T) of its signal and
//     inside x's extent, under both padding rules; the window index inside v[0..L);
//   - the forward passes in the plan's schedule: every butterfly's reads inside the M points, every point of the other buffer written
//     once per pass, every twiddle index below n_fft, and the float i mod Ns (one multiply by a reciprocal that may be an ulp off
//     either way) equal to the integer one;
//   - the gain reads: the lanes of k <= floor(M / 2) read g[k] and g[M - k], every bin 0..M of the row's gains read, every index
//     inside g's extent and never in a gap of the strides, under every stride form;
//   - the buffers: which of the slot's two Stockham buffers each phase reads and writes, for either parity of the pass count.  No
//     phase writes the buffer it reads, the split writes every point Z[0..M) of the other buffer once, M odd (no self-mirrored bin)
//     and M even, and the inverse passes end where the ring reads;
//   - the span walk, the ring with its stepped base mod n_fft and its missing last column, and the flush as the kernel runs them with
//     this source: every output (b, t) stored exactly once, inside out's extent and never in a gap.
// The replay is a copy of the kernel's index arithmetic kept in step by hand (only bhwp_istft_span is shared code): a change of the
// frame load, the gain reads or the buffer order in bhw_mask_mfft.hip, of mfft_pass in bhw_stft_mfft.h or of the ring in
// bhw_istft_mfft.h has to be made here as well.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "bhw_plan.h"

static long g_checks = 0, g_replays = 0, g_odd = 0, g_even = 0, g_parity[2] = {0, 0};
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

static void plan_is_the_inverse_plan(const BhwMaskMfftPlan &pl, const BhwIstftMfftPlan &iv, const bhw_stft &sa, const bhw_stft &ss)
{
    REQUIRE(pl.route == iv.route && pl.normalize == iv.normalize && pl.t0 == iv.t0 && pl.hop == iv.hop && pl.halo == iv.halo, "span plan");
    REQUIRE(pl.span == iv.span && pl.spans == iv.spans && pl.groups == iv.groups && pl.grid == iv.grid && pl.trips == iv.trips, "spans");
    REQUIRE(pl.halo_bound == iv.halo_bound && pl.x_stride == iv.x_stride && pl.len == iv.len, "bounds");
    REQUIRE(pl.m == iv.m && pl.lpf == iv.lpf && pl.fy == iv.fy && pl.cpl == iv.cpl && pl.passes == iv.passes, "lanes");
    REQUIRE(!memcmp(pl.radix, iv.radix, sizeof pl.radix), "schedule");
    REQUIRE(pl.lds_bytes == 2u * pl.fy * pl.m * 8u + 2u * pl.m * 8u + (uint32_t)ss.n_fft * 4u && pl.lds_bytes == iv.lds_bytes + pl.m * 8u, "LDS %u",
            pl.lds_bytes);
    REQUIRE(pl.lds_bytes <= 40000u, "LDS %u", pl.lds_bytes);
    REQUIRE(pl.cpl <= 8u && 8u * pl.lpf >= (uint32_t)ss.n_fft, "columns per lane %u", pl.cpl);
    REQUIRE(pl.in_stride == (sa.x_stride ? sa.x_stride : sa.samples), "in_stride");
}

// The passes of one direction over the slot's M points, lane by lane: reads inside the points, every point written once per pass, the
// twiddle index inside the folded table's range, the float i mod Ns.  (The forward and the inverse passes share this index arithmetic.)
static void replay_passes(const BhwMaskMfftPlan &pl, uint32_t n)
{
    const uint32_t M = pl.m, lpf = pl.lpf;
    std::vector<uint8_t> wrote(M);
    uint32_t Ns = 1, rest = M;
    for (uint32_t p = 0; p < pl.passes; ++p) {
        const uint32_t R = pl.radix[p];
        REQUIRE((R == 5 || R == 3 || R == 4 || R == 2) && rest % R == 0, "radix %u", R);
        rest /= R;
        const uint32_t Q = M / R, ts = 2u * rest;
        REQUIRE(Ns * R * rest == M && ts * R * Ns == n, "pass %u", p);
        std::fill(wrote.begin(), wrote.end(), 0);
        const float exact = 1.0f / (float)Ns;
        for (uint32_t l = 0; l < lpf; ++l)
            for (uint32_t i = l; i < Q; i += lpf) {
                for (uint32_t q = 0; q < R; ++q) REQUIRE(i + q * Q < M, "read %u", i + q * Q);
                uint32_t k = i;
                if (Ns < Q) {
                    k = i % Ns;
                    for (float inv : {exact, std::nextafterf(exact, 0.0f), std::nextafterf(exact, 1.0f)})
                        REQUIRE(i - (uint32_t)(((float)i + 0.5f) * inv) * Ns == k, "float %u mod %u", i, Ns);
                } else {
                    REQUIRE(Ns == Q, "the last pass");
                }
                if (Ns > 1u)
                    for (uint32_t q = 1; q < R; ++q) {
                        const uint32_t idx = q * k * ts;
                        REQUIRE(idx < n && (idx >= M ? idx - M : idx) < M, "twiddle %u", idx);
                    }
                const uint32_t o = (i - k) * R + k;
                for (uint32_t q = 0; q < R; ++q) {
                    REQUIRE(o + q * Ns < M && wrote.at(o + q * Ns) == 0, "point %u written twice or outside", o + q * Ns);
                    wrote[o + q * Ns] = 1;
                }
            }
        for (uint32_t i = 0; i < M; ++i) REQUIRE(wrote[i] == 1, "point %u not written in pass %u", i, p);
        Ns *= R;
    }
    REQUIRE(Ns == M && rest == 1, "the schedule covers M");
}

// One call, as the kernel walks it.  x, g and out are arrays of exactly the extents the checks compute; ASan holds the accesses to them.
static void replay(const BhwMaskMfftPlan &pl, const bhw_stft &sa, const bhw_stft &ss, uint64_t L, uint64_t gs, uint64_t gbs)
{
    const uint32_t M = pl.m, n = (uint32_t)ss.n_fft, lpf = pl.lpf, fy = pl.fy, H = M >> 1, col0 = (uint32_t)ss.col0;
    const uint64_t Tin = sa.samples, T = ss.samples, F = ss.frames, Bn = ss.batch, K = M + 1;
    const uint64_t xs = pl.in_stride, os = pl.x_stride;
    std::vector<uint8_t> x((Bn - 1) * xs + Tin, 1), g((Bn - 1) * gbs + (F - 1) * gs + K, 0), out((Bn - 1) * os + T, 0);
    std::vector<uint8_t> gapx(x.size(), 1), gapg(g.size(), 1), gapo(out.size(), 1);   // 1: a gap of the strides
    for (uint64_t b = 0; b < Bn; ++b) {
        for (uint64_t t = 0; t < Tin; ++t) gapx[b * xs + t] = 0;
        for (uint64_t t = 0; t < T; ++t) gapo[b * os + t] = 0;
        for (uint64_t f = 0; f < F; ++f)
            for (uint64_t k = 0; k < K; ++k) gapg[b * gbs + f * gs + k] = 0;
    }
    const uint32_t passes = pl.passes;
    ++g_parity[passes & 1u];
    ++(M & 1u ? g_odd : g_even);
    std::vector<uint8_t> rowA(n), zw(M), gread(K);
    const uint64_t pool = Bn * pl.spans, hop = pl.hop;
    const uint32_t hm = (uint32_t)(hop % (uint64_t)n);
    for (uint64_t wg = 0; wg < pl.grid; ++wg)
        for (uint64_t grp = wg; grp < pl.groups; grp += pl.grid)
            for (uint32_t slot = 0; slot < fy; ++slot) {
                const uint64_t sp = grp * fy + slot;
                const bool live = sp < pool;
                const uint64_t b = live ? sp / pl.spans : 0, s = live ? sp - b * pl.spans : 0;
                BhwIstftSpan r = bhwp_istft_span(s, pl.span, hop, L, pl.t0, T, F);
                if (!live) r.wlo = r.whi = r.f_lo = r.f_hi = 0;
                uint64_t cur = r.wlo;
                uint32_t bm = (uint32_t)((r.f_lo * hop) % (uint64_t)n);
                auto store = [&](uint64_t w) {
                    REQUIRE(w >= pl.t0 && w - pl.t0 < T, "output %" PRIu64 " outside the signal", w);
                    const uint64_t at = b * os + (w - pl.t0);
                    REQUIRE(!gapo.at(at) && out.at(at) == 0, "output %" PRIu64 " of signal %" PRIu64 " stored twice or in a gap", w, b);
                    out[at] = 1;
                };
                REQUIRE(r.f_hi - r.f_lo <= pl.trips, "frames of a span above trips");
                for (uint64_t it = 0; it < pl.trips; ++it, bm = bm + hm >= n ? bm + hm - n : bm + hm) {
                    const uint64_t f = r.f_lo + it;
                    const bool act = f < r.f_hi;
                    if (!act) continue;                                  // an idle slot reads nothing and its result is not read
                    REQUIRE(f < F, "frame %" PRIu64, f);
                    REQUIRE(bm == (uint32_t)((f * hop) % (uint64_t)n), "the stepped base of frame %" PRIu64, f);
                    // a. the frame load: buffer A of the slot, read by nobody in this phase
                    std::fill(rowA.begin(), rowA.end(), 0);
                    const uint64_t t0 = f * sa.hop - sa.pad;
                    for (uint32_t l = 0; l < lpf; ++l)
                        for (uint32_t j = l; j < n; j += lpf) {
                            const uint32_t k = j - col0;
                            if (k < L) {
                                uint64_t t = t0 + j;
                                if (t >= Tin) {
                                    const int64_t ts = (int64_t)t;
                                    if (sa.pad_mode == BHW_PAD_REFLECT) t = ts < 0 ? (uint64_t)(-ts) : 2 * (Tin - 1) - t;
                                    else t = 0;
                                }
                                REQUIRE(t < Tin, "sample %" PRIu64 " of frame %" PRIu64 " column %u outside [0, T)", t, f, j);
                                REQUIRE(!gapx.at(b * xs + t), "sample read in a gap");
                                REQUIRE(x.at(b * xs + t) == 1, "x");
                            }
                            REQUIRE(rowA.at(j) == 0, "column %u written twice", j);
                            rowA[j] = 1;
                        }
                    for (uint32_t j = 0; j < n; ++j) REQUIRE(rowA[j] == 1, "column %u not written", j);
                    // b. the forward passes alternate between the buffers from A; c. the split reads where they end and writes the other
                    int cur_buf = 0;
                    for (uint32_t p = 0; p < passes; ++p) cur_buf ^= 1;  // each pass reads cur_buf and writes the other: never the same
                    const int split_reads = cur_buf, split_writes = cur_buf ^ 1;
                    REQUIRE(split_reads != split_writes && split_reads == (int)(passes & 1u), "the split writes the buffer it reads");
                    std::fill(zw.begin(), zw.end(), 0);
                    std::fill(gread.begin(), gread.end(), 0);
                    for (uint32_t l = 0; l < lpf; ++l)
                        for (uint32_t k = l; k <= H; k += lpf) {
                            for (uint64_t q : {(uint64_t)k, (uint64_t)(M - k)}) {
                                const uint64_t at = b * gbs + f * gs + q;
                                REQUIRE(at < g.size() && !gapg.at(at), "gain %" PRIu64 " of frame %" PRIu64 " outside its row", q, f);
                                gread.at(q) = 1;
                            }
                            // reads src[k], src[M - k], src[0]; writes Z[k] and, where 2 k != M and k != 0, Z[M - k]
                            REQUIRE(zw.at(k) == 0, "Z[%u] written twice", k);
                            zw[k] = 1;
                            if (k != 0 && 2u * k != M) {
                                REQUIRE(M - k < M && zw.at(M - k) == 0, "Z[%u] written twice", M - k);
                                zw[M - k] = 1;
                            }
                        }
                    for (uint32_t k = 0; k < M; ++k) REQUIRE(zw[k] == 1, "Z[%u] not written", k);
                    for (uint64_t k = 0; k < K; ++k) REQUIRE(gread[k] == 1, "gain %" PRIu64 " not read", k);
                    // the inverse passes start from Z and end where the ring reads; the next trip's load writes A after the last barrier
                    int inv = split_writes;
                    for (uint32_t p = 0; p < passes; ++p) inv ^= 1;
                    REQUIRE(inv == 1, "the ring reads buffer B whatever the parity: %u passes each way and the split", passes);
                    // the ring and the flush
                    const uint64_t base = f * hop;
                    if (cur < base) {
                        for (uint64_t w = cur; w < base; ++w) store(w);
                        cur = base;
                    }
                    uint64_t end = (f + 1 == r.f_hi || base + hop > r.whi) ? r.whi : base + hop;
                    if (end < cur) end = cur;
                    for (uint32_t c = 0; c < 8u; ++c)                     // MaskMfftSource::kMaxCpl
                        for (uint32_t l = 0; l < lpf; ++l) {
                            if (!(c < pl.cpl && c * lpf + l < n)) continue;      // the cols mask
                            const uint32_t q = c * lpf + l;
                            const uint32_t k = q >= bm ? q - bm : q + n - bm;
                            REQUIRE(k < n, "ring index %u", k);
                            const uint64_t w = base + k;
                            if (k < L && w >= cur && w < r.whi && w < end) store(w);
                        }
                    const uint64_t reach = base + L;
                    if (reach < end)
                        for (uint64_t w = reach > cur ? reach : cur; w < end; ++w) store(w);
                    cur = end;
                }
                if (live)
                    for (uint64_t w = cur; w < r.whi; ++w) store(w);
            }
    for (uint64_t i = 0; i < out.size(); ++i) REQUIRE(out[i] == (gapo[i] ? 0 : 1), "output word %" PRIu64 " not stored exactly once", i);
    ++g_replays;
}

int main()
{
    bhw_params p;
    REQUIRE(bhw_params_init(&p, BHW_WIN_BH4, 12, 16) == BHW_OK, "params");
    char line[1280];
    uint64_t combo = 0, sizes = 0;
    // addresses that are never dereferenced: the checks only compare them
    const void *X = (const void *)0x10000000, *G = (const void *)0x4000000000ull, *O = (const void *)0x8000000000ull;
    for (uint64_t n = 1; n <= kMaskMfftMaxN; ++n) {
        if (!bhwp_mfft_supported(n)) continue;
        ++sizes;
        const uint64_t K = n / 2 + 1;
        bool passes_done = false;
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
                                    ++combo;                           // the larger calls are replayed under one gain form each, in turn
                                    for (const auto &gf : forms) {
                                        const int rc = bhwp_mask_mfft_checks(&p, L, &sa, &ss, flags, X, G, gf[0], gf[1], O);
                                        REQUIRE(rc == BHW_OK, "checks %d n %" PRIu64 " L %" PRIu64 " hop %" PRIu64 " F %" PRIu64, rc, n, L, hop, F);
                                        for (int table = 0; table < 2; ++table) {
                                            const BhwMaskMfftPlan pl = bhwp_mask_mfft_plan(&p, L, &sa, &ss, flags, gf[0], gf[1], table != 0);
                                            plan_is_the_inverse_plan(pl, bhwp_istft_mfft_plan(&p, L, &ss, flags, table != 0), sa, ss);
                                            REQUIRE(pl.g_stride == gf[0] && pl.g_bstride == gf[1], "gain strides");
                                        }
                                        REQUIRE(bhwp_describe_mask_mfft(&p, nullptr, L, &sa, &ss, flags, gf[0], gf[1], line, sizeof line) == BHW_OK, "describe");
                                        REQUIRE(strstr(line, "forward + inverse FFT") && strstr(line, "k_mask_mfft_direct") && strlen(line) < sizeof line - 1,
                                                "line");
                                        REQUIRE(bhwp_describe_mask_mfft(&p, nullptr, L, &sa, &ss, flags, gf[0], gf[1], line, 40) == BHW_OK, "short buffer");
                                        const BhwMaskMfftPlan pl = bhwp_mask_mfft_plan(&p, L, &sa, &ss, flags, gf[0], gf[1], false);
                                        if (!passes_done) {              // the schedule and the lanes are functions of n_fft alone
                                            replay_passes(pl, (uint32_t)n);
                                            passes_done = true;
                                        }
                                        // the replay, where the call is small enough to walk lane by lane
                                        const uint64_t work = nb * F * n;
                                        if (work <= (1u << 8) || (work <= (1u << 11) && T <= (1u << 12) && (size_t)(&gf - forms) == combo % 5))
                                            replay(pl, sa, ss, L, gf[0], gf[1]);
                                    }
                                    // a gain stride below its bound, and out inside x or g: refused
                                    REQUIRE(bhwp_mask_mfft_checks(&p, L, &sa, &ss, flags, X, G, K - 1, 0, O) == BHW_ERR_BADARG, "g_stride");
                                    if (F > 1) REQUIRE(bhwp_mask_mfft_checks(&p, L, &sa, &ss, flags, X, G, K, F * K - 1, O) == BHW_ERR_BADARG, "g_batch_stride");
                                    REQUIRE(bhwp_mask_mfft_checks(&p, L, &sa, &ss, flags, X, G, 0, 0, (const char *)X + 4 * (Tin - 1)) == BHW_ERR_BADARG, "x overlap");
                                    REQUIRE(bhwp_mask_mfft_checks(&p, L, &sa, &ss, flags, X, G, 0, 0, (const char *)G + 4 * (K - 1)) == BHW_ERR_BADARG, "g overlap");
                                    REQUIRE(bhwp_mask_mfft_checks(&p, L, &sa, &ss, flags, X, G, 0, 0, (const char *)G + 4 * K) == BHW_OK, "behind one gain row");
                                }
    }
    REQUIRE(sizes == 73, "%" PRIu64 " sizes", sizes);
    REQUIRE(g_odd > 0 && g_even > 0 && g_parity[0] > 0 && g_parity[1] > 0, "M odd %ld, even %ld, passes even %ld, odd %ld", g_odd, g_even,
            g_parity[0], g_parity[1]);
    // the sizes the call does not take
    for (uint64_t n : {8ull, 14ull, 22ull, 512ull, 2048ull, 2160ull, 2560ull, 4050ull, 4096ull, 8192ull}) {
        const bhw_stft s = desc_of(1, 100000, 3, 7, n, 0, n / 2, 0, 0);
        REQUIRE(bhwp_mask_mfft_checks(&p, 8, &s, &s, 0, X, G, 0, 0, O) == BHW_ERR_UNSUPPORTED, "n_fft %" PRIu64, n);
    }
    printf("ok %ld checks, %ld call replays\n", g_checks, g_replays);
    return 0;
}
