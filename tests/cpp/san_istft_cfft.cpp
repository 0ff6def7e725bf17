// san_istft_cfft.cpp -- the planner's part of the fused inverse complex FFT + overlap-add calls for I/Q output (bhw_plan.cpp:
// bhwp_istft_cfft_checks / bhwp_istft_cfft_plan / bhwp_describe_istft_cfft, bhwp_istft_span of bhw_plan.h) swept under
// AddressSanitizer + UBSan over every supported n_fft against L, hop, batch, frames and `samples` at the edges, padded, odd and
// packed, centred and not, with all four flag combinations.  Besides "no report" it asserts the plan's invariants -- LDS within
// 48 KiB, lanes x slots = the workgroup, lanes x columns = n_fft, the lanes and passes of bhwp_stft_cfft_plan, S >= 4 * halo, the spans
// covering the outputs, grid within its bound -- and replays on the host the kernel's index arithmetic (bhw_istft_cfft.hip):
//   - the span walk: every span (b, s) of the pool taken by exactly one (workgroup, trip of the group loop, slot); its frame list
//     within `trips`, and exactly the frames that reach its outputs;
//   - the load: every bin of a row read exactly once, inside the row and Y's extent, with and without the shift, and bin k taken
//     from the column that holds it;
//   - the passes, in float with float32-rounded binary64 twiddles: every point of the destination written exactly once per pass,
//     every twiddle index inside the table after folding, and the scaled result against a direct binary64 inverse DFT of the float32
//     bins within 2^-24 * log2(n_fft) in relative l2 error, for every n_fft (the largest share of that cap is printed);
//   - the ring and the flush, lane by lane: every output pair (b, t) stored exactly once, inside x's extent and never in a gap; the
//     products added to an output are exactly (f, u - f * hop) for the frames reaching it, each once, in ascending f; outputs no
//     frame reaches stored as zeros; every accumulator clear when its slot leaves a span.
// The replay is a copy of the kernel's index arithmetic kept in step by hand (only bhwp_istft_span is shared code): a change of the
// load index, the pass indices, the ring or the flush bound in bhw_istft_cfft.hip has to be made here as well, or this program goes
// on checking the old kernel.
#include <cinttypes>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <utility>
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
static double unit() { return (double)(rnd() >> 11) / 9007199254740992.0 - 0.5; }

static bhw_stft desc_of(uint64_t B, uint64_t T, uint64_t frames, uint64_t hop, uint64_t n_fft, uint64_t col0, uint64_t pad)
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
    s.shift = 15;
    return s;
}

static void plan_invariants(const BhwIstftCfftPlan &pl, const bhw_stft &s, uint64_t L, const bhw_params *p)
{
    const uint64_t n = s.n_fft, end = s.pad - s.col0 + s.samples;
    REQUIRE((1ull << pl.log2n) == n && pl.n == n, "log2n %u n %u", pl.log2n, pl.n);
    REQUIRE(pl.lpf * pl.fy == kFftBlock && (uint64_t)pl.lpf * pl.cpl == n && pl.cpl <= kCfftMaxCpl && pl.cpl >= 4, "lanes %u x %u, %u columns", pl.lpf, pl.fy, pl.cpl);
    REQUIRE(2 * pl.radix4 + pl.radix2 == pl.log2n && pl.radix2 <= 1, "schedule %u x 4, %u x 2", pl.radix4, pl.radix2);
    const BhwStftCfftPlan fw = bhwp_stft_cfft_plan(p, L, &s, 0, false);
    REQUIRE(fw.lpf == pl.lpf && fw.fy == pl.fy && fw.cpl == pl.cpl && fw.radix4 == pl.radix4 && fw.radix2 == pl.radix2, "the forward's lanes and passes");
    REQUIRE(pl.lds_bytes == 2u * pl.fy * pl.n * 8u + pl.n / 2u * 8u + n * 4u && pl.lds_bytes <= 48u * 1024u, "LDS %u", pl.lds_bytes);
    REQUIRE(pl.t0 == s.pad - s.col0 && pl.hop >= 1 && pl.hop <= s.hop && (pl.hop == s.hop || pl.hop == end), "t0 %" PRIu64 " hop %" PRIu64, pl.t0, pl.hop);
    REQUIRE(pl.halo == (L + pl.hop - 1) / pl.hop - 1, "halo %" PRIu64, pl.halo);
    REQUIRE(pl.span >= 1 && pl.span <= s.frames && (pl.span >= kIfftHaloFactor * pl.halo || pl.span == s.frames || pl.span * pl.hop >= end), "S %" PRIu64 " halo %" PRIu64, pl.span, pl.halo);
    REQUIRE(pl.spans >= 1 && pl.spans * pl.span * pl.hop >= end && (pl.spans - 1) * pl.span * pl.hop < end, "spans %" PRIu64, pl.spans);
    REQUIRE(pl.groups == (s.batch * pl.spans + pl.fy - 1) / pl.fy, "groups %" PRIu64, pl.groups);
    REQUIRE(pl.grid >= 1 && pl.grid <= kFftMaxGrid && (pl.grid == pl.groups || (pl.grid == kFftMaxGrid && pl.groups > pl.grid)), "grid %" PRIu64, pl.grid);
    REQUIRE(pl.trips >= 1 && pl.trips <= s.frames && pl.trips <= pl.span + pl.halo, "trips %" PRIu64, pl.trips);
    REQUIRE(pl.y_stride >= 2 * n && pl.y_stride % 2 == 0 && pl.y_bstride % 2 == 0 && pl.x_stride >= 2 * s.samples, "strides");
}

typedef std::complex<float> cf;
// the kernel's cmul, unfused
static cf cmulf(cf a, cf w) { return cf(a.real() * w.real() - a.imag() * w.imag(), a.real() * w.imag() + a.imag() * w.real()); }

// the load and the passes of one row in float, with the kernel's indices and its twiddle table; `cols` is the row as it lies in memory
// (bin (j + n / 2) mod n in column j when shifted); returns the scaled row fl32(z / n)
static std::vector<cf> replay_transform(const BhwIstftCfftPlan &pl, const std::vector<cf> &cols)
{
    const uint32_t n = pl.n, H = n / 2, Q = n / 4;
    std::vector<cf> tw(H), a(n), b(n);
    for (uint32_t k = 0; k < H; ++k) tw[k] = cf((float)cos(2.0 * M_PI * k / n), (float)sin(2.0 * M_PI * k / n));
    auto W = [&](uint32_t idx) {
        REQUIRE(idx < n, "twiddle index %u of %u", idx, n);
        const cf w = tw[idx & (H - 1)];
        return (idx & H) ? -w : w;
    };
    cf *src = a.data(), *dst = b.data();
    std::vector<int> hit(n, 0), readY(n, 0);
    const uint32_t turn = pl.shifted ? H : 0u;
    for (uint32_t l = 0; l < pl.lpf; ++l)
        for (uint32_t c = 0; c < pl.cpl; ++c) {
            const uint32_t k = c * pl.lpf + l, col = (k + turn) & (n - 1);
            REQUIRE(k < n && col < n, "bin %u column %u", k, col);
            REQUIRE(pl.shifted ? (col + H) % n == k : col == k, "bin %u read from column %u", k, col);
            src[k] = cols[col];
            ++hit[k];
            ++readY[col];
        }
    for (uint32_t i = 0; i < n; ++i) REQUIRE(hit[i] == 1 && readY[i] == 1, "load: point %u written %d times, column read %d times", i, hit[i], readY[i]);
    uint32_t Ns = 1;
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
                const cf t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, t3 = cf(a3.imag() - a1.imag(), a1.real() - a3.real());
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
    const float scale = 1.0f / (float)n;
    std::vector<cf> row(n);
    for (uint32_t i = 0; i < n; ++i) row[i] = cf(src[i].real() * scale, src[i].imag() * scale);
    return row;
}

// The group loop, the frame walk, the ring and the stores of every lane.  An accumulator is the list of the (f, k) it was given.
typedef std::vector<std::pair<uint64_t, uint32_t>> Terms;
static void replay_spans(const BhwIstftCfftPlan &pl, const bhw_stft &s, uint64_t L)
{
    const uint64_t F = s.frames, B = s.batch, T = s.samples, n = s.n_fft, hop = pl.hop;
    const uint64_t yext = (B - 1) * pl.y_bstride + (F - 1) * pl.y_stride + 2 * n, xext = (B - 1) * pl.x_stride + 2 * T, pool = B * pl.spans;
    std::vector<int> owned(pool, 0), stored(B * T, 0);
    std::vector<Terms> ring(kFftBlock * kCfftMaxCpl);                      // [tid][c]: one list for the two sums and the envelope
    auto store = [&](uint64_t b, uint64_t w, const Terms &terms) {
        REQUIRE(w >= pl.t0 && w - pl.t0 < T, "output w %" PRIu64 " (t0 %" PRIu64 ", samples %" PRIu64 ", n_fft %" PRIu64 ", L %" PRIu64 ", hop %" PRIu64 ", frames %" PRIu64 ")", w, pl.t0, T, n, L, s.hop, F);
        const uint64_t t = w - pl.t0;
        REQUIRE(b * pl.x_stride + 2 * t + 2 <= xext && 2 * t + 2 <= 2 * T, "x index");      // the pair inside the signal, never in a gap
        ++stored[b * T + t];
        // the contract: the frames f with 0 <= w - f * hop < L, ascending (the real hop: a hop past the outputs leaves frame 0 alone)
        Terms want;
        for (uint64_t f = w >= L ? (w - L) / s.hop : 0; f < F && (unsigned __int128)f * s.hop <= w; ++f)
            if (w - f * s.hop < L) want.push_back({f, (uint32_t)(w - f * s.hop)});
        REQUIRE(terms == want, "output b %" PRIu64 " t %" PRIu64 ": %zu terms, the contract has %zu", b, t, terms.size(), want.size());
    };
    const uint32_t turn = pl.shifted ? (uint32_t)(n / 2) : 0u;
    for (uint64_t wg = 0; wg < pl.grid; ++wg)
        for (uint64_t g = wg; g < pl.groups; g += pl.grid)
            for (uint32_t slot = 0; slot < pl.fy; ++slot) {
                const uint64_t sp = g * pl.fy + slot;
                if (sp >= pool) continue;
                ++owned[sp];
                const uint64_t b = sp / pl.spans, si = sp - b * pl.spans;
                const BhwIstftSpan r = bhwp_istft_span(si, pl.span, hop, L, pl.t0, T, F);
                REQUIRE(r.f_hi - r.f_lo <= pl.trips && r.f_hi <= F && r.wlo <= r.whi, "span %" PRIu64 ": frames [%" PRIu64 ", %" PRIu64 ") of %" PRIu64 " trips", si, r.f_lo, r.f_hi, pl.trips);
                // exactly the frames that reach the span's outputs
                for (uint64_t f = r.wlo >= L + hop ? (r.wlo - L) / hop - 1 : 0; f < F; ++f) {
                    const bool reaches = f * hop < r.whi && f * hop + L > r.wlo && r.whi > r.wlo;
                    REQUIRE(reaches == (f >= r.f_lo && f < r.f_hi), "span %" PRIu64 " frame %" PRIu64, si, f);
                    if (f * hop >= r.whi) break;
                }
                std::vector<uint64_t> cur(pl.lpf, r.wlo);
                for (uint64_t it = 0; it < pl.trips; ++it) {
                    const uint64_t f = r.f_lo + it;
                    if (f >= r.f_hi) continue;
                    for (uint32_t l = 0; l < pl.lpf; ++l) {
                        const uint32_t tid = slot * pl.lpf + l;
                        for (uint32_t c = 0; c < pl.cpl; ++c) {
                            const uint64_t col = (c * pl.lpf + l + turn) & (n - 1);
                            const uint64_t y0 = b * pl.y_bstride + f * pl.y_stride;
                            REQUIRE(y0 + 2 * col + 2 <= yext && 2 * col + 2 <= pl.y_stride, "Y index");
                        }
                        const uint64_t base = f * hop;
                        uint64_t c0 = cur[l];
                        if (c0 < base) {
                            for (uint64_t w = c0 + l; w < base; w += pl.lpf) store(b, w, Terms());
                            c0 = base;
                        }
                        uint64_t end = (f + 1 == r.f_hi || base + hop > r.whi) ? r.whi : base + hop;
                        if (end < c0) end = c0;
                        const uint32_t bm = (uint32_t)(base & (n - 1));
                        for (uint32_t c = 0; c < pl.cpl; ++c) {
                            const uint32_t k = (c * pl.lpf + l - bm) & (uint32_t)(n - 1);
                            const uint64_t w = base + k;
                            if (k < L && w >= c0 && w < r.whi) {
                                REQUIRE(s.col0 + k < n, "row column %" PRIu64, s.col0 + k);
                                Terms &acc = ring[tid * kCfftMaxCpl + c];
                                acc.push_back({f, k});
                                if (w < end) {
                                    store(b, w, acc);
                                    acc.clear();
                                }
                            }
                        }
                        const uint64_t reach = base + L;
                        if (reach < end)
                            for (uint64_t w = (reach > c0 ? reach : c0) + l; w < end; w += pl.lpf) store(b, w, Terms());
                        cur[l] = end;
                    }
                }
                for (uint32_t l = 0; l < pl.lpf; ++l) {
                    for (uint64_t w = cur[l] + l; w < r.whi; w += pl.lpf) store(b, w, Terms());
                    for (uint32_t c = 0; c < kCfftMaxCpl; ++c) REQUIRE(ring[(slot * pl.lpf + l) * kCfftMaxCpl + c].empty(), "accumulator left full");
                }
            }
    for (uint64_t i = 0; i < pool; ++i) REQUIRE(owned[i] == 1, "span %" PRIu64 " owned %d times", i, owned[i]);
    for (uint64_t i = 0; i < stored.size(); ++i) REQUIRE(stored[i] == 1, "output %" PRIu64 " stored %d times", i, stored[i]);
}

int main()
{
    char buf[1100];
    long span_replays = 0, pass_replays = 0, cut = 0;
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 12, 24);
    const uint64_t xa = 0x10000000ull, ya = 0x100000000000ull;
    double worst_share = 0.0;
    for (uint32_t lg = kCfftMinLog; lg <= kCfftMaxLog; ++lg) {
        const uint64_t n = 1ull << lg;
        // the load and the passes in float against a direct binary64 inverse DFT of the float32 bins: relative l2 error within
        // 2^-24 * log2 n, shifted and in order
        for (int trial = 0; trial < 4; ++trial) {
            bhw_stft s = desc_of(1, n, 1, 1, n, 0, 0);
            const uint32_t flags = (trial & 1) ? BHW_CFFT_SHIFT : 0u;
            const BhwIstftCfftPlan pl = bhwp_istft_cfft_plan(&p, n, &s, flags, false);
            std::vector<cf> bins(n), cols(n);
            for (uint64_t k = 0; k < n; ++k)
                bins[k] = cf((float)(unit() * 1000.0 + (trial == 2 && k == 0 ? 250.0 * (double)n : 0.0)), (float)(unit() * 1000.0 + cos(0.7 * (double)k) * (trial == 3 ? 1e3 : 0.0)));
            for (uint64_t j = 0; j < n; ++j) cols[j] = bins[(flags ? j + n / 2 : j) % n];
            const std::vector<cf> row = replay_transform(pl, cols);
            double ne = 0, nr = 0;
            std::vector<std::complex<double>> e(n);
            for (uint64_t j = 0; j < n; ++j) e[j] = std::polar(1.0, 2.0 * M_PI * (double)j / (double)n);
            for (uint64_t j = 0; j < n; ++j) {
                std::complex<double> d(0, 0);
                for (uint64_t k = 0; k < n; ++k) d += std::complex<double>(bins[k].real(), bins[k].imag()) * e[(j * k) % n];
                d /= (double)n;
                ne += std::norm(d - std::complex<double>(row[j].real(), row[j].imag()));
                nr += std::norm(d);
            }
            const double err = sqrt(ne / nr), cap = ldexp((double)lg, -24);
            REQUIRE(err <= cap, "n %" PRIu64 " trial %d: relative l2 error %.3e above the cap %.3e", n, trial, err, cap);
            if (err / cap > worst_share) worst_share = err / cap;
            ++pass_replays;
        }
        for (uint64_t L : {(uint64_t)1, (uint64_t)13, n / 2 + 1, n - 1, n})
            for (uint64_t hop : {(uint64_t)1, (uint64_t)7, n / 4 + 3, n, n + 5})
                for (uint64_t B : {1ull, 3ull, 70ull})
                    for (uint64_t F : {1ull, 2ull, 65ull, 700ull})
                        for (int centred = 0; centred <= 1; ++centred)
                            for (int tail = 0; tail < 3; ++tail)            // samples: torch's default, shorter, past the frames' extent
                                for (int padded = 0; padded <= 2; ++padded) {   // packed, gaps on the 8-byte grid, an odd x_stride
                                    if (!centred && L < n) continue;        // pad < col0
                                    const uint64_t pad = centred ? n / 2 : 0, col0 = (n - L) / 2;
                                    const uint64_t full = n + hop * (F - 1);
                                    if (full <= 2 * pad) continue;
                                    uint64_t T = full - 2 * pad;
                                    if (tail == 1) T = T > 5 ? T - 5 : 1;
                                    if (tail == 2) T += n + 2 * hop + 3;
                                    bhw_stft s = desc_of(B, T, F, hop, n, col0, pad);
                                    if (padded) {
                                        s.x_stride = padded == 1 ? 2 * T + 6 : 2 * T + 3;
                                        s.y_stride = 2 * n + 6;
                                        s.y_batch_stride = F * s.y_stride + 10;
                                    }
                                    if ((unsigned __int128)B * F * n > (1ull << 34)) continue;
                                    for (uint32_t flags : {0u, 1u, 4u, 5u}) {
                                        int rc = bhwp_istft_cfft_checks(&p, L, &s, flags, nullptr, nullptr, false);
                                        REQUIRE(rc == BHW_OK, "checks rc %d: n %" PRIu64 " L %" PRIu64 " hop %" PRIu64 " B %" PRIu64 " F %" PRIu64, rc, n, L, hop, B, F);
                                        rc = bhwp_istft_cfft_checks(&p, L, &s, flags, (const void *)ya, (const void *)(xa + (padded == 2 ? 4 : 0)));
                                        REQUIRE(rc == BHW_OK, "pointer checks rc %d", rc);
                                    }
                                    REQUIRE(bhwp_istft_cfft_checks(&p, L, &s, 0, (const void *)(ya + 4), (const void *)xa) == BHW_ERR_BADARG, "misaligned Y");
                                    REQUIRE(bhwp_istft_cfft_checks(&p, L, &s, 0, (const void *)ya, (const void *)(xa + 2)) == BHW_ERR_BADARG, "misaligned x");
                                    REQUIRE(bhwp_istft_cfft_checks(&p, L, &s, 0, (const void *)ya, (const void *)ya) == BHW_ERR_BADARG, "overlap");
                                    REQUIRE(bhwp_istft_cfft_checks(&p, L, &s, 2u, nullptr, nullptr, false) == BHW_ERR_BADARG, "flags");
                                    REQUIRE(bhwp_istft_cfft_checks(&p, L, &s, 8u, nullptr, nullptr, false) == BHW_ERR_BADARG, "flags");
                                    const uint32_t flags = (tail == 0 ? BHW_OLA_NORMALIZE : 0u) | ((B + hop) % 2 ? BHW_CFFT_SHIFT : 0u);
                                    const BhwIstftCfftPlan pl = bhwp_istft_cfft_plan(&p, L, &s, flags, (B + F) % 2 == 0);
                                    plan_invariants(pl, s, L, &p);
                                    REQUIRE(bhwp_describe_istft_cfft(&p, nullptr, L, &s, flags, buf, sizeof buf) == BHW_OK && strlen(buf) > 40 && strlen(buf) < sizeof buf - 1, "describe");
                                    if (B * (T + F * L) <= 6000 || (B == 1 && F == 700 && hop == 7 && L == 13)) {
                                        replay_spans(pl, s, L);
                                        ++span_replays;
                                        if (pl.spans > 1) ++cut;
                                    }
                                    bhw_stft bad = s;
                                    bad.y_stride = 2 * n - 2;
                                    REQUIRE(bhwp_istft_cfft_checks(&p, L, &bad, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "short y_stride");
                                    bad.y_stride = 2 * n + 3;
                                    REQUIRE(bhwp_istft_cfft_checks(&p, L, &bad, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "odd y_stride");
                                    bad = s;
                                    bad.y_batch_stride = F * (s.y_stride ? s.y_stride : 2 * n) + 1;
                                    REQUIRE(bhwp_istft_cfft_checks(&p, L, &bad, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "odd y_batch_stride");
                                    bad = s;
                                    bad.x_stride = 2 * T - 1;
                                    REQUIRE(bhwp_istft_cfft_checks(&p, L, &bad, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "short x_stride");
                                    bad = s;
                                    bad.channels = 1;
                                    bad.x_stride = 0;
                                    REQUIRE(bhwp_istft_cfft_checks(&p, L, &bad, 0, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED, "channels");
                                    bad = s;
                                    bad.pad_mode = BHW_PAD_REFLECT;
                                    REQUIRE(bhwp_istft_cfft_checks(&p, L, &bad, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "pad_mode");
                                    bad = s;
                                    bad.samples = 0;
                                    bad.x_stride = 0;
                                    bad.y_stride = 3;                       // samples 0: the strides are not looked at
                                    REQUIRE(bhwp_istft_cfft_checks(&p, L, &bad, 4, nullptr, nullptr) == BHW_OK, "samples 0");
                                    REQUIRE(bhwp_describe_istft_cfft(&p, nullptr, L, &bad, 0, buf, sizeof buf) == BHW_OK, "describe samples 0");
                                }
    }
    // a hop past every output, up to 2^63: frame 0 alone
    for (uint64_t hop : {5000ull, 1ull << 40, 1ull << 63}) {
        bhw_stft s = desc_of(2, 700, 3, hop, 256, 28, 128);
        REQUIRE(bhwp_istft_cfft_checks(&p, 200, &s, 5, nullptr, nullptr, false) == BHW_OK, "hop %" PRIu64, hop);
        const BhwIstftCfftPlan pl = bhwp_istft_cfft_plan(&p, 200, &s, 5, false);
        plan_invariants(pl, s, 200, &p);
        replay_spans(pl, s, 200);
    }
    for (uint64_t n : {1ull, 2ull, 8ull, 15ull, 17ull, 48ull, 100ull, 1000ull, 2049ull, 4096ull, 8192ull, 1ull << 20}) {
        bhw_stft s = desc_of(1, 100, 2, 1, n, 0, n / 2);
        REQUIRE(bhwp_istft_cfft_checks(&p, 1, &s, 0, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED, "n_fft %" PRIu64, n);
    }
    {
        bhw_stft s = desc_of(1ull << 20, 100, 2048, 16, 16, 0, 8);             // 2^31 rows x 16 columns = 2^35 > 2^34
        REQUIRE(bhwp_istft_cfft_checks(&p, 16, &s, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "cap");
        s = desc_of(1, 100, 0, 16, 16, 0, 8);
        REQUIRE(bhwp_istft_cfft_checks(&p, 16, &s, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "frames 0 with samples");
        s = desc_of(1, 100, 4, 16, 16, 3, 2);
        REQUIRE(bhwp_istft_cfft_checks(&p, 10, &s, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "pad < col0");
        // the order: a descriptor error before an unknown flag, an unknown flag before the unsupported channels and n_fft
        s = desc_of(1, 100, 4, 0, 4096, 0, 2048);
        REQUIRE(bhwp_istft_cfft_checks(&p, 16, &s, 8, nullptr, nullptr, false) == BHW_ERR_BADARG, "hop 0 first");
        s.hop = 16;
        REQUIRE(bhwp_istft_cfft_checks(&p, 16, &s, 8, nullptr, nullptr, false) == BHW_ERR_BADARG, "then the flags");
        REQUIRE(bhwp_istft_cfft_checks(&p, 16, &s, 4, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED, "then n_fft");
    }
    REQUIRE(bhwp_istft_cfft_checks(&p, 16, nullptr, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "NULL descriptor");
    REQUIRE(span_replays > 1500 && cut > 200 && pass_replays == 32, "replays %ld (%ld cut into spans) %ld", span_replays, cut, pass_replays);
    printf("ok %ld checks, %ld span replays (%ld of signals cut into several spans), %ld pass replays, worst error %.3f of the cap\n", g_checks,
           span_replays, cut, pass_replays, worst_share);
    return 0;
}
