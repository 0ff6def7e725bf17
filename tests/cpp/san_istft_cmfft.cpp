// san_istft_cmfft.cpp -- the planner's part of the fused inverse mixed-radix complex FFT + overlap-add calls for I/Q output
// (bhw_plan.cpp: bhwp_istft_cmfft_checks / bhwp_istft_cmfft_plan / bhwp_describe_istft_cmfft, bhwp_istft_span of bhw_plan.h) under
// AddressSanitizer + UBSan at all 91 supported n_fft.  Besides "no report" it asserts the plan's invariants -- LDS within 56 700
// bytes, lanes x slots = the workgroup, cpl = ceil(n / lpf) <= 8, the lanes, passes and twiddle entries of bhwp_stft_cmfft_plan,
// S >= 4 * halo, the spans covering the outputs, grid within its bound -- and replays on the host the kernel's index arithmetic
// (bhw_istft_cmfft.hip):
//   - the load, at every size: every bin of a row read exactly once, inside the row, with and without the shift; bin k taken from
//     column (k + n / 2) mod n, the column bhw_stft_cmfft.h stores it to; the parts swapped;
//   - the passes, at every size, in float with float32-rounded binary64 twiddles of the FORWARD table: every point read and written
//     exactly once per pass, i mod Ns by the float multiply, every twiddle index below `fold` after the fold and never folded at an
//     odd n; the swapped result times c = (float)(1.0 / (double) n) against a direct binary64 inverse DFT of the float32 bins within
//     2^-24 * log2(n_fft) in relative l2 error (the largest share of that cap is printed);
//   - the ring and the flush, lane by lane, on the geometries of tests/istft_cmfft_cases.py and a sweep: every output pair (b, t)
//     stored exactly once, inside x's extent and never in a gap; the products added to an output are exactly (f, u - f * hop) for the
//     frames reaching it, each once, in ascending f; outputs no frame reaches stored as zeros; every accumulator clear when its slot
//     leaves a span; the stepped base mod n_fft equal to the true modulo.
// The replay is a copy of the kernel's index arithmetic kept in step by hand (only bhwp_istft_span is shared code): a change of the
// load index, the ring or the flush bound in bhw_istft_cmfft.hip, or of mfft_pass in bhw_stft_mfft.h, has to be made here as well.
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

static bool supported(uint64_t n)
{
    if (n < 16 || n > 2047 || !(n & (n - 1))) return false;
    for (uint64_t r : {2ull, 3ull, 5ull})
        while (n % r == 0) n /= r;
    return n == 1;
}

static void plan_invariants(const BhwIstftCmfftPlan &pl, const bhw_stft &s, uint64_t L, const bhw_params *p)
{
    const uint64_t n = s.n_fft, end = s.pad - s.col0 + s.samples;
    REQUIRE(pl.n == n && pl.fold == ((n & 1) ? n : n / 2), "n %u fold %u", pl.n, pl.fold);
    REQUIRE(pl.lpf * pl.fy == kFftBlock && pl.cpl == (n + pl.lpf - 1) / pl.lpf && pl.cpl <= kCfftMaxCpl && pl.cpl >= 3, "lanes %u x %u, %u columns", pl.lpf, pl.fy, pl.cpl);
    const BhwStftCmfftPlan fw = bhwp_stft_cmfft_plan(p, L, &s, 0, false);
    REQUIRE(fw.lpf == pl.lpf && fw.fy == pl.fy && fw.cpl == pl.cpl && fw.passes == pl.passes && fw.fold == pl.fold && !memcmp(fw.radix, pl.radix, sizeof fw.radix),
            "the forward's lanes, passes and twiddles");
    REQUIRE(pl.lds_bytes == 2u * pl.fy * pl.n * 8u + pl.fold * 8u + n * 4u && pl.lds_bytes <= 56700u, "LDS %u", pl.lds_bytes);
    REQUIRE(pl.t0 == s.pad - s.col0 && pl.hop >= 1 && pl.hop <= s.hop && (pl.hop == s.hop || pl.hop == end), "t0 %" PRIu64 " hop %" PRIu64, pl.t0, pl.hop);
    REQUIRE(pl.halo == (L + pl.hop - 1) / pl.hop - 1, "halo %" PRIu64, pl.halo);
    REQUIRE(pl.span >= 1 && pl.span <= s.frames && (pl.span >= kIfftHaloFactor * pl.halo || pl.span == s.frames || pl.span * pl.hop >= end), "S %" PRIu64 " halo %" PRIu64, pl.span, pl.halo);
    REQUIRE(pl.spans >= 1 && pl.spans * pl.span * pl.hop >= end && (pl.spans - 1) * pl.span * pl.hop < end, "spans %" PRIu64, pl.spans);
    REQUIRE(pl.groups == (s.batch * pl.spans + pl.fy - 1) / pl.fy, "groups %" PRIu64, pl.groups);
    REQUIRE(pl.grid >= 1 && pl.grid <= kFftMaxGrid && (pl.grid == pl.groups || (pl.grid == kFftMaxGrid && pl.groups > pl.grid)), "grid %" PRIu64, pl.grid);
    REQUIRE(pl.trips >= 1 && pl.trips <= s.frames && pl.trips <= pl.span + pl.halo, "trips %" PRIu64, pl.trips);
    REQUIRE(pl.y_stride >= 2 * n && pl.y_stride % 2 == 0 && pl.y_bstride % 2 == 0 && pl.x_stride >= 2 * s.samples, "strides");
}

struct C32 {
    float x, y;
};
static C32 cmul(C32 a, C32 w) { return C32{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }
static C32 add(C32 a, C32 b) { return C32{a.x + b.x, a.y + b.y}; }
static C32 sub(C32 a, C32 b) { return C32{a.x - b.x, a.y - b.y}; }
static C32 scl(float s, C32 a) { return C32{s * a.x, s * a.y}; }

// mfft_butterfly of bhw_stft_mfft.h: the FORWARD butterflies
static void butterfly(uint32_t R, C32 *a)
{
    static const float kSin3 = (float)0.86602540378443864676, kCos5a = (float)0.30901699437494742410, kCos5b = (float)-0.80901699437494742410,
                       kSin5a = (float)0.95105651629515357212, kSin5b = (float)0.58778525229247312917;
    if (R == 2) {
        const C32 a0 = a[0], a1 = a[1];
        a[0] = add(a0, a1);
        a[1] = sub(a0, a1);
    } else if (R == 3) {
        const C32 t1 = add(a[1], a[2]), d = sub(a[1], a[2]);
        const C32 t2 = sub(a[0], scl(0.5f, t1)), t3 = scl(kSin3, d);
        a[0] = add(a[0], t1);
        a[1] = C32{t2.x + t3.y, t2.y - t3.x};
        a[2] = C32{t2.x - t3.y, t2.y + t3.x};
    } else if (R == 4) {
        const C32 t0 = add(a[0], a[2]), t1 = sub(a[0], a[2]), t2 = add(a[1], a[3]);
        const C32 t3 = C32{a[1].y - a[3].y, a[3].x - a[1].x};
        a[0] = add(t0, t2);
        a[1] = add(t1, t3);
        a[2] = sub(t0, t2);
        a[3] = sub(t1, t3);
    } else {
        const C32 b1 = add(a[1], a[4]), b2 = add(a[2], a[3]), d1 = sub(a[1], a[4]), d2 = sub(a[2], a[3]);
        const C32 m1 = add(add(a[0], scl(kCos5a, b1)), scl(kCos5b, b2)), m2 = add(add(a[0], scl(kCos5b, b1)), scl(kCos5a, b2));
        const C32 n1 = add(scl(kSin5a, d1), scl(kSin5b, d2)), n2 = sub(scl(kSin5b, d1), scl(kSin5a, d2));
        a[0] = add(add(a[0], b1), b2);
        a[1] = C32{m1.x + n1.y, m1.y - n1.x};
        a[4] = C32{m1.x - n1.y, m1.y + n1.x};
        a[2] = C32{m2.x + n2.y, m2.y - n2.x};
        a[3] = C32{m2.x - n2.y, m2.y + n2.x};
    }
}

// The load and the passes of one row in float, with the kernel's indices and the forward twiddle table; `cols` is the row as it lies
// in memory (bin k in column (k + n / 2) mod n when shifted); returns the row (re, im) = fl32(z.y * c), fl32(z.x * c).
static long g_folds = 0;
static std::vector<C32> replay_transform(const BhwIstftCmfftPlan &pl, const std::vector<C32> &cols)
{
    const uint32_t n = pl.n, fold = pl.fold, lpf = pl.lpf;
    const double pi = 3.14159265358979323846;
    std::vector<C32> tw(fold), A(n), Bf(n);
    for (uint32_t k = 0; k < fold; ++k) tw[k] = C32{(float)cos(2.0 * pi * k / n), (float)-sin(2.0 * pi * k / n)};
    C32 *src = A.data(), *dst = Bf.data();
    std::vector<int> hit(n, 0), readY(n, 0);
    const uint32_t turn = pl.shifted ? n >> 1 : 0u;
    for (uint32_t l = 0; l < lpf; ++l)
        for (uint32_t c = 0; c < pl.cpl; ++c) {
            const uint32_t k = c * lpf + l;
            if (!(k < n)) {                                               // the cols mask: only a lane's last column may be missing
                REQUIRE(c + 1 == pl.cpl, "column %u of %u missing at lane %u", c, pl.cpl, l);
                continue;
            }
            uint32_t col = k + turn;
            col = col >= n ? col - n : col;
            REQUIRE(col < n && col == (k + (pl.shifted ? n / 2 : 0)) % n, "bin %u read from column %u", k, col);
            src[k] = C32{cols[col].y, cols[col].x};                      // the swap
            ++hit[k];
            ++readY[col];
        }
    for (uint32_t i = 0; i < n; ++i) REQUIRE(hit[i] == 1 && readY[i] == 1, "load: point %u written %d times, column read %d times", i, hit[i], readY[i]);
    uint32_t Ns = 1, rest = n;
    for (uint32_t p = 0; p < pl.passes; ++p) {
        const uint32_t R = pl.radix[p];
        REQUIRE(rest % R == 0, "pass %u of radix %u over %u", p, R, rest);
        rest /= R;
        const uint32_t Q = n / R, ts = rest;
        REQUIRE((uint64_t)ts * R * Ns == n && Ns < 2048u, "twiddle stride %u", ts);
        std::vector<int> rd(n, 0), wr(n, 0);
        const float inv = 1.0f / (float)Ns;
        const float inv_lo = nextafterf(inv, 0.0f), inv_hi = nextafterf(inv, 2.0f);   // the hardware's reciprocal is not correctly rounded
        for (uint32_t l = 0; l < lpf; ++l)
            for (uint32_t i = l; i < Q; i += lpf) {
                C32 a[5];
                for (uint32_t q = 0; q < R; ++q) {
                    REQUIRE(i + q * Q < n, "read %u", i + q * Q);
                    ++rd[i + q * Q];
                    a[q] = src[i + q * Q];
                }
                uint32_t k = i;
                if (Ns < Q) {
                    const uint32_t d = (uint32_t)(((float)i + 0.5f) * inv);
                    REQUIRE(d == i / Ns && d == (uint32_t)(((float)i + 0.5f) * inv_lo) && d == (uint32_t)(((float)i + 0.5f) * inv_hi), "%u / %u", i, Ns);
                    k = i - d * Ns;
                } else {
                    REQUIRE(Ns == Q && p + 1 == pl.passes, "k = i outside the last pass");
                }
                if (Ns > 1u) {
                    const uint32_t kt = k * ts;
                    for (uint32_t q = 1; q < R; ++q) {
                        const uint32_t idx = q * kt;
                        REQUIRE(idx < n, "twiddle index %u of %u", idx, n);
                        const bool hi = idx >= fold;
                        REQUIRE(!hi || !(n & 1u), "a fold at the odd n %u", n);
                        const uint32_t at = hi ? idx - fold : idx;
                        REQUIRE(at < fold, "folded twiddle index %u", at);
                        g_folds += hi;
                        a[q] = cmul(a[q], hi ? C32{-tw[at].x, -tw[at].y} : tw[at]);
                    }
                }
                butterfly(R, a);
                const uint32_t o = (i - k) * R + k;
                for (uint32_t q = 0; q < R; ++q) {
                    REQUIRE(o + q * Ns < n, "write %u", o + q * Ns);
                    ++wr[o + q * Ns];
                    dst[o + q * Ns] = a[q];
                }
            }
        for (uint32_t i = 0; i < n; ++i) REQUIRE(rd[i] == 1 && wr[i] == 1, "n_fft %u pass %u point %u read %d written %d", n, p, i, rd[i], wr[i]);
        std::swap(src, dst);
        Ns *= R;
    }
    REQUIRE(Ns == n && rest == 1, "the passes transform %u of %u points", Ns, n);
    const float scale = (float)(1.0 / (double)n);
    std::vector<C32> row(n);
    for (uint32_t i = 0; i < n; ++i) row[i] = C32{src[i].y * scale, src[i].x * scale};   // the swap back, one multiply per part
    return row;
}

// The group loop, the frame walk, the ring and the stores of every lane.  An accumulator is the list of the (f, k) it was given.
typedef std::vector<std::pair<uint64_t, uint32_t>> Terms;
static void replay_spans(const BhwIstftCmfftPlan &pl, const bhw_stft &s, uint64_t L)
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
    const uint32_t turn = pl.shifted ? (uint32_t)(n / 2) : 0u, hm = (uint32_t)(hop % n);
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
                uint32_t bm = (uint32_t)((r.f_lo * hop) % n);
                for (uint64_t it = 0; it < pl.trips; ++it) {
                    const uint64_t f = r.f_lo + it;
                    if (f < r.f_hi) {
                        REQUIRE(bm == (uint32_t)(((unsigned __int128)f * hop) % n), "stepped base mod n: %u at frame %" PRIu64, bm, f);
                        for (uint32_t l = 0; l < pl.lpf; ++l) {
                            const uint32_t tid = slot * pl.lpf + l;
                            for (uint32_t c = 0; c < pl.cpl; ++c) {
                                if (!(c * pl.lpf + l < n)) continue;
                                uint64_t col = c * pl.lpf + l + turn;
                                col = col >= n ? col - n : col;
                                const uint64_t y0 = b * pl.y_bstride + f * pl.y_stride;
                                REQUIRE(y0 + 2 * col + 2 <= yext && 2 * col + 2 <= 2 * n, "Y index");
                            }
                            const uint64_t base = f * hop;
                            uint64_t c0 = cur[l];
                            if (c0 < base) {
                                for (uint64_t w = c0 + l; w < base; w += pl.lpf) store(b, w, Terms());
                                c0 = base;
                            }
                            uint64_t end = (f + 1 == r.f_hi || base + hop > r.whi) ? r.whi : base + hop;
                            if (end < c0) end = c0;
                            for (uint32_t c = 0; c < pl.cpl; ++c) {
                                const uint32_t q = c * pl.lpf + l;
                                if (!(q < n)) continue;
                                const uint32_t k = q >= bm ? q - bm : q + (uint32_t)n - bm;
                                REQUIRE(k < n && (base + k) % n == q, "ring position %u holds k %u", q, k);
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
                    bm += hm;
                    if (bm >= n) bm -= (uint32_t)n;
                }
                for (uint32_t l = 0; l < pl.lpf; ++l) {
                    for (uint64_t w = cur[l] + l; w < r.whi; w += pl.lpf) store(b, w, Terms());
                    for (uint32_t c = 0; c < kCfftMaxCpl; ++c) REQUIRE(ring[(slot * pl.lpf + l) * kCfftMaxCpl + c].empty(), "accumulator left full");
                }
            }
    for (uint64_t i = 0; i < pool; ++i) REQUIRE(owned[i] == 1, "span %" PRIu64 " owned %d times", i, owned[i]);
    for (uint64_t i = 0; i < stored.size(); ++i) REQUIRE(stored[i] == 1, "output %" PRIu64 " stored %d times", i, stored[i]);
}

static long g_span_replays = 0, g_cut = 0;
// one geometry: checks, plan, invariants, describe, the ring replay.  padded: 0 packed, 1 gaps on the 8-byte grid, 2 an odd x_stride
static void geometry(const bhw_params *p, uint64_t n, uint64_t L, uint64_t hop, uint64_t B, uint64_t F, bool centred, int64_t extra, int padded,
                     uint32_t flags, bool replay)
{
    char buf[1100];
    const uint64_t xa = 0x10000000ull, ya = 0x100000000000ull;
    const uint64_t pad = centred ? n / 2 : 0, col0 = (n - L) / 2, full = n + hop * (F - 1);
    if (full <= 2 * pad || (int64_t)(full - 2 * pad) + extra < 1 || pad < col0) return;
    const uint64_t T = full - 2 * pad + extra;
    bhw_stft s = desc_of(B, T, F, hop, n, col0, pad);
    if (padded) {
        s.x_stride = padded == 1 ? 2 * (T + 5) : 2 * T + 3;
        s.y_stride = 2 * n + 6;
        s.y_batch_stride = F * s.y_stride + 10;
    }
    int rc = bhwp_istft_cmfft_checks(p, L, &s, flags, nullptr, nullptr, false);
    REQUIRE(rc == BHW_OK, "checks rc %d: n %" PRIu64 " L %" PRIu64 " hop %" PRIu64 " B %" PRIu64 " F %" PRIu64, rc, n, L, hop, B, F);
    rc = bhwp_istft_cmfft_checks(p, L, &s, flags, (const void *)ya, (const void *)(xa + (padded == 2 ? 4 : 0)));
    REQUIRE(rc == BHW_OK, "pointer checks rc %d", rc);
    const BhwIstftCmfftPlan pl = bhwp_istft_cmfft_plan(p, L, &s, flags, (B + F) % 2 == 0);
    plan_invariants(pl, s, L, p);
    REQUIRE(pl.normalize == ((flags & BHW_OLA_NORMALIZE) != 0) && pl.shifted == ((flags & BHW_CFFT_SHIFT) != 0), "flags in the plan");
    REQUIRE(bhwp_describe_istft_cmfft(p, nullptr, L, &s, flags, buf, sizeof buf) == BHW_OK && strlen(buf) > 40 && strlen(buf) < sizeof buf - 1, "describe");
    REQUIRE(!strncmp(buf, "istft cmfft direct", 18) && strstr(buf, " twiddles"), "%s", buf);
    if (replay) {
        replay_spans(pl, s, L);
        ++g_span_replays;
        if (pl.spans > 1) ++g_cut;
    }
}

int main()
{
    char buf[1100];
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 12, 24);
    const uint64_t xa = 0x10000000ull, ya = 0x100000000000ull;
    const double pi = 3.14159265358979323846;
    long sizes = 0, odd = 0, refused = 0, pass_replays = 0;
    double worst_share = 0.0;
    for (uint64_t n = 1; n <= 5000; ++n) {
        bhw_stft s = desc_of(1, n, 1, 1, n, 0, 0);
        const int rc = bhwp_istft_cmfft_checks(&p, n < 16 ? n : 16, &s, 5, nullptr, nullptr, false);
        REQUIRE(bhwp_cmfft_supported(n) == supported(n) && rc == (supported(n) ? BHW_OK : BHW_ERR_UNSUPPORTED), "n_fft %" PRIu64 ": rc %d", n, rc);
        if (!supported(n)) {
            ++refused;
            continue;
        }
        ++sizes;
        odd += n & 1;
        // the load and the passes in float against a direct binary64 inverse DFT of the float32 bins, shifted and in order
        std::vector<double> cs(n), sn(n);
        for (uint64_t k = 0; k < n; ++k) {
            cs[k] = cos(2.0 * pi * (double)k / (double)n);
            sn[k] = sin(2.0 * pi * (double)k / (double)n);
        }
        for (int trial = 0; trial < 2; ++trial) {
            s = desc_of(1, n, 1, 1, n, 0, 0);
            const uint32_t flags = trial ? BHW_CFFT_SHIFT : 0u;
            const BhwIstftCmfftPlan pl = bhwp_istft_cmfft_plan(&p, n, &s, flags, false);
            plan_invariants(pl, s, n, &p);
            std::vector<C32> bins(n), cols(n);
            for (uint64_t k = 0; k < n; ++k) bins[k] = C32{(float)(unit() * 2000.0), (float)(unit() * 2000.0)};
            for (uint64_t k = 0; k < n; ++k) cols[(k + (flags ? n / 2 : 0)) % n] = bins[k];   // what the forward call stores under the flag
            const std::vector<C32> row = replay_transform(pl, cols);
            double ne = 0, nr = 0;
            for (uint64_t j = 0; j < n; ++j) {
                double re = 0, im = 0;
                for (uint64_t k = 0; k < n; ++k) {
                    const uint64_t at = (j * k) % n;
                    re += (double)bins[k].x * cs[at] - (double)bins[k].y * sn[at];
                    im += (double)bins[k].y * cs[at] + (double)bins[k].x * sn[at];
                }
                re /= (double)n;
                im /= (double)n;
                ne += ((double)row[j].x - re) * ((double)row[j].x - re) + ((double)row[j].y - im) * ((double)row[j].y - im);
                nr += re * re + im * im;
            }
            const double err = sqrt(ne / nr), cap = ldexp(log2((double)n), -24);
            REQUIRE(err <= cap, "n %" PRIu64 " trial %d: relative l2 error %.3e above the cap %.3e", n, trial, err, cap);
            if (err / cap > worst_share) worst_share = err / cap;
            ++pass_replays;
        }
        // a small sweep of the ring at every size: windows, hops and lengths at the edges, all four flag combinations
        uint32_t fl = (uint32_t)(n % 4);
        for (uint64_t L : {(uint64_t)1, n / 2 + 1, n})
            for (uint64_t hop : {(uint64_t)7, n / 4 + 3, n + 5}) {
                const uint32_t flags = (fl & 1u ? BHW_OLA_NORMALIZE : 0u) | (fl & 2u ? BHW_CFFT_SHIFT : 0u);
                const uint64_t F = n <= 100 ? 40 : n <= 600 ? 12 : 5;
                geometry(&p, n, L, hop, n <= 100 ? 3 : 1, F, true, (int64_t)(fl % 3) * 9 - 9, (int)(fl % 3), flags, true);
                ++fl;
            }
    }
    REQUIRE(sizes == 91 && odd == 18 && refused == 4909 && pass_replays == 182 && g_folds > 0, "sizes %ld odd %ld refused %ld", sizes, odd, refused);
    // the geometries of tests/istft_cmfft_cases.py: (n, L, hop, B, F, centred, extra, padded, flags)
    struct Case {
        uint64_t n, L, hop, B, F;
        bool centred;
        int64_t extra;
        int padded;
        uint32_t flags;
    };
    const Case cases[] = {
        {18, 13, 5, 3, 18, true, 0, 0, 1},         {25, 25, 12, 13, 4, true, -1, 0, 4},     {27, 20, 7, 3, 40, true, -9, 2, 1},
        {48, 48, 4, 9, 6, true, 90, 0, 1},         {75, 75, 29, 2, 44, false, 0, 0, 1},     {100, 90, 37, 4, 50, true, 300, 1, 5},
        {100, 40, 300, 11, 5, true, 0, 1, 1},      {400, 400, 160, 2, 26, true, 0, 0, 1},   {1000, 900, 300, 3, 17, true, 0, 0, 0},
        {1215, 1215, 400, 5, 12, false, 0, 0, 5},  {1280, 1000, 700, 7, 8, true, 0, 0, 1},  {1458, 1458, 365, 5, 12, true, 0, 0, 1},
        {1536, 1200, 384, 4, 16, true, 0, 0, 5},   {2000, 100, 200, 1, 2047, true, 1000, 0, 1}, {2000, 2000, 16, 1, 1100, true, 0, 0, 1},
        {2025, 2025, 506, 5, 12, true, 0, 0, 1},
    };
    for (const Case &c : cases) geometry(&p, c.n, c.L, c.hop, c.B, c.F, c.centred, c.extra, c.padded, c.flags, !(c.n == 2000 && c.hop == 16));
    // a heavier sweep at a few sizes: batch, frames, tails and strides
    for (uint64_t n : {18ull, 75ull, 100ull})
        for (uint64_t L : {(uint64_t)1, (uint64_t)13, n / 2 + 1, n - 1, n})
            for (uint64_t hop : {(uint64_t)1, (uint64_t)7, n / 4 + 3, n, n + 5})
                for (uint64_t B : {1ull, 3ull, 70ull})
                    for (uint64_t F : {1ull, 2ull, 65ull, 700ull})
                        for (int centred = 0; centred <= 1; ++centred)
                            for (int tail = 0; tail < 3; ++tail)
                                for (int padded = 0; padded <= 2; ++padded) {
                                    const uint64_t full = n + hop * (F - 1), pad = centred ? n / 2 : 0;
                                    if (full <= 2 * pad) continue;
                                    const int64_t extra = tail == 0 ? 0 : tail == 1 ? -(int64_t)(full - 2 * pad > 5 ? 5 : 0) : (int64_t)(n + 2 * hop + 3);
                                    const uint64_t T = full - 2 * pad + extra;
                                    const uint32_t flags = (tail == 0 ? BHW_OLA_NORMALIZE : 0u) | ((B + hop) % 2 ? BHW_CFFT_SHIFT : 0u);
                                    geometry(&p, n, L, hop, B, F, centred != 0, extra, padded, flags, B * (T + F * L) <= 6000 || (B == 1 && F == 700 && hop == 7 && L == 13));
                                }
    // a hop past every output, up to 2^63: frame 0 alone
    for (uint64_t hop : {5000ull, 1ull << 40, 1ull << 63}) {
        bhw_stft s = desc_of(2, 700, 3, hop, 250, 25, 125);
        REQUIRE(bhwp_istft_cmfft_checks(&p, 200, &s, 5, nullptr, nullptr, false) == BHW_OK, "hop %" PRIu64, hop);
        const BhwIstftCmfftPlan pl = bhwp_istft_cmfft_plan(&p, 200, &s, 5, false);
        plan_invariants(pl, s, 200, &p);
        replay_spans(pl, s, 200);
    }
    // the refusals and their order
    {
        bhw_stft s = desc_of(4, 16000, 101, 160, 600, 100, 300);
        REQUIRE(bhwp_istft_cmfft_checks(&p, 400, &s, 5, (const void *)ya, (const void *)xa) == BHW_OK, "the good call");
        REQUIRE(bhwp_istft_cmfft_checks(&p, 400, &s, 0, (const void *)(ya + 4), (const void *)xa) == BHW_ERR_BADARG, "misaligned Y");
        REQUIRE(bhwp_istft_cmfft_checks(&p, 400, &s, 0, (const void *)ya, (const void *)(xa + 2)) == BHW_ERR_BADARG, "misaligned x");
        REQUIRE(bhwp_istft_cmfft_checks(&p, 400, &s, 0, (const void *)ya, (const void *)ya) == BHW_ERR_BADARG, "overlap");
        for (uint32_t flags : {2u, 3u, 8u, 16u, 1u << 31}) REQUIRE(bhwp_istft_cmfft_checks(&p, 400, &s, flags, nullptr, nullptr, false) == BHW_ERR_BADARG, "flags");
        bhw_stft bad = s;
        bad.y_stride = 1198;
        REQUIRE(bhwp_istft_cmfft_checks(&p, 400, &bad, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "short y_stride");
        bad.y_stride = 1203;
        REQUIRE(bhwp_istft_cmfft_checks(&p, 400, &bad, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "odd y_stride");
        bad = s;
        bad.y_batch_stride = 101 * 1200 + 1;
        REQUIRE(bhwp_istft_cmfft_checks(&p, 400, &bad, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "odd y_batch_stride");
        bad = s;
        bad.x_stride = 31999;
        REQUIRE(bhwp_istft_cmfft_checks(&p, 400, &bad, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "short x_stride");
        bad = s;
        bad.channels = 1;
        REQUIRE(bhwp_istft_cmfft_checks(&p, 400, &bad, 0, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED && strstr(bhw_last_error(), "bhw_istft_mfft_f32_*"), "channels");
        bad = s;
        bad.n_fft = 512;
        bad.col0 = 56;
        bad.pad = 256;
        REQUIRE(bhwp_istft_cmfft_checks(&p, 400, &bad, 0, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED && strstr(bhw_last_error(), "bhw_istft_cfft_f32_*"), "a power of two");
        bad = s;
        bad.pad_mode = BHW_PAD_REFLECT;
        REQUIRE(bhwp_istft_cmfft_checks(&p, 400, &bad, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "pad_mode");
        bad = s;
        bad.samples = 0;
        bad.y_stride = 3;                                                 // samples 0: the strides are not looked at
        REQUIRE(bhwp_istft_cmfft_checks(&p, 400, &bad, 4, nullptr, nullptr) == BHW_OK, "samples 0");
        REQUIRE(bhwp_describe_istft_cmfft(&p, nullptr, 400, &bad, 0, buf, sizeof buf) == BHW_OK && strstr(buf, "nothing (samples 0)"), "describe samples 0");
        // the order: a descriptor error before an unknown flag, an unknown flag before the unsupported channels and n_fft
        s = desc_of(1, 100, 4, 0, 700, 0, 350);
        s.channels = 1;
        REQUIRE(bhwp_istft_cmfft_checks(&p, 16, &s, 8, nullptr, nullptr, false) == BHW_ERR_BADARG && strstr(bhw_last_error(), "hop"), "hop 0 first");
        s.hop = 16;
        REQUIRE(bhwp_istft_cmfft_checks(&p, 16, &s, 8, nullptr, nullptr, false) == BHW_ERR_BADARG && strstr(bhw_last_error(), "flags"), "then the flags");
        REQUIRE(bhwp_istft_cmfft_checks(&p, 16, &s, 4, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED && strstr(bhw_last_error(), "channels"), "then the channels");
        s.channels = 2;
        REQUIRE(bhwp_istft_cmfft_checks(&p, 16, &s, 4, nullptr, nullptr, false) == BHW_ERR_UNSUPPORTED && strstr(bhw_last_error(), "n_fft 700"), "then n_fft");
    }
    REQUIRE(bhwp_istft_cmfft_checks(&p, 16, nullptr, 0, nullptr, nullptr, false) == BHW_ERR_BADARG, "NULL descriptor");
    REQUIRE(g_span_replays > 1500 && g_cut > 200, "replays %ld (%ld cut into spans)", g_span_replays, g_cut);
    printf("ok %ld checks, %ld sizes, %ld odd, %ld refused, %ld span replays (%ld of signals cut into several spans), %ld pass replays, worst error %.3f "
           "of the cap\n", g_checks, sizes, odd, refused, g_span_replays, g_cut, pass_replays, worst_share);
    return 0;
}
