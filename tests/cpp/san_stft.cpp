// san_stft.cpp -- the planner's part of the batched, centred STFT framing and overlap-add (bhw_plan.cpp: bhwp_stft_checks,
// bhwp_stft_plan, bhwp_stft_ola, bhwp_describe_stft) swept under AddressSanitizer + UBSan over B, T, n_fft, L, col0, pad, hop, C and
// both pad modes.  Besides "no report", it replays on the host
//   - the lane and row-pool arithmetic of stft_loop (bhw_stft.h): every (b, f, j) of every row is written exactly once, and the
//     window columns read the time index t' of the contract (reflect or constant);
//   - the reflect map against a direct restatement for every T <= 64, pad <= T - 1 and t in [-pad, T + pad);
//   - the batched overlap-add (ola_f32_loop with grid z over the signals, bhw_ola_f32.h): every product is summed once, in ascending
//     frame order per output, and never across signals.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "bhw_plan.h"

static long g_checks = 0;
#define REQUIRE(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static bhw_stft stft_of(uint64_t B, uint64_t T, uint64_t frames, uint64_t hop, uint64_t n_fft, uint64_t col0, uint64_t pad, uint32_t mode,
                        uint32_t C)
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
    s.col0 = col0;
    s.pad = pad;
    s.pad_mode = mode;
    s.shift = 15;
    return s;
}

// the contract's t' (bhw.h), restated directly: -1 for a constant-mode zero
static int64_t t_contract(int64_t t, int64_t T, uint32_t mode)
{
    if (t >= 0 && t < T) return t;
    if (mode == BHW_PAD_CONSTANT) return -1;
    return t < 0 ? -t : 2 * (T - 1) - t;
}

// stft_loop's index arithmetic: one unsigned range test, the reflect map only where it fails
static int64_t t_kernel(uint64_t f, uint64_t hop, uint64_t j, uint64_t pad, uint64_t T, uint32_t mode)
{
    uint64_t t = f * hop + j - pad;
    if (t >= T) {
        const int64_t ts = (int64_t)t;
        if (mode == BHW_PAD_REFLECT) t = ts < 0 ? (uint64_t)(-ts) : 2 * (T - 1) - t;
        else return -1;
    }
    return (int64_t)t;
}

// every lane of the grid, every row of its row blocks, in the kernel's order (stft_step's (b, f) stepping)
static void replay_frames(const BhwStftPlan &pl, const bhw_stft &s, uint64_t L)
{
    const uint64_t F = s.frames, B = s.batch, N = s.n_fft;
    std::vector<int> writes(B * F * N, 0);
    const uint64_t span = pl.group * pl.fy;
    for (uint64_t bx = 0; bx < pl.grid_x; ++bx)
        for (uint64_t gy = 0; gy < pl.grid_y; ++gy)
            for (uint32_t tid = 0; tid < kFramesBlock; ++tid) {
                const uint64_t j = bx * pl.kx + (tid & (pl.kx - 1u));
                const uint32_t ty = tid / pl.kx;
                if (j >= N) continue;
                const bool in = (uint32_t)(j - s.col0) < L;
                REQUIRE(in == (j >= s.col0 && j < s.col0 + L), "j %" PRIu64, j);
                for (uint64_t by = gy; by < pl.row_blocks; by += pl.grid_y) {
                    const uint64_t r_beg = by * span + ty, r_end = (by + 1) * span < pl.rows ? (by + 1) * span : pl.rows;
                    if (r_beg >= r_end) continue;
                    uint64_t b = r_beg / F, f = r_beg - b * F;
                    for (uint64_t r = r_beg; r < r_end; r += pl.fy) {
                        REQUIRE(b * F + f == r && f < F && b < B, "row %" PRIu64 " -> (%" PRIu64 ", %" PRIu64 ")", r, b, f);
                        ++writes[(b * F + f) * N + j];
                        if (in) {
                            const int64_t t = (int64_t)(f * s.hop + j) - (int64_t)s.pad;
                            const int64_t tk = t_kernel(f, s.hop, j, s.pad, s.samples, s.pad_mode);
                            REQUIRE(tk == t_contract(t, (int64_t)s.samples, s.pad_mode), "t %" PRId64, t);
                            REQUIRE(tk < (int64_t)s.samples, "t' %" PRId64, tk);
                        }
                        f += pl.step_f;                             // stft_step
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

// ola_f32_loop over grid z = the signals, restated as san_f32.cpp restates it, with the row offset col0 * C and the batch strides
static void replay_ola(const BhwOlaPlan &pl, const bhw_ola &o, const BhwOlaBatch &bt, const bhw_stft &s, uint64_t N)
{
    const uint64_t C = s.channels, T = o.count;
    std::vector<int> visits(bt.batch * T * N, 0);
    std::vector<int64_t> last_f(bt.batch * T, -1);
    const uint64_t rlim = N - (pl.jmax - 1) * o.hop;
    const int64_t frames = (int64_t)o.frames;
    const uint64_t ysig = (s.frames - 1) * o.y_stride + s.n_fft * C;
    for (uint64_t b0 = 0; b0 < bt.batch; b0 += kOlaMaxGridZ)
        for (uint64_t bz = 0; bz < bt.batch - b0 && bz < kOlaMaxGridZ; ++bz)
            for (uint64_t bx = 0; bx < pl.grid_x; ++bx)
                for (uint64_t gy = 0; gy < pl.grid_y; ++gy)
                    for (uint32_t tid = 0; tid < kOlaBlock; ++tid) {
                        const uint64_t b = b0 + bz;
                        const uint32_t ty = tid / pl.rx;
                        const uint64_t sl = bx * pl.rx + (tid & (pl.rx - 1u));
                        const bool lane_ok = sl < pl.lanes;
                        uint64_t r = pl.r0 + sl;
                        int64_t qb = (int64_t)pl.q0;
                        if (r >= o.hop) { r -= o.hop; ++qb; }
                        const int64_t jr = (!lane_ok || r >= N) ? 0 : (r < rlim ? (int64_t)pl.jmax : (int64_t)pl.jmax - 1);
                        for (uint64_t by = gy; by < pl.row_blocks; by += pl.grid_y) {
                            const uint64_t ia = (by * pl.fy + ty) * pl.q;
                            const uint64_t u0 = ia < pl.rows ? ia * o.hop + sl : o.count;
                            uint32_t nrow = 0;
                            if (lane_ok && u0 < o.count) {
                                const uint64_t left = (o.count - u0 - 1) / o.hop + 1;
                                nrow = left < pl.q ? (uint32_t)left : pl.q;
                            }
                            const int64_t qa = qb + (int64_t)ia;
                            const int64_t jlo = qa - frames + 1 > 0 ? qa - frames + 1 : 0;
                            const int64_t jhi = (qa + (int64_t)nrow - 1) < jr - 1 ? qa + (int64_t)nrow - 1 : jr - 1;
                            const uint32_t trip = (nrow && jhi >= jlo) ? (uint32_t)(jhi - jlo + 1) : 0u;
                            for (uint32_t n = 0; n < trip; ++n) {
                                const int64_t j = jhi - (int64_t)n;
                                const uint64_t k = r + (uint64_t)j * o.hop;
                                REQUIRE(k < N, "k %" PRIu64, k);
                                for (uint32_t i = 0; i < nrow; ++i) {
                                    const int64_t f = qa - j + (int64_t)i;
                                    if (f < 0 || f >= frames) continue;
                                    const uint64_t u = u0 + (uint64_t)i * o.hop;
                                    // the element read and the output written stay inside signal b
                                    const uint64_t yi = b * bt.y_bstride + s.col0 * C + (uint64_t)f * o.y_stride + k * C;
                                    const uint64_t xi = b * bt.x_bstride + u * C;
                                    REQUIRE(yi >= b * bt.y_bstride && yi + C <= b * bt.y_bstride + ysig, "y index %" PRIu64, yi);
                                    REQUIRE(xi >= b * bt.x_bstride && xi + C <= b * bt.x_bstride + T * C, "x index %" PRIu64, xi);
                                    REQUIRE(u < T && u + s.pad == (uint64_t)f * o.hop + s.col0 + k, "u %" PRIu64, u);
                                    REQUIRE(f > last_f[b * T + u], "signal %" PRIu64 " output %" PRIu64 ": frame %" PRId64 " after %" PRId64, b, u, f,
                                            last_f[b * T + u]);
                                    last_f[b * T + u] = f;
                                    ++visits[(b * T + u) * N + k];
                                }
                            }
                        }
                    }
    for (uint64_t b = 0; b < bt.batch; ++b)
        for (uint64_t u = 0; u < T; ++u)
            for (uint64_t k = 0; k < N; ++k) {
                const uint64_t pt = u + s.pad - s.col0;                        // f * hop + k
                const bool reached = pt >= k && (pt - k) % o.hop == 0 && (pt - k) / o.hop < s.frames;
                REQUIRE(visits[(b * T + u) * N + k] == (reached ? 1 : 0), "b %" PRIu64 " u %" PRIu64 " k %" PRIu64, b, u, k);
            }
}

int main()
{
    char buf[640];
    long frame_replays = 0, ola_replays = 0;
    // the reflect map, every small case
    for (int64_t T = 1; T <= 64; ++T)
        for (int64_t pad = 0; pad <= T - 1; ++pad)
            for (int64_t t = -pad; t < T + pad; ++t) {
                const int64_t want = t < 0 ? -t : t >= T ? 2 * (T - 1) - t : t;
                REQUIRE(t_contract(t, T, BHW_PAD_REFLECT) == want && want >= 0 && want < T, "T %" PRId64 " t %" PRId64, T, t);
                REQUIRE(t_kernel((uint64_t)(t + pad), 1, 0, (uint64_t)pad, (uint64_t)T, BHW_PAD_REFLECT) == want, "T %" PRId64, T);
            }
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 12, 24);
    for (uint64_t B : {1ull, 3ull, 64ull})
        for (uint64_t T : {1ull, 7ull, 33ull, 100ull})
            for (uint64_t n_fft : {1ull, 16ull, 48ull, 64ull, 300ull})
                for (uint64_t L : {1ull, 13ull, 16ull, 48ull, 64ull})
                    for (uint64_t hop : {1ull, 5ull, 16ull, 70ull})
                        for (uint32_t C = 1; C <= 2; ++C)
                            for (uint32_t mode = 0; mode <= 2; ++mode)
                                for (int center = 0; center <= 1; ++center) {
                                    if (L > n_fft && n_fft != 1) continue;
                                    const uint64_t col0 = n_fft >= L ? (n_fft - L) / 2 : 0;
                                    const uint64_t pad = center ? n_fft / 2 : 0;
                                    const uint64_t frames = T + 2 * pad >= n_fft ? 1 + (T + 2 * pad - n_fft) / hop : 0;
                                    bhw_stft s = stft_of(B, T, frames, hop, n_fft, col0, pad, mode, C);
                                    int rc = bhwp_stft_checks(&p, L, &s, false, 0, nullptr, nullptr, false);
                                    const bool want_ok = mode <= 1 && col0 + L <= n_fft && !(frames && mode == BHW_PAD_REFLECT && pad > T - 1);
                                    REQUIRE((rc == BHW_OK) == want_ok, "frames checks rc %d: B %" PRIu64 " T %" PRIu64 " n_fft %" PRIu64 " L %" PRIu64
                                            " mode %u", rc, B, T, n_fft, L, mode);
                                    if (rc == BHW_OK && frames) {
                                        const BhwStftPlan pl = bhwp_stft_plan(&p, L, &s, (B + T) % 2 == 0);
                                        REQUIRE(pl.kx && (pl.kx & (pl.kx - 1)) == 0 && pl.kx * pl.fy == kFramesBlock, "kx %u", pl.kx);
                                        REQUIRE(pl.grid_x * pl.kx >= n_fft && (pl.grid_x - 1) * pl.kx < n_fft, "grid_x");
                                        REQUIRE(pl.rows == B * frames && pl.row_blocks * pl.group * pl.fy >= pl.rows, "rows");
                                        REQUIRE(pl.grid_y >= 1 && pl.grid_y <= kFramesMaxGridY && pl.step_b * frames + pl.step_f == pl.fy, "grid_y");
                                        REQUIRE(bhwp_describe_stft(&p, nullptr, L, &s, false, 0, buf, sizeof buf) == BHW_OK, "describe");
                                        if (B * frames * n_fft <= 200000) {
                                            replay_frames(pl, s, L);
                                            ++frame_replays;
                                        }
                                    }
                                    if (mode != 0 || !center || !frames) continue;
                                    // the inverse of the same framing, length T and T past the extent
                                    for (uint64_t Tout : {T, T + 3 * hop + 5}) {
                                        bhw_stft si = stft_of(B, Tout, frames, hop, n_fft, col0, pad, 0, C);
                                        for (uint32_t flags = 0; flags <= 1; ++flags) {
                                            rc = bhwp_stft_checks(&p, L, &si, true, flags, nullptr, nullptr, false);
                                            REQUIRE((rc == BHW_OK) == (col0 + L <= n_fft && pad >= col0), "ola checks rc %d", rc);
                                            if (rc) continue;
                                            bhw_ola o;
                                            BhwOlaBatch bt;
                                            bhwp_stft_ola(&si, o, bt);
                                            REQUIRE(o.t0 == pad - col0 && o.count == Tout && bt.batch == B, "mapping");
                                            const BhwOlaPlan pl = bhwp_ola_plan(&p, &o, false, 0, 0, L, flags ? kOlaQMaxNorm : kOlaQMax, B);
                                            REQUIRE(bhwp_describe_stft(&p, nullptr, L, &si, true, flags, buf, sizeof buf) == BHW_OK, "describe");
                                            if (B * Tout * L <= 400000) {
                                                replay_ola(pl, o, bt, si, L);
                                                ++ola_replays;
                                            }
                                        }
                                    }
                                }
    REQUIRE(frame_replays > 100 && ola_replays > 100, "replays %ld %ld", frame_replays, ola_replays);
    printf("ok %ld checks, %ld frames replays, %ld overlap-add replays\n", g_checks, frame_replays, ola_replays);
    return 0;
}
