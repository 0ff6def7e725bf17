// san_f32.cpp -- the planner's part of the float32 frame apply and overlap-add (bhw_plan.cpp: bhwp_f32_checks, the float32 frames
// plan, bhwp_describe_f32) swept under AddressSanitizer + UBSan over phi_width 4..30, the models, window lengths, hops, frame counts
// and both channel counts.  Besides "no report", it checks that a float32 frames plan never takes the per-frame route and otherwise has
// the shape of the int32 kernel route, and -- on small windows -- replays the lane arithmetic of ola_f32_loop (bhw_ola_f32.h) to check
// that every (frame, k) product of every output in range is summed exactly once and in ascending frame order (the order is part of
// the float32 contract: binary64 addition does not associate).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "bhw_plan.h"

static long g_checks = 0;
#define REQUIRE(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static bhw_frames frames_of(uint64_t frames, uint64_t hop, uint32_t C, uint64_t ys, uint32_t shift)
{
    bhw_frames f;
    memset(&f, 0, sizeof f);
    f.struct_size = sizeof f;
    f.channels = C;
    f.frames = frames;
    f.hop = hop;
    f.y_stride = ys;
    f.shift = shift;
    return f;
}

static bhw_ola ola_of(uint64_t frames, uint64_t hop, uint32_t C, uint64_t t0, uint64_t count)
{
    bhw_ola o;
    memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.channels = C;
    o.frames = frames;
    o.hop = hop;
    o.t0 = t0;
    o.count = count;
    return o;
}

// The lane arithmetic of ola_f32_loop on the host, for every lane of the grid, in the kernel's trip order: visits[u * N + k] counts
// the visits of the product of output u at window index k, last_f[u] the frame the output was last summed from.  Each product must
// be visited once when frame (t0 + u - k) / hop exists, never otherwise, and the frames of one output must ascend.
static void replay_order(const BhwOlaPlan &pl, const bhw_ola &o, uint64_t N)
{
    std::vector<int> visits(o.count * N, 0);
    std::vector<int64_t> last_f(o.count, -1);
    const uint64_t rlim = N - (pl.jmax - 1) * o.hop;
    const int64_t frames = (int64_t)o.frames;
    for (uint64_t bx = 0; bx < pl.grid_x; ++bx)
        for (uint64_t gy = 0; gy < pl.grid_y; ++gy)
            for (uint32_t tid = 0; tid < kOlaBlock; ++tid) {
                const uint32_t ty = tid / pl.rx;
                const uint64_t s = bx * pl.rx + (tid & (pl.rx - 1u));
                const bool lane_ok = s < pl.lanes;
                uint64_t r = pl.r0 + s;
                int64_t qb = (int64_t)pl.q0;
                if (r >= o.hop) { r -= o.hop; ++qb; }
                const int64_t jr = (!lane_ok || r >= N) ? 0 : (r < rlim ? (int64_t)pl.jmax : (int64_t)pl.jmax - 1);
                for (uint64_t by = gy; by < pl.row_blocks; by += pl.grid_y) {
                    const uint64_t ia = (by * pl.fy + ty) * pl.q;
                    const uint64_t u0 = ia < pl.rows ? ia * o.hop + s : o.count;
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
                        const int64_t j = jhi - (int64_t)n;                  // the kernel's descending j
                        const uint64_t k = r + (uint64_t)j * o.hop;
                        REQUIRE(k < N, "k %" PRIu64, k);
                        for (uint32_t i = 0; i < nrow; ++i) {
                            const int64_t f = qa - j + (int64_t)i;
                            if (f < 0 || f >= frames) continue;
                            const uint64_t u = u0 + (uint64_t)i * o.hop;
                            REQUIRE(u < o.count && o.t0 + u == (uint64_t)f * o.hop + k, "u %" PRIu64, u);
                            REQUIRE(f > last_f[u], "output %" PRIu64 ": frame %" PRId64 " after frame %" PRId64, u, f, last_f[u]);
                            last_f[u] = f;
                            ++visits[u * N + k];
                        }
                    }
                }
            }
    for (uint64_t u = 0; u < o.count; ++u)
        for (uint64_t k = 0; k < N; ++k) {
            const uint64_t t = o.t0 + u;
            const bool reached = t >= k && (t - k) % o.hop == 0 && (t - k) / o.hop < o.frames;
            REQUIRE(visits[u * N + k] == (reached ? 1 : 0), "u %" PRIu64 " k %" PRIu64 " visits %d", u, k, visits[u * N + k]);
        }
}

int main()
{
    char buf[512], tiny[1];
    static const uint64_t kFrames[] = {1, 2, 3, 5, 16, 17, 1000, 1u << 20};
    long replays = 0;
    for (uint32_t model = 0; model <= BHW_MODEL_VHDL; ++model)
        for (uint32_t pw = 4; pw <= 30; ++pw)
            for (uint32_t W = 8; W <= 32; W += 8)
                for (uint32_t sin_type = 0; sin_type <= 2; sin_type += 2)
                    for (uint32_t win : {(uint32_t)BHW_WIN_HANN, (uint32_t)BHW_WIN_BH7}) {
                        bhw_params p;
                        memset(&p, 0, sizeof p);
                        bhw_params_init(&p, win, pw, W);
                        p.model = model;
                        p.sin_type = sin_type;
                        if (bhwp_validate(&p)) continue;
                        const uint64_t P2 = 1ull << pw;
                        for (uint64_t L : {P2, P2 - 1, P2 / 2 + 3, (uint64_t)3}) {
                            const int rc = bhwp_f32_checks(&p, L, 0);
                            if (sin_type != BHW_SIN_CORDIC) { REQUIRE(rc == BHW_ERR_UNSUPPORTED, "taylor rc %d", rc); continue; }
                            REQUIRE(rc == BHW_OK, "rc %d pw %u L %" PRIu64, rc, pw, L);
                            REQUIRE(bhwp_f32_checks(&p, L, BHW_OLA_NORMALIZE) == BHW_OK, "normalize flag");
                            REQUIRE(bhwp_f32_checks(&p, L, 2u) == BHW_ERR_BADARG && bhwp_f32_checks(&p, L, ~0u) == BHW_ERR_BADARG, "flags");
                            const bool any = L != P2;
                            const uint64_t lk = any ? L : 0;                 // the length the run functions pass the planner
                            const uint64_t hops[] = {1, 3, L / 4 ? L / 4 : 1, L, L + 5};
                            for (uint64_t frames : kFrames)
                                for (uint64_t hop : hops)
                                    for (uint32_t C = 1; C <= 2; ++C) {
                                        const bhw_frames f = frames_of(frames, hop, C, 0, (uint32_t)(frames % 63));
                                        if (bhwp_frames_checks(&p, &f, nullptr, nullptr, false, L) != BHW_OK) {
                                            REQUIRE(frames * L > (1ull << 34), "frames check pw %u L %" PRIu64, pw, L);
                                            continue;
                                        }
                                        for (int from_table = 0; from_table <= 1; ++from_table) {
                                            const BhwFramesPlan pf = bhwp_frames_plan(&p, &f, from_table != 0, -1, lk, true);
                                            REQUIRE(pf.route == (from_table ? BHWP_FRAMES_TABLE : BHWP_FRAMES_DIRECT), "f32 route %d", pf.route);
                                            // a forced per-frame route is not taken either
                                            REQUIRE(bhwp_frames_plan(&p, &f, from_table != 0, BHWP_FRAMES_PER_FRAME, lk, true).route != BHWP_FRAMES_PER_FRAME, "forced");
                                            // the shape of the int32 kernel route
                                            const BhwFramesPlan pi = bhwp_frames_plan(&p, &f, from_table != 0, from_table ? -1 : BHWP_FRAMES_DIRECT, lk);
                                            REQUIRE(pi.route == pf.route && pi.kx == pf.kx && pi.fy == pf.fy && pi.group == pf.group && pi.grid_x == pf.grid_x &&
                                                    pi.grid_y == pf.grid_y && pi.y_stride == pf.y_stride && pi.len == pf.len, "shape");
                                            REQUIRE(pf.grid_y >= 1 && pf.grid_y <= kFramesMaxGridY && pf.grid_x * pf.kx >= L, "grid");
                                        }
                                        REQUIRE(bhwp_describe_f32(&p, nullptr, L, false, &f, nullptr, 0, buf, sizeof buf) == BHW_OK, "describe");
                                        REQUIRE(strstr(buf, any ? "k_frames_f32_direct_len<" : "k_frames_f32_direct<") && strstr(buf, "f32 frames direct"), "%s", buf);
                                        REQUIRE(bhwp_describe_f32(&p, nullptr, L, false, &f, nullptr, BHW_OLA_NORMALIZE, buf, sizeof buf) == BHW_ERR_BADARG, "frames flags");
                                        REQUIRE(bhwp_describe_f32(&p, nullptr, L, false, &f, nullptr, 0, tiny, sizeof tiny) == BHW_OK && tiny[0] == 0, "tiny");
                                        // overlap-add: the whole extent, plans of the int32 call, the describe text
                                        const unsigned __int128 ext128 = (unsigned __int128)(frames - 1) * hop + L;
                                        if (ext128 > (1ull << 34)) continue;
                                        const uint64_t ext = (uint64_t)ext128;
                                        for (int rv = 0; rv < 2; ++rv) {
                                            const uint64_t t0 = rv == 0 ? 0 : ext / 3;
                                            const uint64_t count = rv == 0 ? ext : ext / 3 + 1;
                                            const bhw_ola o = ola_of(frames, hop, C, t0, count);
                                            if (bhwp_ola_checks(&p, &o, nullptr, nullptr, false, L) != BHW_OK) {
                                                REQUIRE(frames * L > (1ull << 34), "ola check");
                                                continue;
                                            }
                                            for (uint32_t flags : {0u, (uint32_t)BHW_OLA_NORMALIZE}) {
                                                REQUIRE(bhwp_describe_f32(&p, nullptr, L, false, nullptr, &o, flags, buf, sizeof buf) == BHW_OK, "describe ola");
                                                REQUIRE(strstr(buf, any ? "k_ola_f32_direct_len<" : "k_ola_f32_direct<") &&
                                                        strstr(buf, flags ? "normalised by the window envelope" : "not normalised"), "%s", buf);
                                            }
                                            const BhwOlaPlan pl = bhwp_ola_plan(&p, &o, false, 0, 0, lk);
                                            // the normalised kernels hold kOlaQMaxNorm rows: their plans stay inside, otherwise the same rule
                                            const BhwOlaPlan pn = bhwp_ola_plan(&p, &o, false, 0, 0, lk, kOlaQMaxNorm);
                                            REQUIRE(pn.q >= 1 && pn.q <= kOlaQMaxNorm && pn.q == (pl.q < kOlaQMaxNorm ? pl.q : kOlaQMaxNorm), "norm Q %u", pn.q);
                                            REQUIRE(pn.rx == pl.rx && pn.grid_x == pl.grid_x && pn.grid_y <= kOlaMaxGridY, "norm shape");
                                            if (L <= 64 && o.count <= 4096 && W == 32 && model == 0 && win == BHW_WIN_HANN) {
                                                replay_order(pl, o, L);
                                                replay_order(pn, o, L);
                                                for (uint32_t fq : {1u, 3u, kOlaQMax}) {
                                                    replay_order(bhwp_ola_plan(&p, &o, false, fq, 1, lk), o, L);
                                                    replays += 2;
                                                }
                                                ++replays;
                                            }
                                        }
                                    }
                            REQUIRE(bhwp_f32_checks(&p, 0, 0) == BHW_ERR_BADARG && bhwp_f32_checks(&p, P2 + 1, 0) == BHW_ERR_BADARG, "length");
                            REQUIRE(bhwp_describe_f32(&p, nullptr, L, false, nullptr, nullptr, 0, buf, sizeof buf) == BHW_ERR_BADARG, "neither");
                        }
                    }
    REQUIRE(replays > 500, "replays %ld", replays);
    // both descriptors, NULL buffers, NULL params
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 10, 24);
    const bhw_frames f = frames_of(3, 256, 1, 0, 23);
    const bhw_ola o = ola_of(3, 256, 1, 0, 100);
    REQUIRE(bhwp_describe_f32(&p, nullptr, 1024, false, &f, &o, 0, buf, sizeof buf) == BHW_ERR_BADARG, "both");
    REQUIRE(bhwp_describe_f32(&p, nullptr, 1024, false, &f, nullptr, 0, nullptr, 8) == BHW_ERR_BADARG, "NULL buf");
    REQUIRE(bhwp_f32_checks(nullptr, 1024, 0) == BHW_ERR_BADARG, "NULL params");
    // the forced any-length kernels at L = 2^phi_width are named as such
    REQUIRE(bhwp_describe_f32(&p, nullptr, 1024, true, &f, nullptr, 0, buf, sizeof buf) == BHW_OK && strstr(buf, "k_frames_f32_direct_len<"), "%s", buf);
    printf("ok %ld\n", g_checks);
    return 0;
}
