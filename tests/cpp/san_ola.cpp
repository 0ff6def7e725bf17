// san_ola.cpp -- the planner's part of the weighted overlap-add (bhw_plan.cpp: argument checks, Q, lane layout, grid, extent and
// overlap checks, the text of bhw_overlap_add_describe) swept under AddressSanitizer + UBSan over phi_width 4..30, hops 1, 3, N/8,
// N/4, N/2, N, N + 5, frame counts, both channel counts, strides and output ranges.  Besides "no report", it checks that the grid
// covers every residue and row once in whole workgroups inside the launch limits, and -- on the small windows -- replays the lane
// arithmetic of k_ola (bhw_ola.hip) to check that every (frame, k) pair of every output in range is summed exactly once.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "bhw_plan.h"

extern "C" int bhw_dbg_describe_ola_from_table(const bhw_params *p_table, uint32_t table_format, const bhw_params *p_call, const bhw_ola *o,
                                               char *buf, uint64_t len);

static long g_checks = 0;
#define REQUIRE(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static bhw_ola ola_of(uint64_t frames, uint64_t hop, uint32_t C, uint64_t ys, uint64_t t0, uint64_t count, uint32_t shift)
{
    bhw_ola o;
    memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.channels = C;
    o.frames = frames;
    o.hop = hop;
    o.y_stride = ys;
    o.t0 = t0;
    o.count = count;
    o.shift = shift;
    return o;
}

// The lane arithmetic of ola_loop (bhw_ola.hip) on the host, for every lane of the grid: visits[u * N + k] counts the products of
// output u at window index k.  Each one must be visited once when frame (t0 + u - k) / hop exists, never otherwise.
static void replay(const BhwOlaPlan &pl, const bhw_ola &o, uint64_t N)
{
    std::vector<int> visits(o.count * N, 0);
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
                        const int64_t j = jlo + (int64_t)n;
                        const uint64_t k = r + (uint64_t)j * o.hop;
                        REQUIRE(k < N, "k %" PRIu64, k);
                        for (uint32_t i = 0; i < nrow; ++i) {
                            const int64_t f = qa - j + (int64_t)i;
                            if (f < 0 || f >= frames) continue;
                            const uint64_t u = u0 + (uint64_t)i * o.hop;
                            REQUIRE(u < o.count && o.t0 + u == (uint64_t)f * o.hop + k, "u %" PRIu64, u);
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
    char buf[384], tiny[1];
    static const uint64_t kFrames[] = {1, 2, 3, 5, 16, 17, 1000, 16384, 1u << 20};
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
                        const uint64_t N = 1ull << pw;
                        const uint64_t hops[] = {1, 3, N / 8, N / 4, N / 2, N, N + 5};
                        for (uint64_t frames : kFrames)
                            for (uint64_t hop : hops)
                                for (uint32_t C = 1; C <= 2; ++C)
                                    for (int sv = 0; sv < 2; ++sv)
                                        for (int rv = 0; rv < 3; ++rv) {
                                            const uint64_t ys = sv == 0 ? 0 : N * C + 17;
                                            const bool too_many = frames * N > (1ull << 34);
                                            const unsigned __int128 ext128 = (unsigned __int128)(frames - 1) * hop + N;
                                            const uint64_t ext = ext128 > (1ull << 34) ? 0 : (uint64_t)ext128;
                                            // output ranges: the whole extent, a middle block, the last few outputs
                                            const uint64_t t0 = rv == 0 ? 0 : rv == 1 ? ext / 3 : (ext > 7 ? ext - 7 : 0);
                                            const uint64_t count = rv == 0 ? ext : rv == 1 ? ext / 3 + 1 : ext - t0;
                                            const bhw_ola o = ola_of(frames, hop, C, ys, t0, count ? count : 1, (uint32_t)(frames % 63));
                                            const int rc = bhwp_ola_checks(&p, &o, (const void *)0x1000, (const void *)0x1000, false);
                                            if (sin_type != BHW_SIN_CORDIC) { REQUIRE(rc == BHW_ERR_UNSUPPORTED, "rc %d", rc); continue; }
                                            if (too_many || !ext) {
                                                REQUIRE(rc == BHW_ERR_BADARG, "frames * N / extent > 2^34 pw %u frames %" PRIu64, pw, frames);
                                                continue;
                                            }
                                            REQUIRE(rc == BHW_OK, "rc %d pw %u frames %" PRIu64 " hop %" PRIu64, rc, pw, frames, hop);
                                            // the same pointers for x and y overlap whenever there is something to do
                                            REQUIRE(bhwp_ola_checks(&p, &o, (const void *)0x1000, (const void *)0x1000) == BHW_ERR_BADARG, "overlap");
                                            // one past the extent
                                            const bhw_ola past = ola_of(frames, hop, C, ys, t0, ext - t0 + 1, 0);
                                            REQUIRE(bhwp_ola_checks(&p, &past, nullptr, nullptr, false) == BHW_ERR_BADARG, "past the extent");
                                            for (int from_table = 0; from_table <= 1; ++from_table) {
                                                const BhwOlaPlan pl = bhwp_ola_plan(&p, &o, from_table != 0);
                                                REQUIRE(pl.route == (from_table ? BHWP_OLA_TABLE : BHWP_OLA_DIRECT), "route");
                                                REQUIRE(pl.y_stride == (ys ? ys : N * C), "stride");
                                                REQUIRE(pl.q0 * hop + pl.r0 == o.t0 && pl.r0 < hop, "t0 split");
                                                REQUIRE(pl.jmax >= 1 && pl.jmax * hop >= N && (pl.jmax - 1) * hop < N, "jmax");
                                                REQUIRE(pl.rx * pl.fy == kOlaBlock && (pl.rx & (pl.rx - 1)) == 0, "block shape");
                                                REQUIRE(pl.q >= 1 && pl.q <= kOlaQMax, "Q %u", pl.q);
                                                REQUIRE(pl.lanes == (hop < o.count ? hop : o.count) && pl.rows * hop >= o.count && (pl.rows - 1) * hop < o.count, "rows");
                                                REQUIRE(pl.grid_x * pl.rx >= pl.lanes && (pl.grid_x - 1) * pl.rx < pl.lanes && pl.grid_x < (1ull << 31), "grid x");
                                                const uint64_t per_wg = (uint64_t)pl.fy * pl.q;
                                                REQUIRE(pl.row_blocks * per_wg >= pl.rows && (pl.row_blocks - 1) * per_wg < pl.rows, "row blocks");
                                                REQUIRE(pl.grid_y >= 1 && pl.grid_y <= kOlaMaxGridY && pl.grid_y <= pl.row_blocks, "grid y");
                                                // forced shapes stay inside the same limits
                                                for (uint32_t fq : {1u, 5u, kOlaQMax})
                                                    for (uint32_t frx : {1u, 64u, kOlaBlock}) {
                                                        const BhwOlaPlan pf = bhwp_ola_plan(&p, &o, from_table != 0, fq, frx);
                                                        REQUIRE(pf.q == fq && pf.rx == frx && pf.grid_y <= kOlaMaxGridY && pf.grid_x < (1ull << 31), "forced");
                                                        if (N <= 64 && o.count <= 4096 && from_table == 0 && W == 32 && model == 0 && win == BHW_WIN_HANN) {
                                                            replay(pf, o, N);
                                                            ++replays;
                                                        }
                                                    }
                                                if (N <= 64 && o.count <= 4096 && from_table == 0 && W == 32 && model == 0) {
                                                    replay(pl, o, N);
                                                    ++replays;
                                                }
                                            }
                                            // describe: truncation safe
                                            REQUIRE(bhwp_describe_ola(&p, nullptr, &o, buf, sizeof buf) == BHW_OK, "describe");
                                            REQUIRE(strlen(buf) > 10 && strlen(buf) < sizeof buf && strstr(buf, "k_ola_direct<"), "%s", buf);
                                            REQUIRE(bhwp_describe_ola(&p, nullptr, &o, tiny, sizeof tiny) == BHW_OK && tiny[0] == 0, "tiny");
                                            if (frames == 5 && hop == N / 2 && W == 32 && rv == 0) {
                                                REQUIRE(bhw_dbg_describe_ola_from_table(&p, BHW_TABLE_BEST, &p, &o, buf, sizeof buf) == BHW_OK, "table describe");
                                                REQUIRE(strstr(buf, "k_ola_table<") != nullptr, "%s", buf);
                                            }
                                        }
                    }
    REQUIRE(replays > 500, "replays %ld", replays);
    // the grid-stride rows: hop 1 over a 2^34 extent needs more row blocks than a grid's y
    {
        bhw_params p;
        bhw_params_init(&p, BHW_WIN_HANN, 4, 16);
        const bhw_ola o = ola_of((1ull << 30) - 1, 16, 1, 0, 0, (1ull << 34) - 16, 0);
        REQUIRE(bhwp_ola_checks(&p, &o, nullptr, nullptr, false) == BHW_OK, "%s", bhw_last_error());
        const BhwOlaPlan pl = bhwp_ola_plan(&p, &o, false, 1, 1);
        REQUIRE(pl.row_blocks > kOlaMaxGridY && pl.grid_y == kOlaMaxGridY, "grid stride");
    }
    // bad descriptors
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH7, 12, 32);
    bhw_ola o = ola_of(4, 0, 1, 0, 0, 10, 0);
    REQUIRE(bhwp_ola_checks(&p, &o, nullptr, nullptr) == BHW_ERR_BADARG, "hop 0");
    o = ola_of(3, UINT64_MAX, 1, 0, 0, 1, 0);
    REQUIRE(bhwp_ola_checks(&p, &o, (const void *)0x1000, (const void *)0x100000000ull) == BHW_ERR_BADARG, "hop overflow");
    o = ola_of(1, UINT64_MAX, 1, 0, 0, 4096, 0);                                     // one frame: any hop
    REQUIRE(bhwp_ola_checks(&p, &o, (const void *)0x1000, (const void *)0x100000000ull) == BHW_OK, "one frame, any hop");
    REQUIRE(bhwp_ola_plan(&p, &o, false).jmax == 1 && bhwp_ola_plan(&p, &o, false).lanes == 4096, "one frame plan");
    o = ola_of(3, 1, 1, UINT64_MAX, 0, 1, 0);
    REQUIRE(bhwp_ola_checks(&p, &o, (const void *)0x1000, (const void *)0x100000000ull) == BHW_ERR_BADARG, "stride overflow");
    o = ola_of(3, 1, 1, 0, 0, 1, 0);
    REQUIRE(bhwp_ola_checks(&p, &o, (const void *)(UINT64_MAX - 64), (const void *)0x1000) == BHW_ERR_BADARG, "y wraps");
    REQUIRE(bhwp_ola_checks(&p, nullptr, nullptr, nullptr) == BHW_ERR_BADARG, "NULL");
    REQUIRE(bhwp_ola_checks(nullptr, &o, nullptr, nullptr) == BHW_ERR_BADARG, "NULL");
    printf("ok %ld\n", g_checks);
    return 0;
}
