// san_frames.cpp -- the planner's part of the overlapped-frame apply (bhw_plan.cpp: argument checks, route rule, frame-group size, grid
// shape, extent and overlap checks, the text of bhw_apply_frames_describe) swept under AddressSanitizer + UBSan over phi_width 4..30,
// hops 1..2N, 1..2^20 frames, both channel counts, strides, sources and tables.  Besides "no report", it checks that the grid covers
// every frame exactly once in whole workgroups and stays inside the launch limits.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "bhw_plan.h"

extern "C" int bhw_dbg_describe_frames_from_table(const bhw_params *p_table, uint32_t table_format, const bhw_params *p_call,
                                                  const bhw_frames *f, char *buf, uint64_t len);

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

int main()
{
    char buf[384], tiny[1];
    static const uint64_t kFrames[] = {1, 2, 3, 4, 5, 15, 16, 17, 255, 1000, 4096, 16384, 65535, 65537, 1u << 20};
    for (uint32_t model = 0; model <= BHW_MODEL_VHDL; ++model)
        for (uint32_t pw = 4; pw <= 30; ++pw)
            for (uint32_t W = 8; W <= 32; W += 8)
                for (uint32_t sin_type = 0; sin_type <= 2; ++sin_type)
                    for (uint32_t win : {(uint32_t)BHW_WIN_HANN, (uint32_t)BHW_WIN_BH4, (uint32_t)BHW_WIN_BH7}) {
                        bhw_params p;
                        memset(&p, 0, sizeof p);
                        bhw_params_init(&p, win, pw, W);
                        p.model = model;
                        p.sin_type = sin_type;
                        if (bhwp_validate(&p)) continue;
                        const uint64_t N = 1ull << pw;
                        const uint64_t hops[] = {1, 3, N / 4 ? N / 4 : 1, N / 2, N - 1, N, N + 5, 2 * N};
                        for (uint64_t frames : kFrames)
                            for (uint64_t hop : hops)
                                for (uint32_t C = 1; C <= 2; ++C)
                                    for (int sv = 0; sv < 3; ++sv) {
                                        const uint64_t ys = sv == 0 ? 0 : sv == 1 ? N * C : N * C + 17;
                                        const bhw_frames f = frames_of(frames, hop, C, ys, (uint32_t)(frames % 63));
                                        const int rc = bhwp_frames_checks(&p, &f, (const void *)0x1000, (const void *)0x1000, false);
                                        const bool too_many = frames * N > (1ull << 34);
                                        if (sin_type != BHW_SIN_CORDIC && C == 2) { REQUIRE(rc == BHW_ERR_UNSUPPORTED, "rc %d", rc); continue; }
                                        if (too_many) { REQUIRE(rc == BHW_ERR_BADARG, "frames * N > 2^34 pw %u frames %" PRIu64, pw, frames); continue; }
                                        REQUIRE(rc == BHW_OK, "rc %d pw %u frames %" PRIu64 " hop %" PRIu64, rc, pw, frames, hop);
                                        // the same pointers for x and y overlap whenever there is something to do
                                        REQUIRE(bhwp_frames_checks(&p, &f, (const void *)0x1000, (const void *)0x1000) == BHW_ERR_BADARG, "overlap");
                                        for (int from_table = 0; from_table <= (sin_type == BHW_SIN_CORDIC ? 1 : 0); ++from_table) {
                                            const BhwFramesPlan pl = bhwp_frames_plan(&p, &f, from_table != 0);
                                            REQUIRE(pl.y_stride == (ys ? ys : N * C), "stride");
                                            if (from_table) REQUIRE(pl.route == BHWP_FRAMES_TABLE, "table route");
                                            else if (C == 2) REQUIRE(pl.route == BHWP_FRAMES_DIRECT, "I/Q: frames kernel");
                                            else if (sin_type != BHW_SIN_CORDIC) REQUIRE(pl.route == BHWP_FRAMES_PER_FRAME, "Taylor: per frame");
                                            if (pl.route == BHWP_FRAMES_PER_FRAME) continue;
                                            REQUIRE(pl.kx * pl.fy == kFramesBlock && pl.grid_x * pl.kx == N && (pl.kx & (pl.kx - 1)) == 0, "block shape");
                                            REQUIRE(pl.grid_y >= 1 && pl.grid_y <= kFramesMaxGridY && pl.grid_x < (1ull << 31), "grid limits");
                                            const uint64_t per_wg = pl.group * pl.fy;
                                            REQUIRE(pl.group >= 1 && pl.grid_y * per_wg >= frames && (pl.grid_y - 1) * per_wg < frames,
                                                    "cover: frames %" PRIu64 " G %" PRIu64 " gy %" PRIu64, frames, pl.group, pl.grid_y);
                                            // the last frame's extents stay inside what the checks accepted
                                            const unsigned __int128 xe = ((unsigned __int128)(frames - 1) * hop + N) * C;
                                            REQUIRE(xe <= (1ull << 60), "x extent");
                                        }
                                        // describe: the same text through the library call and the table call, truncation safe
                                        REQUIRE(bhwp_describe_frames(&p, nullptr, &f, buf, sizeof buf) == BHW_OK, "describe");
                                        REQUIRE(strlen(buf) > 10 && strlen(buf) < sizeof buf, "text");
                                        REQUIRE(bhwp_describe_frames(&p, nullptr, &f, tiny, sizeof tiny) == BHW_OK && tiny[0] == 0, "tiny");
                                        if (sin_type == BHW_SIN_CORDIC && frames == 4 && hop == N / 2 && W == 32) {
                                            REQUIRE(bhw_dbg_describe_frames_from_table(&p, BHW_TABLE_BEST, &p, &f, buf, sizeof buf) == BHW_OK, "table describe");
                                            REQUIRE(strstr(buf, "k_frames_table<") != nullptr, "%s", buf);
                                        }
                                    }
                    }
    // bad descriptors
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH7, 12, 32);
    bhw_frames f = frames_of(4, 0, 1, 0, 0);
    REQUIRE(bhwp_frames_checks(&p, &f, nullptr, nullptr) == BHW_ERR_BADARG, "hop 0");
    f = frames_of(3, UINT64_MAX, 1, 0, 0);
    REQUIRE(bhwp_frames_checks(&p, &f, (const void *)0x1000, (const void *)0x100000000ull) == BHW_ERR_BADARG, "hop overflow");
    f = frames_of(3, 1, 1, UINT64_MAX, 0);
    REQUIRE(bhwp_frames_checks(&p, &f, (const void *)0x1000, (const void *)0x100000000ull) == BHW_ERR_BADARG, "stride overflow");
    f = frames_of(3, 1, 1, 0, 0);
    REQUIRE(bhwp_frames_checks(&p, &f, (const void *)0x1000, (const void *)(UINT64_MAX - 64)) == BHW_ERR_BADARG, "y wraps");
    REQUIRE(bhwp_frames_checks(&p, nullptr, nullptr, nullptr) == BHW_ERR_BADARG, "NULL");
    REQUIRE(bhwp_frames_checks(nullptr, &f, nullptr, nullptr) == BHW_ERR_BADARG, "NULL");
    printf("ok %ld\n", g_checks);
    return 0;
}
