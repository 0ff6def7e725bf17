// san_len.cpp -- windows of any length on the host side, under AddressSanitizer + UBSan: the phase map of bhw_len.h against exact
// 128-bit integer arithmetic (every L <= 2^12 at several phi_width, with the no-tie property asserted), the argument checks of the
// *_len calls, the frames and overlap-add plans for any L (grids that cover [0, L) in whole workgroups, power-of-two L giving the
// plans of today), and a host replay of the overlap-add lane arithmetic at non-power-of-two L that sums every product exactly once.
// With a file argument it reads lines "L P m" and prints theta_1(m) for each: the Python side compares them with Python integers.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "bhw_plan.h"

extern "C" int bhw_dbg_describe_frames_from_table(const bhw_params *p_table, uint32_t table_format, const bhw_params *p_call,
                                                  const bhw_frames *f, char *buf, uint64_t len);

static long g_checks = 0;
#define REQUIRE(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// round(mk * 2^P / L) mod 2^P in exact arithmetic, and whether the fraction is exactly one half
static uint32_t exact_theta(uint64_t mk, uint64_t L, uint32_t P, bool *tie)
{
    const unsigned __int128 num = (unsigned __int128)mk << P;     // mk * 2^P
    const unsigned __int128 q = num / L, r = num % L;
    *tie = 2 * r == L;
    return (uint32_t)((q + (2 * r >= L ? 1 : 0)) & ((1u << P) - 1u));
}

// theta of one m_k against the exact value, with no tie and the odd symmetry
static void check_theta(uint64_t L, uint32_t P, uint64_t mk, const BhwLenPhase &lp)
{
    bool tie;
    const uint32_t want = exact_theta(mk, L, P, &tie);
    REQUIRE(!tie, "tie L %" PRIu64 " P %u mk %" PRIu64, L, P, mk);
    REQUIRE(bhw_len_theta(mk, lp) == want, "theta L %" PRIu64 " P %u mk %" PRIu64 ": %u != %u", L, P, mk, bhw_len_theta(mk, lp), want);
    if (mk) REQUIRE(((bhw_len_theta(L - mk, lp) + want) & ((1u << P) - 1u)) == 0, "symmetry L %" PRIu64 " mk %" PRIu64, L, mk);
}

// m_k = (k * m) mod L for the harmonics k = 1..6 by bhw_len_step, and theta of each
static void check_phase(uint64_t L, uint32_t P, uint64_t m)
{
    const BhwLenPhase lp = bhw_len_phase(P, L);
    uint64_t mk = 0;
    for (uint64_t k = 1; k <= 6; ++k) {
        mk = bhw_len_step(mk, m, lp);
        REQUIRE(mk == (k * m) % L, "m_k L %" PRIu64 " m %" PRIu64, L, m);
        check_theta(L, P, mk, lp);
    }
    if (L == (1ull << P)) REQUIRE(bhw_len_theta(m, lp) == (uint32_t)m, "identity at L = 2^P");
}

static bhw_frames frames_of(uint64_t frames, uint64_t hop, uint32_t C, uint64_t ys)
{
    bhw_frames f;
    memset(&f, 0, sizeof f);
    f.struct_size = sizeof f;
    f.channels = C;
    f.frames = frames;
    f.hop = hop;
    f.y_stride = ys;
    return f;
}

static bhw_ola ola_of(uint64_t frames, uint64_t hop, uint32_t C, uint64_t ys, uint64_t t0, uint64_t count)
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
    return o;
}

// The lane arithmetic of ola_loop (bhw_ola.hip) for a window of length L = pl.len: visits[u * L + k] counts the products of output u
// at window index k, each of which must be visited once when frame (t0 + u - k) / hop exists, never otherwise.
static void replay(const BhwOlaPlan &pl, const bhw_ola &o)
{
    const uint64_t L = pl.len;
    std::vector<int> visits(o.count * L, 0);
    const uint64_t rlim = L - (pl.jmax - 1) * o.hop;
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
                const int64_t jr = (!lane_ok || r >= L) ? 0 : (r < rlim ? (int64_t)pl.jmax : (int64_t)pl.jmax - 1);
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
                        REQUIRE(k < L, "k %" PRIu64 " L %" PRIu64, k, L);
                        for (uint32_t i = 0; i < nrow; ++i) {
                            const int64_t f = qa - j + (int64_t)i;
                            if (f < 0 || f >= frames) continue;
                            const uint64_t u = u0 + (uint64_t)i * o.hop;
                            REQUIRE(u < o.count && o.t0 + u == (uint64_t)f * o.hop + k, "u %" PRIu64, u);
                            ++visits[u * L + k];
                        }
                    }
                }
            }
    for (uint64_t u = 0; u < o.count; ++u)
        for (uint64_t k = 0; k < L; ++k) {
            const uint64_t t = o.t0 + u;
            const bool reached = t >= k && (t - k) % o.hop == 0 && (t - k) / o.hop < o.frames;
            REQUIRE(visits[u * L + k] == (reached ? 1 : 0), "L %" PRIu64 " u %" PRIu64 " k %" PRIu64 " visits %d", L, u, k, visits[u * L + k]);
        }
}

static int print_thetas(const char *path)
{
    FILE *fp = fopen(path, "r");
    if (!fp) return 2;
    unsigned long long L, m;
    unsigned P;
    while (fscanf(fp, "%llu %u %llu", &L, &P, &m) == 3) {
        const BhwLenPhase lp = bhw_len_phase(P, L);
        printf("%u\n", bhw_len_theta(bhw_len_mod(m, lp), lp));
    }
    fclose(fp);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1) return print_thetas(argv[1]);

    // ---- the phase map: every L <= 2^12 and every m < L at several P (P >= log2 L), then large L and 64-bit indices
    for (uint32_t P : {12u, 16u, 23u, 30u})
        for (uint64_t L = 1; L <= 4096; ++L) {
            const BhwLenPhase lp = bhw_len_phase(P, L);
            for (uint64_t m = 0; m < L; ++m) check_theta(L, P, m, lp);
            check_phase(L, P, L / 3);
            check_phase(L, P, L - 1);
        }
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&s]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int i = 0; i < 200000; ++i) {
        const uint32_t P = 4 + (uint32_t)(rnd() % 27);
        const uint64_t L = 1 + rnd() % (1ull << P);
        const BhwLenPhase lp = bhw_len_phase(P, L);
        const uint64_t n = rnd();
        REQUIRE(bhw_len_mod(n, lp) == n % L, "mod n %" PRIu64 " L %" PRIu64, n, L);
        check_phase(L, P, n % L);
        uint64_t r;
        REQUIRE(bhw_len_div2l(n, lp, r) == n / (2 * L) && r == n % (2 * L), "div2l");
    }
    for (uint64_t n : {(uint64_t)0, (uint64_t)1, ~(uint64_t)0, ~(uint64_t)0 - 1, (uint64_t)1 << 63, ((uint64_t)1 << 40) + 5})
        for (uint32_t P : {4u, 17u, 30u})
            for (uint64_t L : {(uint64_t)1, (uint64_t)3, ((uint64_t)1 << P) - 1, (uint64_t)1 << P}) {
                const BhwLenPhase lp = bhw_len_phase(P, L);
                REQUIRE(bhw_len_mod(n, lp) == n % L, "mod edge");
            }

    // ---- argument checks and plans
    char buf[512];
    long replays = 0;
    for (uint32_t model = 0; model <= BHW_MODEL_SCALED; ++model)
        for (uint32_t pw : {4u, 5u, 9u, 10u, 12u, 16u, 20u, 24u, 30u})
            for (uint32_t W : {8u, 16u, 24u, 32u}) {
                bhw_params p;
                memset(&p, 0, sizeof p);
                bhw_params_init(&p, BHW_WIN_BH7, pw, W);
                p.model = model;
                const uint64_t N = 1ull << pw;
                if (model <= BHW_MODEL_VHDL && bhwp_validate(&p)) continue;
                if (model > BHW_MODEL_VHDL) {
                    REQUIRE(bhwp_len_checks(&p, N - 1) == BHW_ERR_UNSUPPORTED, "model %u", model);
                    continue;
                }
                REQUIRE(bhwp_len_checks(&p, 0) == BHW_ERR_BADARG, "length 0");
                REQUIRE(bhwp_len_checks(&p, N + 1) == BHW_ERR_BADARG, "length above 2^P");
                p.sin_type = BHW_SIN_TAYLOR_ALL;
                REQUIRE(bhwp_len_checks(&p, N - 1) == BHW_ERR_UNSUPPORTED, "taylor");
                p.sin_type = BHW_SIN_CORDIC;
                const uint64_t lens[] = {1, 2, 3, 5, 7, N / 2 + 1, N - 1, N, 400, 1000, 3 * (N >> 2)};
                for (uint64_t L : lens) {
                    if (L == 0 || L > N) continue;
                    REQUIRE(bhwp_len_checks(&p, L) == BHW_OK, "L %" PRIu64 " pw %u", L, pw);
                    REQUIRE(bhwp_len_kernels(&p, L, false) == (L != N) && bhwp_len_kernels(&p, L, true), "route rule");
                    for (uint64_t frames : {(uint64_t)1, (uint64_t)3, (uint64_t)17, (uint64_t)1000, (uint64_t)1 << 16})
                        for (uint64_t hop : {(uint64_t)1, (uint64_t)3, L / 2 + 1, L, L + 5})
                            for (uint32_t C = 1; C <= 2; ++C)
                                for (int sv = 0; sv < 2; ++sv) {
                                    const uint64_t ys = sv ? (L * C + 17) : 0;
                                    const bhw_frames f = frames_of(frames, hop, C, ys);
                                    const int rc = bhwp_frames_checks(&p, &f, nullptr, nullptr, false, L);
                                    if (frames * L > (1ull << 34)) { REQUIRE(rc == BHW_ERR_BADARG, "frames * L"); continue; }
                                    REQUIRE(rc == BHW_OK, "frames checks rc %d L %" PRIu64, rc, L);
                                    const bhw_frames bad = frames_of(frames, hop, C, L * C - 1);
                                    REQUIRE(L * C == 1 || bhwp_frames_checks(&p, &bad, nullptr, nullptr, false, L) == BHW_ERR_BADARG, "stride below L * C");
                                    for (int from_table = 0; from_table <= 1; ++from_table) {
                                        const BhwFramesPlan pl = bhwp_frames_plan(&p, &f, from_table != 0, -1, L);
                                        REQUIRE(pl.len == L && pl.route == (from_table ? BHWP_FRAMES_TABLE : BHWP_FRAMES_DIRECT), "route");
                                        REQUIRE((pl.kx & (pl.kx - 1)) == 0 && pl.kx * pl.fy == kFramesBlock, "block shape");
                                        REQUIRE(pl.grid_x * pl.kx >= L && (pl.grid_x - 1) * pl.kx < L && pl.grid_x < (1ull << 31), "grid x covers [0, L)");
                                        REQUIRE(pl.group >= 1 && pl.grid_y >= 1 && pl.grid_y <= kFramesMaxGridY, "grid y");
                                        REQUIRE(pl.grid_y * pl.group * pl.fy >= frames && (pl.grid_y - 1) * pl.group * pl.fy < frames, "frames covered");
                                        REQUIRE(pl.y_stride == (ys ? ys : L * C), "stride");
                                        // the highest element a lane touches stays inside d_x / d_y
                                        const uint64_t kmax = L - 1, fmax = frames - 1;
                                        REQUIRE((fmax * hop + kmax) * C + (C - 1) < ((frames - 1) * hop + L) * C, "x bound");
                                        REQUIRE(fmax * pl.y_stride + kmax * C + (C - 1) < (frames - 1) * pl.y_stride + L * C, "y bound");
                                        if (L == N) {                                           // power of two: today's plan
                                            const BhwFramesPlan p0 = bhwp_frames_plan(&p, &f, from_table != 0, from_table ? -1 : BHWP_FRAMES_DIRECT);
                                            REQUIRE(p0.kx == pl.kx && p0.fy == pl.fy && p0.group == pl.group && p0.grid_x == pl.grid_x &&
                                                    p0.grid_y == pl.grid_y && p0.y_stride == pl.y_stride && p0.len == N, "pow2 frames plan");
                                        }
                                    }
                                    // overlap-add over the whole extent and a middle block
                                    const unsigned __int128 ext128 = (unsigned __int128)(frames - 1) * hop + L;
                                    if (ext128 > (1ull << 34)) continue;
                                    const uint64_t ext = (uint64_t)ext128;
                                    for (int rv = 0; rv < 2; ++rv) {
                                        const uint64_t t0 = rv ? ext / 3 : 0, count = rv ? ext / 3 + 1 : ext;
                                        const bhw_ola o = ola_of(frames, hop, C, ys, t0, count);
                                        REQUIRE(bhwp_ola_checks(&p, &o, nullptr, nullptr, false, L) == BHW_OK, "ola checks %s", bhw_last_error());
                                        const bhw_ola past = ola_of(frames, hop, C, ys, t0, ext - t0 + 1);
                                        REQUIRE(bhwp_ola_checks(&p, &past, nullptr, nullptr, false, L) == BHW_ERR_BADARG, "past the extent");
                                        const BhwOlaPlan pl = bhwp_ola_plan(&p, &o, false, 0, 0, L);
                                        REQUIRE(pl.len == L && pl.jmax >= 1 && pl.jmax * hop >= L && (pl.jmax - 1) * hop < L, "jmax");
                                        REQUIRE(pl.grid_x * pl.rx >= pl.lanes && pl.grid_y <= kOlaMaxGridY && pl.q >= 1 && pl.q <= kOlaQMax, "ola grid");
                                        if (L == N) {
                                            const BhwOlaPlan p0 = bhwp_ola_plan(&p, &o, false);
                                            REQUIRE(memcmp(&p0, &pl, sizeof pl) == 0, "pow2 ola plan");
                                        }
                                        if (L <= 1000 && L != N && o.count <= 4096 && W == 32 && model == 0 && (pw == 10 || pw == 12)) {
                                            replay(pl, o);
                                            for (uint32_t fq : {1u, 7u})
                                                replay(bhwp_ola_plan(&p, &o, false, fq, 32, L), o);
                                            replays += 3;
                                        }
                                    }
                                }
                    // describe: the route is named, at L = 2^P the existing text follows
                    const bhw_frames f = frames_of(8, L > 2 ? L / 2 : 1, 1, 0);
                    REQUIRE(bhwp_describe_len(&p, nullptr, false, L, false, 5, 3 * L, nullptr, nullptr, buf, sizeof buf) == BHW_OK, "describe");
                    REQUIRE(strstr(buf, L == N ? "power-of-two route" : "any-length route (L = ") == buf, "%s", buf);
                    REQUIRE(L == N || strstr(buf, "k_direct_len<"), "%s", buf);
                    REQUIRE(bhwp_describe_len(&p, nullptr, false, L, true, 5, 3 * L, &f, nullptr, buf, sizeof buf) == BHW_OK &&
                            strstr(buf, "k_frames_direct_len<"), "%s", buf);
                    char tiny[1];
                    REQUIRE(bhwp_describe_len(&p, nullptr, false, L, true, 0, L, &f, nullptr, tiny, sizeof tiny) == BHW_OK && tiny[0] == 0, "tiny");
                }
            }
    REQUIRE(replays > 100, "replays %ld", replays);
    printf("ok %ld\n", g_checks);
    return 0;
}
