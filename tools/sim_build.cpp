// sim_build.cpp -- CPU model of the table-build kernel's arithmetic (k_table_build_mirror), used to establish on the host
// that its short cuts are exact before (and after) they are written for the GPU:
//   (1) octant mirror: chain(E - u) == swap(chain(u)) unless some z_k == 0 before the hand-over rotation KS;
//   (2) narrow state: inside a "safe" 64-leaf group every x_k, y_k lies in [0, 2^NITER) from the group's split rotation on, so
//       the rotations run on 32-bit unsigned words with logical shifts;
//   (3) table tail: for the last TAIL rotations  (y_k >> k) == (y_KS >> KS) >> (k - KS)  as long as the low KS bits of x_KS, y_KS
//       keep a margin of 128 to both ends, so  x_end = x_KS - D[p][y_KS >> KS],  y_end = y_KS + D[p][x_KS >> KS]  with
//       D[p][v] = sum_j sigma_j(p) (v >> j)  and p the decision pattern looked up from z_KS;
//   (4) biased narrow state (round 4): a group whose x runs up to 2^NITER (1 + eps) -- the first third of a degree of the octant,
//       where x alone does not fit the 32-bit word -- keeps x - 2^(NITER-1) in the word instead:  (x >> k) = ((x - B) >> k) + (B >> k)
//       exactly, B = 2^(NITER-1) being a multiple of 2^k for every k < NITER, and the tail table gets a 65th row (x >> KS = 64).
//   (5) rank entry: from its split rotation k0 the angle of a group's leaves is affine in the lane, z_k0(lane) = zf + (lane << z_shl),
//       so the first J = 4 decisions of a leaf are its rank among the 2^J - 1 sign-change thresholds of the decision tree (partial
//       sums +- lut[k0] +- lut[k0+1] +- lut[k0+2], in order).  The 2^J states a group can reach are computed once per group, the
//       rank is a population count over a 64-bit mask of the lanes at which a threshold is crossed, and a zero event z_(k0+i) == 0
//       is z_k0 == the threshold just below the rank.  Each leaf is also walked through the J rotations one by one and compared.
// Every entry of the first-quadrant table is compared with the plain chain (the rotation loop of
// hls/windows/win_function.cpp:110-125 | cpp/cordic_sincos.cpp:49-63 | src/cordic_dds.vhd:197-213).
// Test infrastructure / design evidence only: nothing here is linked into the product.
// Besides the comparison it prints what the rare paths of the kernel see in this configuration: the deferred images of the fullest
// workgroup (the kernel's worklist bound) and the entries that leave the four-bit fields of the nibble formats (the format the
// device settles on).
//   usage: sim_build [--escapes] <model 0 hls | 1 cpp | 2 vhdl> <PW> <W> [precision [tail rotations 6 | 7]]     (exit code 0 = every entry identical)
// --escapes adds a last line "listed entries:" with the index u of every entry the nibble + escapes format lists, in ascending order
// (tools/escape_lengths.py chooses from it the window lengths whose gathers reach such entries).
#include <quadmath.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int64_t T2[48], T4[48], G46, G47;

static void tables()
{
    const __float128 pi = M_PIq;
    __float128 k = 1.0Q;
    for (int i = 0; i < 48; ++i) {
        const __float128 a = atanq(ldexpq(1.0Q, -i)) / pi;
        T2[i] = (int64_t)floorq(ldexpq(a, 47) + 0.5Q);
        T4[i] = (int64_t)floorq(ldexpq(a, 48) + 0.5Q);
    }
    T4[47] = 0;
    for (int i = 0; i < 120; ++i) k *= sqrtq(1.0Q + ldexpq(1.0Q, -2 * i));
    G46 = (int64_t)floorq(ldexpq(1.0Q, 46) / k + 0.5Q);
    G47 = (int64_t)floorq(ldexpq(1.0Q, 47) / k + 0.5Q);
}

struct Cfg {
    int64_t lut[32];
    int64_t x0;
    int n_iter, z_shl, out_shr;
    uint32_t E;   // first-quadrant entries (z_shr == 0)
};

static void step(int64_t &x, int64_t &y, int64_t &z, int k, int64_t l)
{
    const int64_t xs = x >> k, ys = y >> k;
    if (z < 0) { x += ys; y -= xs; z += l; }
    else       { x -= ys; y += xs; z -= l; }
}

int main(int argc, char **argv)
{
    bool list_escapes = false;
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--escapes")) {
            list_escapes = true;
            for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
            --argc; --i;
        }
    if (argc < 4) { fprintf(stderr, "usage: sim_build [--escapes] model PW W [precision]\n"); return 2; }
    tables();
    const int model = atoi(argv[1]), PW = atoi(argv[2]), W = atoi(argv[3]), P = argc > 4 ? atoi(argv[4]) : 1;
    Cfg c{};
    if (model == 0)      { for (int i = 0; i + 1 < W; ++i) c.lut[i] = T4[i] >> (47 - W); c.x0 = G46 >> (46 - W); c.n_iter = W; c.z_shl = W - PW + 2; c.out_shr = 2; }
    else if (model == 1) { for (int i = 0; i + 1 < W; ++i) c.lut[i] = T2[i] >> (47 - W); c.x0 = G46 >> (46 - W); c.n_iter = W; c.z_shl = W - PW + 1; c.out_shr = 2; }
    else { const int Wi = W + P; for (int i = 0; i + 1 < W; ++i) c.lut[i] = T4[i] >> (49 - Wi); c.x0 = G47 >> (49 - Wi); c.n_iter = W - 1; c.z_shl = W - PW + P; c.out_shr = P; }
    // z_shr == 0 as bhwp_resolve_cordic has it: hls / cpp at PW - 1 < W; vhdl up to PW == W (z_shl = P there: the 21-rotation tables at 22 / 22)
    if (c.z_shl < 0 || (model == 0 ? PW - 1 >= W : model == 1 ? PW - 1 >= W : PW > W)) { fprintf(stderr, "z_shr != 0: not a mirror-kernel configuration\n"); return 2; }
    c.E = 1u << (PW - 2);
    const int N = c.n_iter, TAIL = argc > 5 ? atoi(argv[5]) : 6, KS = N - TAIL, PREFIX_MAX = 20;
    if (TAIL != 6 && TAIL != 7) { fprintf(stderr, "tail of 6 or 7 rotations\n"); return 2; }
    const int NV = 1 << TAIL, NP = 1 << TAIL, MARGIN = 2 << TAIL;     // rows / patterns of D; the tail moves x by less than MARGIN
    const int kcap = KS < PREFIX_MAX ? KS : PREFIX_MAX;
    const uint32_t E = c.E;
    const int s = c.z_shl;
    if (2 * c.lut[0] != ((int64_t)E << s)) { fprintf(stderr, "2 lut[0] is not a quarter turn\n"); return 2; }

    // reference: plain chain for every entry
    std::vector<int32_t> rc(E), rs(E);
    for (uint32_t u = 0; u < E; ++u) {
        int64_t x = c.x0, y = 0, z = (int64_t)u << s;
        for (int k = 0; k < N; ++k) step(x, y, z, k, c.lut[k]);
        rc[u] = (int32_t)(x >> c.out_shr);
        rs[u] = (int32_t)(y >> c.out_shr);
    }

    // tail tables: pattern of z_KS (range [-ZB, ZB)), D[p][v]
    const int ZB = 4 << TAIL;                                                // |z_KS| < ZB (checked per lane below)
    std::vector<uint16_t> Pz(2 * ZB);
    for (int zi = 0; zi < 2 * ZB; ++zi) {
        int64_t z = zi - ZB;
        unsigned p = 0;
        for (int j = 0; j < TAIL; ++j) {
            const int k = KS + j;
            if (z < 0) { p |= 1u << j; z += c.lut[k]; } else z -= c.lut[k];
        }
        Pz[zi] = (uint16_t)p;
    }
    std::vector<std::vector<int16_t>> D(NP, std::vector<int16_t>(NV + 1));
    for (unsigned p = 0; p < (unsigned)NP; ++p)
        for (int v = 0; v <= NV; ++v) {
            int d = 0;
            for (int j = 0; j < TAIL; ++j) d += ((p >> j) & 1u) ? -(v >> j) : (v >> j);    // sigma = +1 when z >= 0
            D[p][v] = (int16_t)d;
        }

    std::vector<int32_t> gc(E, INT32_MIN), gs(E, INT32_MIN);
    uint64_t hi_groups = 0;
    const int KA = KS - 10;                                                  // the kernel's ten-rotation block starts here
    const int64_t BX = (int64_t)1 << (N - 1);                                // bias of the biased narrow state
    uint64_t n_groups = E >> 7, wide_groups = 0, unsafe_waves = 0, unsafe_lanes = 0, zero_lanes = 0, zero_prefix = 0;
    const int64_t LIM = (int64_t)1 << N;
    constexpr int J = 4;                                                     // rotations a rank group skips
    uint64_t rank_groups = 0, rank_refused = 0, rank_bad = 0, zero_thr = 0, zero_rot = 0;
    // deferred images per workgroup of the kernel, for both of its shapes (64 and 256 own groups): what its worklist (kWorkMax = 8 x
    // groups per workgroup) has to hold
    std::vector<uint32_t> def64((n_groups + 63) / 64, 0u), def256((n_groups + 255) / 256, 0u);
    auto full_chain = [&](uint32_t u, int32_t &oc, int32_t &os) {           // the kernel's deferred / fallback chain
        int64_t x = c.x0, y = c.x0, z = ((int64_t)u << s) - c.lut[0];
        for (int k = 1; k < N; ++k) step(x, y, z, k, c.lut[k]);
        oc = (int32_t)(x >> c.out_shr); os = (int32_t)(y >> c.out_shr);
    };
    for (uint64_t g = 0; g < n_groups; ++g) {
        // phase 1: shared prefix
        int64_t X = c.x0, Y = c.x0, zf = ((int64_t)(g << 6) << s) - c.lut[0];
        const int64_t span = (int64_t)63 << s;
        int k0 = 1;
        bool zero0 = false;
        for (int kk = 1; kk < kcap; ++kk) {
            const int64_t zl = zf + span;
            if ((zf < 0) != (zl < 0)) break;
            zero0 |= zf == 0;
            step(X, Y, zf, kk, c.lut[kk]);
            k0 = kk + 1;
        }
        zero_prefix += zero0;
        // narrow-state test (scalar, per group)
        const int64_t Dr = ((int64_t)1 << (N - k0 + 1)) + 2;
        bool narrow = X >= Dr && Y >= Dr && X + Dr < LIM && Y + Dr < LIM && N <= 32;
        // biased: x - B in [Dr, 2^32 - Dr), x below 65 * 2^KS (row 64 of the tail table), y as in the plain narrow state; only groups
        // that enter the ten-rotation block (split rotation >= KA)
        const bool hi = !narrow && N <= 32 && k0 >= KA && Y >= Dr && Y + Dr < LIM && X - BX >= Dr && X - BX + Dr < ((int64_t)1 << 32) &&
                        X + Dr < LIM + ((int64_t)1 << KS);
        const int64_t bias = hi ? BX : 0;
        hi_groups += hi;
        narrow = narrow || hi;
        wide_groups += !narrow;
        if (!narrow && getenv("SIM_VERBOSE")) fprintf(stderr, "wide g=%llu k0=%d X=%lld Y=%lld Dr=%lld\n", (unsigned long long)g, k0, (long long)X, (long long)Y, (long long)Dr);
        bool wave_unsafe = false;
        // rank entry (per group, as one lane of the kernel's phase 1 has it): thresholds in order, the lane at which each is crossed,
        // the 2^J candidate states
        bool ranked = narrow && k0 >= KA && k0 + J <= KS;
        int32_t Tb[1 << J], Cr[1 << J];                                      // threshold just below rank r; z offset of rank r
        uint32_t cx[1 << J], cy[1 << J];
        uint64_t M = 0;
        int base = 0;
        if (ranked) {
            int32_t prev = INT32_MIN;
            int n_hi = 0;
            Tb[0] = INT32_MIN;
            for (int p = 1; p < (1 << J); ++p) {                             // in-order position p: depth J - 1 - ctz(p), path p >> (ctz(p) + 1)
                const int tz = __builtin_ctz(p), depth = J - 1 - tz, path = p >> (tz + 1);
                int64_t T = 0;
                for (int m = 0; m < depth; ++m) T += ((path >> (depth - 1 - m)) & 1) ? c.lut[k0 + m] : -c.lut[k0 + m];
                if (T <= prev) ranked = false;                               // not in order: the ROM words do not nest
                prev = (int32_t)T;
                Tb[p] = (int32_t)T;
                const int64_t num = T - zf + (((int64_t)1 << s) - 1);        // l = ceil((T - zf) / 2^s): first lane with z >= T
                if (num != (int32_t)num) { fprintf(stderr, "threshold difference leaves 32 bits\n"); return 1; }
                const int32_t l = (int32_t)num >> s;
                if (l <= 0) ++base;
                else if (l <= 63) M |= 1ull << (l - 1);
                else ++n_hi;
            }
            if (__builtin_popcountll(M) + base + n_hi != (1 << J) - 1) ranked = false;   // two thresholds between the same two lanes
            for (int r = 0; r < (1 << J); ++r) {
                int64_t C = 0;
                for (int m = 0; m < J; ++m) C += ((r >> (J - 1 - m)) & 1) ? c.lut[k0 + m] : -c.lut[k0 + m];
                Cr[r] = (int32_t)C;
            }
            cx[0] = (uint32_t)(X - bias); cy[0] = (uint32_t)Y;
            for (int m = 0; m < J; ++m)                                      // level m: 2^m states -> 2^(m+1), child 2r + 1 = forward (z >= 0)
                for (int r = (1 << m) - 1; r >= 0; --r) {
                    const uint32_t a = cy[r] >> (k0 + m), b = (cx[r] >> (k0 + m)) + (uint32_t)(bias >> (k0 + m));
                    const uint32_t xr = cx[r], yr = cy[r];
                    cx[2 * r] = xr + a; cy[2 * r] = yr - b;
                    cx[2 * r + 1] = xr - a; cy[2 * r + 1] = yr + b;
                }
            rank_refused += !ranked;
            rank_groups += ranked;
        }
        struct Lane { int64_t x, y, z; bool zero; } L[64];
        for (int lane = 0; lane < 64; ++lane) {
            int64_t x = X, y = Y, z = zf + ((int64_t)lane << s);
            bool zero = false;
            int kfrom = k0;
            if (ranked) {
                // the J rotations one by one (what the rank entry replaces) ...
                int64_t xr = X, yr = Y, zr = z;
                bool zrot = false;
                for (int k = k0; k < k0 + J; ++k) { zrot |= zr == 0; step(xr, yr, zr, k, c.lut[k]); }
                // ... and the rank entry
                const int rank = base + __builtin_popcountll(M & ((1ull << lane) - 1ull));
                zero = (int32_t)z == Tb[rank];
                x = (int64_t)cx[rank] + bias; y = cy[rank]; z = z - Cr[rank];
                zero_thr += zero; zero_rot += zrot;
                if (x != xr || y != yr || z != zr || zero != zrot) { if (rank_bad < 5) fprintf(stderr, "rank entry differs g=%llu lane=%d rank=%d\n", (unsigned long long)g, lane, rank); ++rank_bad; }
                kfrom = k0 + J;
            }
            for (int k = kfrom; k < KS; ++k) {
                zero |= z == 0;
                if (narrow) {
                    if (x - bias < 0 || y < 0 || x - bias >= ((int64_t)1 << 32) || y >= LIM) { fprintf(stderr, "narrow range violated g=%llu lane=%d k=%d\n", (unsigned long long)g, lane, k); return 1; }
                    const uint32_t xu = (uint32_t)(x - bias), yu = (uint32_t)y;
                    const uint32_t a = yu >> k, b = (xu >> k) + (uint32_t)(bias >> k);     // logical shifts on 32-bit words
                    uint32_t xn, yn;
                    if (z < 0) { xn = xu + a; yn = yu - b; z += c.lut[k]; } else { xn = xu - a; yn = yu + b; z -= c.lut[k]; }
                    x = (int64_t)xn + bias; y = yn;
                } else step(x, y, z, k, c.lut[k]);
            }
            L[lane] = Lane{x, y, z, zero};
            if (narrow) {
                if (x - bias < 0 || y < 0 || x - bias >= ((int64_t)1 << 32) || y >= LIM) { fprintf(stderr, "narrow range violated at KS\n"); return 1; }
                const uint32_t lowm = (1u << KS) - 1u;
                const bool ok = (((uint32_t)(x - bias) + (uint32_t)MARGIN) & lowm) >= 2u * (uint32_t)MARGIN && (((uint32_t)y + (uint32_t)MARGIN) & lowm) >= 2u * (uint32_t)MARGIN &&
                                (uint64_t)(z + ZB) < (uint64_t)(2 * ZB);
                if (!ok) { wave_unsafe = true; ++unsafe_lanes; }
            }
        }
        unsafe_waves += wave_unsafe;
        for (int lane = 0; lane < 64; ++lane) {
            const uint32_t u = (uint32_t)(g << 6) + lane;
            int64_t x = L[lane].x, y = L[lane].y, z = L[lane].z;
            int64_t x2 = y, y2 = x, z2 = -z;
            int32_t oc, os, oc2, os2;
            if (narrow && !wave_unsafe) {
                const uint32_t xu = (uint32_t)(x - bias);
                const uint32_t xx = (xu >> KS) + (uint32_t)(bias >> KS), yy = (uint32_t)y >> KS;
                if (xx > (uint32_t)NV || yy >= (uint32_t)NV) { fprintf(stderr, "tail operand out of range\n"); return 1; }
                const unsigned p = Pz[z + ZB], p2 = Pz[-z + ZB];
                const uint32_t bo = (uint32_t)(bias >> c.out_shr);
                oc = (int32_t)(((xu - (uint32_t)(int32_t)D[p][yy]) >> c.out_shr) + bo);
                os = (int32_t)(((uint32_t)y + (uint32_t)(int32_t)D[p][xx]) >> c.out_shr);
                oc2 = (int32_t)(((uint32_t)y - (uint32_t)(int32_t)D[p2][xx]) >> c.out_shr);
                os2 = (int32_t)(((xu + (uint32_t)(int32_t)D[p2][yy]) >> c.out_shr) + bo);
            } else {
                for (int k = KS; k < N; ++k) { step(x, y, z, k, c.lut[k]); step(x2, y2, z2, k, c.lut[k]); }
                oc = (int32_t)(x >> c.out_shr); os = (int32_t)(y >> c.out_shr);
                oc2 = (int32_t)(x2 >> c.out_shr); os2 = (int32_t)(y2 >> c.out_shr);
            }
            gc[u] = oc; gs[u] = os;
            if (u >= 1 && u <= (E >> 1) - 1) {
                if (L[lane].zero || (zero0 && lane == 0)) { ++zero_lanes; ++def64[g >> 6]; ++def256[g >> 8]; full_chain(E - u, oc2, os2); }   // worklist / leaf-0 replay
                gc[E - u] = oc2; gs[E - u] = os2;
            }
        }
    }
    full_chain(E >> 1, gc[E >> 1], gs[E >> 1]);                                 // the middle entry: a deferred chain
    ++def64.back(); ++def256.back();                                            // ... of the last workgroup (the kernel's work_n starts at 1 there)
    uint32_t def64_max = 0, def256_max = 0;
    for (uint32_t v : def64) def64_max = v > def64_max ? v : def64_max;
    for (uint32_t v : def256) def256_max = v > def256_max ? v : def256_max;

    // Nibble formats, restated from the kernel's store_entry and its records: cells of 2^d entries (d as bhwk_resid_dlog has it), record
    // = the cell's first entry (c, s) and the step to the next cell's (the table's last cell: the step from the cell before it), line
    // = head + ((step * place) >> d), field = value - line + 8 stored in four bits.  "nibble": no field may leave 0 .. 15.  "nibble +
    // escapes": the line lies one higher (kEscBias), the c field 0 is the marker, and what does not fit goes to the list of the
    // workgroup that stores the entry (an own entry u < E/2, the image E - u of one, the middle entry with the last workgroup): a list
    // beyond kEscFill = 96 entries refuses the format.  The workgroup has 256 own groups from 2^24 entries on, 64 below.
    int dlog = (2 * PW - W - 2) / 2;
    if (dlog > 9) dlog = 9;
    if (dlog < 7 || W + c.out_shr > 34) dlog = 0;                                // no residual cell: not a configuration of the packed formats
    uint64_t nib_out = 0, esc_all = 0;
    uint32_t esc_wg_max = 0;
    std::vector<uint32_t> esc_u;                                                 // the listed entries (--escapes)
    const uint32_t wg_groups = E >= (1u << 24) ? 256u : 64u;
    if (dlog) {
        std::vector<uint32_t> esc_wg((n_groups + wg_groups - 1) / wg_groups, 0u);
        const uint32_t cells = E >> dlog, fm = (1u << dlog) - 1u;
        for (uint32_t u = 0; u < E; ++u) {
            const uint32_t cell = u >> dlog, h = cell << dlog, pos = u & fm;
            const int32_t dc = cell + 1 < cells ? rc[h + fm + 1] - rc[h] : rc[h] - rc[h - fm - 1];
            const int32_t ds = cell + 1 < cells ? rs[h + fm + 1] - rs[h] : rs[h] - rs[h - fm - 1];
            const int32_t pc = rc[h] - 8 + ((dc * (int32_t)pos) >> dlog), ps = rs[h] - 8 + ((ds * (int32_t)pos) >> dlog);
            const uint32_t nc = (uint32_t)(rc[u] - pc), ns = (uint32_t)(rs[u] - ps);
            nib_out += (nc | ns) > 15u;
            const uint32_t ec = nc - 1u, es = ns - 1u;                           // the same fields against the line one higher
            if (ec - 1u > 14u || es > 15u) {
                const uint32_t src = u < (E >> 1) ? u : u == (E >> 1) ? (E >> 1) - 1u : E - u;   // the own entry whose workgroup stores it
                ++esc_all;
                esc_u.push_back(u);
                ++esc_wg[(src >> 6) / wg_groups];
            }
        }
        for (uint32_t v : esc_wg) esc_wg_max = v > esc_wg_max ? v : esc_wg_max;
    }
    uint64_t bad = 0;
    for (uint32_t u = 0; u < E; ++u)
        if (gc[u] != rc[u] || gs[u] != rs[u]) { if (bad < 5) fprintf(stderr, "mismatch u=%u got (%d,%d) want (%d,%d)\n", u, gc[u], gs[u], rc[u], rs[u]); ++bad; }
    printf("model %d PW %d W %d P %d: entries %u, groups %llu, wide-state groups %llu (%.2f %%), waves with an unsafe tail lane %llu (lanes %llu), "
           "deferred images %llu (prefix zeros %llu), biased-narrow groups %llu, mismatches %llu, deferred per workgroup max %u of 64 groups | %u of 256 groups, "
           "cell log %d, outside nibble fields %llu, escape lists %llu (max %u in one workgroup of %u groups)\n", model, PW, W, P, E, (unsigned long long)n_groups,
           (unsigned long long)wide_groups, 100.0 * wide_groups / n_groups, (unsigned long long)unsafe_waves, (unsigned long long)unsafe_lanes,
           (unsigned long long)zero_lanes, (unsigned long long)zero_prefix, (unsigned long long)hi_groups, (unsigned long long)bad, def64_max, def256_max,
           dlog, (unsigned long long)nib_out, (unsigned long long)esc_all, esc_wg_max, wg_groups);
    // (a line of its own: the sweep's parsers read the line above as it always was)
    printf("rank entry J %d: groups %llu of %llu, refused %llu, leaves that differ from the rotations %llu, zero events by threshold %llu | by rotation %llu\n", J,
           (unsigned long long)rank_groups, (unsigned long long)n_groups, (unsigned long long)rank_refused, (unsigned long long)rank_bad,
           (unsigned long long)zero_thr, (unsigned long long)zero_rot);
    if (list_escapes) {
        printf("listed entries:");
        for (uint32_t u : esc_u) printf(" %u", u);
        printf("\n");
    }
    return bad || rank_bad || zero_thr != zero_rot ? 1 : 0;
}
