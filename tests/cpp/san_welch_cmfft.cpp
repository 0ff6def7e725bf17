// san_welch_cmfft.cpp -- the planner's part of the fused Welch PSD calls for I/Q input at a mixed-radix n_fft (bhw_plan.cpp:
// bhwp_welch_cmfft_checks / bhwp_welch_cmfft_plan / bhwp_welch_cmfft_workspace_bytes / bhwp_describe_welch_cmfft) swept under
// AddressSanitizer + UBSan over every supported n_fft, and a host replay, lane by lane, of what bhw_welch_cmfft.hip does with the plan:
//   - run ownership and the padded frame map: workgroup w walks the groups first(w), next(...) of stft_cmfft_rows under an epilogue
//     that owns runs; every group of the padded pool is visited exactly once, by the workgroup that owns its run, a run's groups in
//     ascending order and never across a signal; a slot is live exactly when its frame is below F;
//   - the accumulate step, both regimes, with the compare-and-subtract column turn of BHW_CFFT_SHIFT (n is no power of two, and may
//     be odd), on a q array of exactly B * F * n doubles and a workspace of exactly the plan's bytes: every chunk sum is written
//     exactly once, every read and write stays inside, and every (b, f < F, k) is added exactly once, in ascending f inside its chunk;
//   - the join: both launches lane by lane over the same workspace (bins = n_fft, flags 0), every block sum and every P written
//     once, P's row inside p_stride, and P equal bit for bit to the contract restated as three plain loops, column j holding bin j
//     or (j + n - n / 2) mod n.
// Then the three-level sum against the contract on random positive doubles, bit for bit.
// The arrays the replay indexes are std::vectors of exactly the sizes the contract states, so an index the asserts missed is ASan's.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
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

static bhw_stft desc_of(uint64_t B, uint64_t T, uint64_t frames, uint64_t hop, uint64_t n_fft, uint64_t col0, uint64_t pad, uint32_t mode)
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
    s.pad_mode = mode;
    s.shift = 15;
    return s;
}

constexpr uint32_t CH = BHW_WELCH_FFT_CHUNK, BLK = BHW_WELCH_BLOCK;

// bin k's column under the turn (0 or n / 2, integer division): a compare and a subtract, as the kernel; and its inverse
static uint32_t col_of(uint32_t k, uint32_t turn, uint32_t n)
{
    const uint32_t j = k + turn;
    return j >= n ? j - n : j;
}
static uint32_t bin_of(uint32_t j, uint32_t turn, uint32_t n)
{
    return turn ? (j + n - turn) % n : j;
}

// the contract of include/bhw.h as three plain loops over q[(b * F + f) * K + k]
static double contract_sum(const std::vector<double> &q, uint64_t b, uint64_t F, uint64_t K, uint64_t k)
{
    double A = 0.0;
    for (uint64_t f0 = 0; f0 < F; f0 += BLK) {
        double Ab = 0.0;
        for (uint64_t c0 = f0; c0 < F && c0 < f0 + BLK; c0 += CH) {
            double Ac = 0.0;
            for (uint64_t f = c0; f < F && f < c0 + CH; ++f) Ac += q.at((b * F + f) * K + k);
            Ab += Ac;
        }
        A += Ab;
    }
    return A;
}

// k_welch_fft_join<GROUPED, FINAL> as bhwk_welch_join launches it, every lane of every workgroup
static void replay_join(bool grouped, bool final, const std::vector<double> &in, std::vector<double> *out, std::vector<int> *out_hit,
                        std::vector<float> &P, std::vector<int> &P_hit, uint64_t batch, uint64_t bins, uint64_t n_fft, uint64_t n_in,
                        uint64_t n_out, uint64_t p_stride, double scale, uint32_t flags, uint64_t grid)
{
    constexpr uint32_t U = BLK / CH;
    REQUIRE(grid * 256u >= batch * n_out * bins && (grid - 1) * 256u < batch * n_out * bins, "join grid %" PRIu64, grid);
    for (uint64_t wg = 0; wg < grid; ++wg)
        for (uint32_t t = 0; t < 256; ++t) {
            const uint64_t i = wg * 256u + t;
            if (i >= batch * n_out * bins) continue;
            const uint64_t k = i % bins, rest = i / bins;
            const uint64_t o = rest % n_out, b = rest / n_out;
            const uint64_t base = b * n_in * bins + k;
            const uint64_t i0 = grouped ? o * U : 0, i1 = grouped ? (i0 + U < n_in ? i0 + U : n_in) : n_in;
            REQUIRE(i0 < i1, "an output with no input");
            double A = 0.0;
            for (uint64_t j = i0; j < i1; j += U) {
                double v[U];
                for (uint32_t u = 0; u < U; ++u) v[u] = in.at(base + (j + u < i1 ? j + u : i1 - 1u) * bins);
                for (uint32_t u = 0; u < U; ++u)
                    if (j + u < i1) A += v[u];
            }
            if (final) {
                REQUIRE(!bhw_psd_doubled(flags, k, bins, n_fft), "nothing is doubled");
                REQUIRE(k < p_stride, "P's row inside p_stride");
                P.at(b * p_stride + k) = (float)(A * scale);
                ++P_hit.at(b * p_stride + k);
            } else {
                out->at((b * n_out + o) * bins + k) = A;
                ++out_hit->at((b * n_out + o) * bins + k);
            }
        }
}

// One call, lane by lane.  q: B * F * n distinct non-negative doubles standing for the powers of the transformed rows, by BIN.
static void replay_call(const BhwWelchCmfftPlan &wp, const bhw_stft &s, double scale)
{
    const BhwStftCmfftPlan &pl = wp.fft;
    const uint64_t B = s.batch, F = s.frames, K = wp.bins;
    const uint32_t fy = pl.fy, n = pl.n;
    const uint32_t turn = pl.shifted ? n >> 1 : 0u;
    REQUIRE(K == n && K == s.n_fft && wp.fpad % wp.run == 0 && wp.run % fy == 0 && wp.run % CH == 0 && wp.fpad >= F && wp.fpad - F < wp.run, "the padded axis");
    REQUIRE(wp.gpr == wp.run / fy && (wp.gpr & (wp.gpr - 1)) == 0, "groups per run: a power of two");
    REQUIRE(pl.groups == B * wp.fpad / fy && wp.runs == B * wp.fpad / wp.run && pl.grid == (wp.runs < kFftMaxGrid ? wp.runs : kFftMaxGrid), "groups, runs, grid");
    REQUIRE(wp.chunks == (F + CH - 1) / CH && wp.blocks == (F + BLK - 1) / BLK, "chunks, blocks");
    REQUIRE(wp.ws_bytes == 8u * B * K * (wp.chunks + (wp.blocks > 1 ? wp.blocks : 0)), "workspace bytes");
    REQUIRE(wp.acc == (fy >= CH ? 0u : (n + kFftBlock - 1) / kFftBlock) && wp.acc <= kWelchCmfftMaxAcc, "accumulators");
    uint32_t lpf = 4;
    while (lpf < kFftBlock && 4u * lpf < n) lpf *= 2;
    REQUIRE(pl.lpf == lpf && fy == kFftBlock / lpf && (fy & (fy - 1)) == 0 && fy <= 32, "the mixed-radix complex layout: fy a power of two");
    REQUIRE(wp.run == (fy > CH ? fy : CH) && wp.gpr == (fy >= CH ? 1u : CH / fy), "run = max(16, fy), gpr = max(1, 16 / fy)");
    // the shifted columns are a permutation of the bins, and torch.fft.fftshift's: column j holds bin (j - n / 2) mod n
    if (turn) {
        std::vector<int> seen(n, 0);
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t j = col_of(k, turn, n);
            REQUIRE(j < n && bin_of(j, turn, n) == k && j == (k + n / 2) % n, "column %u of bin %u", j, k);
            ++seen[j];
        }
        for (uint32_t j = 0; j < n; ++j) REQUIRE(seen[j] == 1, "column %u taken %d times", j, seen[j]);
    }
    std::vector<double> q(B * F * K);
    for (auto &v : q) v = (double)(rnd() >> 20) * 0x1p-20 + 1.0;
    std::vector<double> ws(wp.ws_bytes / 8);                                                 // exactly the plan's bytes
    std::vector<int> ws_hit(ws.size(), 0), q_hit(q.size(), 0), group_hit(pl.groups, 0);
    double *chunk_ws = ws.data();
    const uint64_t n_chunk_ws = B * wp.chunks * K;
    for (uint64_t w = 0; w < pl.grid; ++w) {
        std::vector<double> acc((size_t)kFftBlock * kWelchCmfftMaxAcc, 0.0);                     // the lanes' registers
        uint64_t prev = UINT64_MAX;
        // mfft_first_group / mfft_next_group of bhw_stft_mfft.h under an epilogue that owns runs
        for (uint64_t g = w * wp.gpr; g < pl.groups; g = ((g + 1u) & (wp.gpr - 1u)) ? g + 1u : g + 1u + (pl.grid - 1u) * wp.gpr) {
            ++group_hit.at(g);
            const uint64_t r0 = g * fy, b = r0 / wp.fpad, f0 = r0 - b * wp.fpad;
            REQUIRE(b < B && f0 + fy <= wp.fpad, "a group inside one signal");
            if (prev != UINT64_MAX && (g & (wp.gpr - 1u))) REQUIRE(g == prev + 1, "a run's groups in ascending order");
            REQUIRE((g / wp.gpr) % pl.grid == w, "run %" PRIu64 " belongs to workgroup %" PRIu64, g / wp.gpr, w);
            prev = g;
            // the row map: slot live iff its frame is below F (what the loads and the accumulate step both use)
            for (uint32_t slot = 0; slot < fy; ++slot) {
                const bool live = f0 + slot < F;
                const uint64_t f = live ? f0 + slot : 0;
                REQUIRE(f < F, "a live row's frame");
            }
            // the accumulate step, every lane; an LDS slot index stays below fy, a point index below n
            if (fy >= CH) {
                const uint32_t pairs = (fy / CH) * n;
                for (uint32_t tid = 0; tid < kFftBlock; ++tid)
                    for (uint32_t i = tid; i < pairs; i += kFftBlock) {
                        const uint32_t c = i / n, k = i - c * n;
                        const uint64_t fc = f0 + (uint64_t)c * CH;
                        if (fc >= F) continue;
                        const uint32_t m = F - fc < CH ? (uint32_t)(F - fc) : CH;
                        double A = 0.0;
                        for (uint32_t sl = 0; sl < m; ++sl) {
                            const uint32_t slot = c * CH + sl;
                            REQUIRE(slot < fy && k < n && f0 + slot < F, "the slot read is live");
                            const uint64_t qi = (b * F + f0 + slot) * K + k;
                            A += q.at(qi);
                            ++q_hit[qi];
                        }
                        const uint64_t wi = (b * wp.chunks + fc / CH) * K + col_of(k, turn, n);
                        REQUIRE(wi < n_chunk_ws, "chunk sum %" PRIu64 " of %" PRIu64, wi, n_chunk_ws);
                        chunk_ws[wi] = A;
                        ++ws_hit.at(wi);
                    }
            } else {
                const uint32_t m = f0 >= F ? 0u : F - f0 < fy ? (uint32_t)(F - f0) : fy;
                const bool last = ((g + 1u) & (wp.gpr - 1u)) == 0u;
                REQUIRE(f0 / CH < wp.chunks && (b * wp.chunks + f0 / CH + 1) * K <= n_chunk_ws, "the pointer every group of the run forms stays inside");
                for (uint32_t tid = 0; tid < kFftBlock; ++tid)
                    for (uint32_t i = 0; i < kWelchCmfftMaxAcc; ++i) {
                        const uint32_t k = tid + i * kFftBlock;
                        if (k >= n) continue;
                        REQUIRE(i < wp.acc, "accumulator %u of %u, bin %u", i, wp.acc, k);
                        double A = acc[(size_t)tid * kWelchCmfftMaxAcc + i];
                        for (uint32_t sl = 0; sl < m; ++sl) {
                            REQUIRE(sl < fy, "a slot of the group");
                            const uint64_t qi = (b * F + f0 + sl) * K + k;
                            A += q.at(qi);
                            ++q_hit[qi];
                        }
                        if (last) {
                            REQUIRE((f0 + fy) % CH == 0 && f0 / CH == (f0 + fy - CH) / CH && f0 / CH * CH < F, "the run's chunk exists");
                            const uint64_t wi = (b * wp.chunks + f0 / CH) * K + col_of(k, turn, n);
                            REQUIRE(wi < n_chunk_ws, "chunk sum %" PRIu64 " of %" PRIu64, wi, n_chunk_ws);
                            chunk_ws[wi] = A;
                            ++ws_hit.at(wi);
                            A = 0.0;
                        }
                        acc[(size_t)tid * kWelchCmfftMaxAcc + i] = A;
                    }
            }
        }
        for (double a : acc) REQUIRE(a == 0.0, "nothing is carried out of a workgroup's last run");
    }
    for (uint64_t g = 0; g < pl.groups; ++g) REQUIRE(group_hit[g] == 1, "group %" PRIu64 " visited %d times", g, group_hit[g]);
    for (size_t i = 0; i < q.size(); ++i) REQUIRE(q_hit[i] == 1, "q %zu added %d times", i, q_hit[i]);
    for (uint64_t i = 0; i < n_chunk_ws; ++i) REQUIRE(ws_hit[i] == 1, "chunk sum %" PRIu64 " written %d times", i, ws_hit[i]);
    // ascending f from +0.0 inside every chunk: the stored sums are the plain loops', at the bin's column
    for (uint64_t b = 0; b < B; ++b)
        for (uint64_t c = 0; c < wp.chunks; ++c)
            for (uint64_t k = 0; k < K; k += (K > 40 ? 37 : 1)) {
                double Ac = 0.0;
                for (uint64_t f = c * CH; f < F && f < (c + 1) * CH; ++f) Ac += q[(b * F + f) * K + k];
                REQUIRE(memcmp(&Ac, &chunk_ws[(b * wp.chunks + c) * K + col_of(k, turn, n)], 8) == 0, "chunk sum (%" PRIu64 ", %" PRIu64 ", %" PRIu64 ")", b, c, k);
            }
    // the join: bins = n_fft, flags 0
    const uint64_t ps = wp.p_stride;
    std::vector<float> P((B - 1) * ps + K, -1.0f);
    std::vector<int> P_hit(P.size(), 0);
    std::vector<double> chunk_in(ws.begin(), ws.begin() + n_chunk_ws);
    if (wp.blocks == 1) {
        REQUIRE(wp.join_grid == 0, "one launch");
        replay_join(true, true, chunk_in, nullptr, nullptr, P, P_hit, B, K, s.n_fft, wp.chunks, 1, ps, scale, 0, wp.blocks_grid);
    } else {
        std::vector<double> blk(ws.size() - n_chunk_ws);                                        // what follows the chunk sums, exactly
        std::vector<int> blk_hit(blk.size(), 0);
        REQUIRE(blk.size() == B * wp.blocks * K, "the block sums follow the chunk sums");
        replay_join(true, false, chunk_in, &blk, &blk_hit, P, P_hit, B, K, s.n_fft, wp.chunks, wp.blocks, ps, scale, 0, wp.blocks_grid);
        for (size_t i = 0; i < blk.size(); ++i) REQUIRE(blk_hit[i] == 1, "block sum %zu written %d times", i, blk_hit[i]);
        replay_join(false, true, blk, nullptr, nullptr, P, P_hit, B, K, s.n_fft, wp.blocks, 1, ps, scale, 0, wp.join_grid);
    }
    for (uint64_t b = 0; b < B; ++b)
        for (uint64_t j = 0; j < ps && b * ps + j < P.size(); ++j) {
            REQUIRE(P_hit[b * ps + j] == (j < K ? 1 : 0), "P (%" PRIu64 ", %" PRIu64 ") written %d times", b, j, P_hit[b * ps + j]);
            if (j >= K) continue;
            const uint64_t k = bin_of((uint32_t)j, turn, n);                                        // column j holds bin (j + n - n / 2) mod n
            const float want = (float)(contract_sum(q, b, F, K, k) * scale);
            REQUIRE(memcmp(&want, &P[b * ps + j], 4) == 0, "P (%" PRIu64 ", %" PRIu64 "): %a != %a", b, j, P[b * ps + j], want);
        }
}

// chunk sums -> block sums -> A as the kernels associate them, against the contract's loops, on random positive doubles
static void three_levels(uint64_t F)
{
    std::vector<double> q(F);
    for (auto &v : q) v = ldexp((double)(rnd() >> 11) + 1.0, (int)(rnd() % 80) - 60);
    const uint64_t chunks = (F + CH - 1) / CH, blocks = (F + BLK - 1) / BLK;
    std::vector<double> cs(chunks), bs(blocks);
    for (uint64_t c = 0; c < chunks; ++c) {                                                      // as a lane carries it: group by group
        double A = 0.0;
        for (uint64_t f = c * CH; f < F && f < (c + 1) * CH; ++f) A += q[f];
        cs[c] = A;
    }
    for (uint64_t b = 0; b < blocks; ++b) {
        double A = 0.0;
        for (uint64_t c = b * (BLK / CH); c < chunks && c < (b + 1) * (BLK / CH); ++c) A += cs[c];
        bs[b] = A;
    }
    double A = 0.0;
    for (uint64_t b = 0; b < blocks; ++b) A += bs[b];
    if (blocks == 1) A = bs[0];                                                                 // one launch: the block sum IS A
    const double want = contract_sum(q, 0, F, 1, 0);
    REQUIRE(memcmp(&A, &want, 8) == 0, "F %" PRIu64 ": %a != %a", F, A, want);
    if (F <= CH) {                                                                              // the plain ascending sum of bhw_welch_psd_f32
        double S = 0.0;
        for (uint64_t f = 0; f < F; ++f) S += q[f];
        REQUIRE(memcmp(&S, &want, 8) == 0, "F %" PRIu64 " <= 16: the plain sum", F);
    }
}

int main()
{
    char buf[1400];
    long replays = 0, sizes = 0;
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 12, 24);
    const uint64_t xa = 0x10000000ull, pa = 0x100000000000ull, wa = 0x200000000000ull;
    for (uint64_t n = 1; n <= 2100; ++n) {
        if (!bhwp_cmfft_supported(n)) {
            bhw_stft s = desc_of(1, 1ull << 20, 2, 1, n, 0, 0, 0);
            REQUIRE(bhwp_welch_cmfft_checks(&p, 1, &s, 0, 1.0, 0, nullptr, nullptr, nullptr, 0, false) == (n ? BHW_ERR_UNSUPPORTED : BHW_ERR_BADARG),
                    "n_fft %" PRIu64, n);
            continue;
        }
        ++sizes;
        for (uint64_t L : {(uint64_t)13, n})
            for (uint64_t hop : {(uint64_t)7, n + 5})
                for (uint64_t B : {1ull, 3ull})
                    // the edges of a chunk (16), of a run of two chunks (32, n_fft <= 30) and of a block (256)
                    for (uint64_t F : {1ull, 15ull, 16ull, 17ull, 31ull, 32ull, 33ull, 65ull, 256ull, 257ull, 531ull})
                        for (int framing = 0; framing < 3; ++framing) {                   // 0 Welch + detrend, 1 Welch, 2 centred reflect
                            const bool centred = framing >= 2;
                            const uint64_t pad = centred ? n / 2 : 0, col0 = centred ? (n - L) / 2 : 0;
                            const uint64_t reach = centred ? n : L;
                            uint64_t T = (F - 1) * hop + reach;
                            T = T > 2 * pad ? T - 2 * pad : 1;
                            if (centred && (T + 2 * pad < (F - 1) * hop + n || pad > T - 1)) continue;
                            const uint32_t shiftf = (B + F + framing) % 2 ? BHW_CFFT_SHIFT : 0u;
                            const uint32_t flags = (framing == 0 ? BHW_WELCH_DETREND_CONSTANT : 0u) | shiftf;
                            bhw_stft s = desc_of(B, T, F, hop, n, col0, pad, framing == 2 ? BHW_PAD_REFLECT : BHW_PAD_CONSTANT);
                            const uint64_t ps = (B + F) % 3 == 0 ? n + 5 : 0;
                            const uint64_t need = bhwp_welch_cmfft_workspace_bytes(&s);
                            int rc = bhwp_welch_cmfft_checks(&p, L, &s, flags, 0.5, ps, nullptr, nullptr, nullptr, 0, false);
                            REQUIRE(rc == BHW_OK, "checks rc %d: n %" PRIu64 " L %" PRIu64 " hop %" PRIu64 " B %" PRIu64 " F %" PRIu64 " framing %d: %s", rc, n, L, hop, B, F, framing, bhw_last_error());
                            REQUIRE(bhwp_stft_cmfft_checks(&p, L, &s, flags, nullptr, nullptr, false) == BHW_OK, "the forward checks agree");
                            auto full = [&](const bhw_stft &d, uint32_t fl, double scale, uint64_t pstr, uint64_t x, uint64_t P, uint64_t w, uint64_t wb) {
                                return bhwp_welch_cmfft_checks(&p, L, &d, fl, scale, pstr, (const void *)x, (const void *)P, (const void *)w, wb);
                            };
                            REQUIRE(full(s, flags, 0.5, ps, xa, pa, wa, need) == BHW_OK, "pointer checks: %s", bhw_last_error());
                            REQUIRE(full(s, flags, 0.5, ps, xa + 4, pa + 4, wa, need + 8) == BHW_OK, "4-byte aligned x and P");
                            REQUIRE(full(s, flags, 0.5, ps, xa, pa + 2, wa, need) == BHW_ERR_BADARG, "misaligned P");
                            REQUIRE(full(s, flags, 0.5, ps, xa + 1, pa, wa, need) == BHW_ERR_BADARG, "misaligned x");
                            REQUIRE(full(s, flags, 0.5, ps, xa, pa, wa + 4, need) == BHW_ERR_BADARG, "misaligned workspace");
                            REQUIRE(full(s, flags, 0.5, ps, xa, pa, 0, need) == BHW_ERR_BADARG, "NULL workspace");
                            REQUIRE(full(s, flags, 0.5, ps, xa, pa, wa, need - 1) == BHW_ERR_WORKSPACE, "short workspace");
                            REQUIRE(full(s, flags, 0.5, ps, pa, pa, wa, need) == BHW_ERR_BADARG, "x on P");
                            REQUIRE(full(s, flags, 0.5, ps, xa, pa, xa, need) == BHW_ERR_BADARG, "workspace on x");
                            REQUIRE(full(s, flags, 0.5, ps, xa, wa + need - 4, wa, need) == BHW_ERR_BADARG, "P on the workspace's end");
                            REQUIRE(full(s, flags, 0.5, ps, xa, wa + need, wa, need) == BHW_OK, "P behind the workspace");
                            REQUIRE(full(s, flags | BHW_CFFT_POWER, 0.5, ps, xa, pa, wa, need) == BHW_ERR_BADARG, "BHW_CFFT_POWER");
                            REQUIRE(full(s, flags | 8u, 0.5, ps, xa, pa, wa, need) == BHW_ERR_BADARG, "unknown flags");
                            REQUIRE(full(s, flags, INFINITY, ps, xa, pa, wa, need) == BHW_ERR_BADARG && full(s, flags, NAN, ps, xa, pa, wa, need) == BHW_ERR_BADARG, "scale");
                            REQUIRE(full(s, flags, 0.5, n - 1, xa, pa, wa, need) == BHW_ERR_BADARG, "short p_stride");
                            bhw_stft bad = s;
                            bad.y_stride = 2 * n + 2;
                            REQUIRE(full(bad, flags, 0.5, ps, xa, pa, wa, need) == BHW_ERR_BADARG, "y_stride");
                            bad = s;
                            bad.y_batch_stride = F * (2 * n + 2);
                            REQUIRE(full(bad, flags, 0.5, ps, xa, pa, wa, need) == BHW_ERR_BADARG, "y_batch_stride");
                            bad = s;
                            bad.channels = 1;
                            REQUIRE(full(bad, flags, 0.5, ps, xa, pa, wa, need) == BHW_ERR_UNSUPPORTED, "channels");
                            bad = s;
                            bad.frames = 0;
                            REQUIRE(bhwp_welch_cmfft_checks(&p, L, &bad, flags, 0.5, ps, nullptr, nullptr, nullptr, 0) == BHW_OK, "frames 0");
                            REQUIRE(bhwp_welch_cmfft_workspace_bytes(&bad) == 0, "frames 0 needs no workspace");
                            REQUIRE(bhwp_describe_welch_cmfft(&p, nullptr, L, &bad, flags, buf, sizeof buf) == BHW_OK, "describe frames 0");
                            const BhwWelchCmfftPlan z = bhwp_welch_cmfft_plan(&p, L, &bad, flags, ps, false);
                            REQUIRE(z.fft.rows == 0 && z.fft.groups == 0 && z.fft.grid == 0 && z.runs == 0 && z.ws_bytes == 0, "the plan of nothing");
                            const BhwWelchCmfftPlan wp = bhwp_welch_cmfft_plan(&p, L, &s, flags, ps, (B + F) % 2 == 0);
                            const BhwStftCmfftPlan fw = bhwp_stft_cmfft_plan(&p, L, &s, flags, (B + F) % 2 == 0);
                            REQUIRE(wp.fft.lpf == fw.lpf && wp.fft.fy == fw.fy && wp.fft.cpl == fw.cpl && wp.fft.passes == fw.passes &&
                                    memcmp(wp.fft.radix, fw.radix, sizeof fw.radix) == 0 && wp.fft.fold == fw.fold &&
                                    wp.fft.lds_bytes == fw.lds_bytes && wp.fft.rows == fw.rows && wp.fft.n == fw.n && wp.fft.x_stride == fw.x_stride &&
                                    wp.fft.route == fw.route && wp.fft.detrend == fw.detrend && wp.fft.shifted == fw.shifted &&
                                    wp.fft.len == fw.len && !wp.fft.power && !wp.fft.y_stride && !wp.fft.y_bstride,
                                    "the forward plan's lanes, LDS and schedule, field for field");
                            const BhwWelchRuns r = bhwp_welch_runs(B, F, fw.fy, n);
                            REQUIRE(wp.run == r.run && wp.gpr == r.gpr && wp.fpad == r.fpad && wp.chunks == r.chunks && wp.blocks == r.blocks && wp.runs == r.runs &&
                                    wp.fft.groups == r.groups && wp.fft.grid == r.grid && wp.blocks_grid == r.blocks_grid && wp.join_grid == r.join_grid &&
                                    wp.ws_bytes == r.ws_bytes, "the shared run arithmetic");
                            REQUIRE(wp.ws_bytes == need && wp.p_stride == (ps ? ps : n), "workspace and p_stride");
                            REQUIRE(bhwp_describe_welch_cmfft(&p, nullptr, L, &s, flags, buf, sizeof buf) == BHW_OK && strlen(buf) > 80 && strlen(buf) < sizeof buf - 1, "describe");
                            REQUIRE(strstr(buf, "accumulator") && strstr(buf, "chunk 16 frames") && strstr(buf, "workspace") && strstr(buf, "twiddles") &&
                                    strstr(buf, shiftf ? "bins shifted" : "bins in order"), "the line's own fields in %s", buf);
                            // every size is replayed at the edges of a chunk and a run, with one signal and with three, shifted and not;
                            // the edges of a block at the sizes up to 256, where the q array stays small
                            if (hop == 7 && L == n && framing == (int)((B + F) % 2) && (F <= 65 || n <= 256)) {
                                replay_call(wp, s, 1.0 / (3.7 * (double)F));
                                ++replays;
                            }
                        }
    }
    REQUIRE(sizes == 91, "supported sizes %ld", sizes);
    for (uint32_t flags : {0u, (uint32_t)BHW_CFFT_SHIFT}) {   // more runs than workgroups, 513 blocks through the join: 18 / 16 / 2, 131 142 frames
        bhw_stft s = desc_of(1, 262300, 131142, 2, 18, 1, 0, 0);
        REQUIRE(bhwp_welch_cmfft_checks(&p, 16, &s, flags, 1.0, 0, nullptr, nullptr, nullptr, 0, false) == BHW_OK, "the long case: %s", bhw_last_error());
        const BhwWelchCmfftPlan wp = bhwp_welch_cmfft_plan(&p, 16, &s, flags, 0, false);
        REQUIRE(wp.runs > kFftMaxGrid && wp.fft.grid == kFftMaxGrid && wp.blocks == 513 && wp.fft.fy == 32, "runs %" PRIu64 " blocks %" PRIu64, wp.runs, wp.blocks);
        replay_call(wp, s, 0.25);
        ++replays;
    }
    {   // a signal of 2^24 samples at 2000 / 500: 2 097 chunk chains, the plan alone
        bhw_stft t2 = desc_of(1, 1ull << 24, 33551, 500, 2000, 0, 0, 0);
        const BhwWelchCmfftPlan w2 = bhwp_welch_cmfft_plan(&p, 2000, &t2, BHW_WELCH_DETREND_CONSTANT, 0, true);
        REQUIRE(w2.runs == 2097 && w2.fft.grid == 2048 && w2.chunks == 2097 && w2.blocks == 132 && w2.acc == 8 && w2.gpr == 16, "T2's plan");
    }
    REQUIRE(bhwp_welch_cmfft_checks(&p, 16, nullptr, 0, 1.0, 0, nullptr, nullptr, nullptr, 0, false) == BHW_ERR_BADARG, "NULL descriptor");
    REQUIRE(bhwp_welch_cmfft_workspace_bytes(nullptr) == 0, "NULL descriptor needs nothing");
    long sums = 0;
    for (uint64_t F = 1; F <= 1200; ++F, ++sums) three_levels(F);
    for (uint64_t F : {4095ull, 4096ull, 4097ull, 16381ull, 131142ull}) three_levels(F), ++sums;
    REQUIRE(replays >= 91 * 8, "replays %ld", replays);
    printf("ok %ld checks, %ld call replays over %ld sizes, %ld three-level sums\n", g_checks, replays, sizes, sums);
    return 0;
}
