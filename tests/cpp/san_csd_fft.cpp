// san_csd_fft.cpp -- the planner's part of the fused Welch cross spectra (bhw_plan.cpp: bhwp_csd_fft_checks / bhwp_csd_fft_plan /
// bhwp_csd_fft_workspace_bytes / bhwp_describe_csd_fft) swept under AddressSanitizer + UBSan, and a host replay, lane by lane, of what
// bhw_csd_fft.hip does with the plan:
//   - the slot -> (operand, frame) map and run ownership: workgroup w walks the groups first(w), next(...) of stft_fft_rows under an
//     epilogue that owns runs of frame pairs; every group of the padded pool is visited exactly once, by one workgroup, a run's groups
//     in ascending order and never across a signal; the first fy / 2 slots are x, the others y, slot s and slot pairs + s carry the
//     same frame, and a slot is live exactly when its frame is below F; under broadcast x is read from signal 0 only;
//   - the accumulate step, both regimes, on four term arrays of exactly B * F * K doubles and a workspace of exactly the plan's bytes:
//     every chunk sum of every chain is written exactly once, every read and write stays inside, and every (b, f < F, k) is added
//     exactly once per chain, in ascending f inside its chunk;
//   - the join: k_welch_fft_join<true, false> over 4 K bins (several blocks) and k_csd_fft_out lane by lane over the same workspace,
//     every block sum and every output written once, an output's row inside o_stride, outputs not asked for untouched, and the
//     outputs equal bit for bit to the contract restated as three plain loops per chain and the formulas of bhw_welch_csd_f32.
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
    s.channels = 1;
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

constexpr uint32_t CH = BHW_WELCH_FFT_CHUNK, BLK = BHW_WELCH_BLOCK, NC = kCsdFftChains;
static const uint32_t kBits[kCsdOutputs] = {BHW_CSD_PXY, BHW_CSD_PXX, BHW_CSD_PYY, BHW_CSD_COHERENCE, BHW_CSD_H1};
static const uint32_t kWidth[kCsdOutputs] = {2, 1, 1, 1, 2};          // floats per element

// the contract of include/bhw.h as three plain loops over t[(b * F + f) * K + k]
static double contract_sum(const std::vector<double> &t, uint64_t b, uint64_t F, uint64_t K, uint64_t k)
{
    double A = 0.0;
    for (uint64_t f0 = 0; f0 < F; f0 += BLK) {
        double Ab = 0.0;
        for (uint64_t c0 = f0; c0 < F && c0 < f0 + BLK; c0 += CH) {
            double Ac = 0.0;
            for (uint64_t f = c0; f < F && f < c0 + CH; ++f) Ac += t.at((b * F + f) * K + k);
            Ab += Ac;
        }
        A += Ab;
    }
    return A;
}

// the output formulas of bhw_welch_csd_f32 (include/bhw.h), unfused: out[i][0..width)
static void contract_out(const double *S, double scale, uint32_t flags, uint64_t k, uint64_t K, uint64_t n_fft, float out[kCsdOutputs][2])
{
    const double sk = bhw_psd_doubled(flags & BHW_CSD_ONESIDED ? BHW_PSD_ONESIDED : 0u, k, K, n_fft) ? scale * 2.0 : scale;
    const volatile double sxx = S[0], syy = S[1], cre = S[2], cim = S[3];
    out[0][0] = (float)(cre * sk), out[0][1] = (float)(cim * sk);
    out[1][0] = (float)(sxx * sk);
    out[2][0] = (float)(syy * sk);
    const volatile double n = cre * cre, m = cim * cim;
    const volatile double num = n + m, den = sxx * syy;
    out[3][0] = (float)(num / den);
    out[4][0] = (float)(cre / sxx), out[4][1] = (float)(cim / sxx);
}

// k_welch_fft_join<true, false> over `bins` bins, every lane of every workgroup
static void replay_join_blocks(const std::vector<double> &in, std::vector<double> &out, std::vector<int> &out_hit, uint64_t batch, uint64_t bins,
                               uint64_t n_in, uint64_t n_out, uint64_t grid)
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
            const uint64_t i0 = o * U, i1 = i0 + U < n_in ? i0 + U : n_in;
            REQUIRE(i0 < i1, "an output with no input");
            double A = 0.0;
            for (uint64_t j = i0; j < i1; j += U) {
                double v[U];
                for (uint32_t u = 0; u < U; ++u) v[u] = in.at(base + (j + u < i1 ? j + u : i1 - 1u) * bins);
                for (uint32_t u = 0; u < U; ++u)
                    if (j + u < i1) A += v[u];
            }
            out.at((b * n_out + o) * bins + k) = A;
            ++out_hit.at((b * n_out + o) * bins + k);
        }
}

// One call, lane by lane.  t[c]: B * F * K doubles standing for the terms of chain c of the transformed rows.
static void replay_call(const BhwCsdFftPlan &cp, const bhw_stft &s, double scale)
{
    const BhwStftFftPlan &pl = cp.fft;
    const uint64_t B = s.batch, F = s.frames, K = cp.bins, row = NC * K;
    const uint32_t fy = pl.fy, M = pl.m, pairs = cp.pairs;
    REQUIRE(fy >= 2 && pairs == fy / 2 && pl.lpf * fy == kFftBlock && pl.lpf <= kCsdFftMaxLpf && pl.cpl <= kFftMaxCpl && pl.lds_bytes <= 65536, "x and y side by side");
    REQUIRE(K == (uint64_t)M + 1 && cp.fpad % cp.run == 0 && cp.run % pairs == 0 && cp.run % CH == 0 && cp.fpad >= F && cp.fpad - F < cp.run, "the padded axis");
    REQUIRE(cp.run == (pairs > CH ? pairs : CH) && cp.gpr == cp.run / pairs && (cp.gpr & (cp.gpr - 1)) == 0, "groups per run: a power of two");
    REQUIRE(pl.groups == B * cp.fpad / pairs && cp.runs == B * cp.fpad / cp.run && pl.grid == (cp.runs < kFftMaxGrid ? cp.runs : kFftMaxGrid), "groups, runs, grid");
    REQUIRE(cp.chunks == (F + CH - 1) / CH && cp.blocks == (F + BLK - 1) / BLK, "chunks, blocks");
    REQUIRE(cp.ws_bytes == 8u * B * row * (cp.chunks + (cp.blocks > 1 ? cp.blocks : 0)), "workspace bytes");
    REQUIRE(cp.acc == (pairs >= CH ? 0u : (uint32_t)((K + kFftBlock - 1) / kFftBlock)) && cp.acc <= kCsdFftMaxAcc, "accumulators");
    const bool bcast = (cp.flags & BHW_CSD_BROADCAST_X) != 0;
    std::vector<double> t[NC];
    for (uint32_t c = 0; c < NC; ++c) {
        t[c].resize(B * F * K);
        for (auto &v : t[c]) v = ((double)(rnd() >> 20) * 0x1p-20 + 1.0) * (c >= 2 && (rnd() & 1) ? -1.0 : 1.0);
    }
    std::vector<double> ws(cp.ws_bytes / 8);                                                 // exactly the plan's bytes
    std::vector<int> ws_hit(ws.size(), 0), t_hit(B * F * K * NC, 0), group_hit(pl.groups, 0);
    double *chunk_ws = ws.data();
    const uint64_t n_chunk_ws = B * cp.chunks * row;
    auto add = [&](double *S, uint64_t b, uint64_t f, uint32_t k) {                          // csd_fft_add of one (bin, frame)
        REQUIRE(b < B && f < F && k <= M, "a live frame's bin");
        const uint64_t ti = (b * F + f) * K + k;
        for (uint32_t c = 0; c < NC; ++c) {
            S[c] += t[c].at(ti);
            ++t_hit.at(ti * NC + c);
        }
    };
    auto store = [&](uint64_t b, uint64_t chunk, uint32_t k, const double *S) {
        for (uint32_t c = 0; c < NC; ++c) {
            const uint64_t wi = (b * cp.chunks + chunk) * row + (uint64_t)c * K + k;
            REQUIRE(chunk < cp.chunks && wi < n_chunk_ws, "chunk sum %" PRIu64 " of %" PRIu64, wi, n_chunk_ws);
            chunk_ws[wi] = S[c];
            ++ws_hit.at(wi);
        }
    };
    for (uint64_t w = 0; w < pl.grid; ++w) {
        std::vector<double> acc((size_t)kFftBlock * kCsdFftMaxAcc * NC, 0.0);                   // the lanes' registers
        uint64_t prev = UINT64_MAX;
        // fft_first_group / fft_next_group of bhw_stft_fft.h under an epilogue that owns runs
        for (uint64_t g = w * cp.gpr; g < pl.groups; g = ((g + 1u) & (cp.gpr - 1u)) ? g + 1u : g + 1u + (pl.grid - 1u) * cp.gpr) {
            ++group_hit.at(g);
            const uint64_t r0 = g * pairs, b = r0 / cp.fpad, f0 = r0 - b * cp.fpad;
            REQUIRE(b < B && f0 + pairs <= cp.fpad, "a group inside one signal");
            if (prev != UINT64_MAX && (g & (cp.gpr - 1u))) REQUIRE(g == prev + 1, "a run's groups in ascending order");
            REQUIRE((g / cp.gpr) % pl.grid == w, "run %" PRIu64 " belongs to workgroup %" PRIu64, g / cp.gpr, w);
            prev = g;
            // the slot map of stft_fft_rows under kPairs: operand, frame, live, and the signal each operand reads
            for (uint32_t slot = 0; slot < fy; ++slot) {
                const bool second = slot >= pairs;
                const uint32_t fs = second ? slot - pairs : slot;
                const bool live = f0 + fs < F;
                const uint64_t f = live ? f0 + fs : 0;
                const uint64_t sig = second ? b : (bcast ? 0 : b);
                REQUIRE(f < F && fs < pairs && sig < (second || !bcast ? B : 1), "a live row's frame and signal");
                REQUIRE(live == (f0 + fs < F) && (!live || f == f0 + fs), "slot %u and slot %u carry the same frame", fs, pairs + fs);
            }
            // the accumulate step, every lane
            if (pairs >= CH) {
                const uint32_t units = (pairs / CH) * (uint32_t)K;
                for (uint32_t tid = 0; tid < kFftBlock; ++tid)
                    for (uint32_t i = tid; i < units; i += kFftBlock) {
                        const uint32_t c = i / (uint32_t)K, k = i - c * (uint32_t)K;
                        const uint64_t fc = f0 + (uint64_t)c * CH;
                        if (fc >= F) continue;
                        const uint32_t n = F - fc < CH ? (uint32_t)(F - fc) : CH;
                        double S[NC] = {0.0, 0.0, 0.0, 0.0};
                        for (uint32_t sl = 0; sl < n; ++sl) {
                            REQUIRE(c * CH + sl < pairs, "the slot pair read is inside the group");
                            add(S, b, fc + sl, k);
                        }
                        store(b, fc / CH, k, S);
                    }
            } else {
                const uint32_t n = f0 >= F ? 0u : F - f0 < pairs ? (uint32_t)(F - f0) : pairs;
                const bool last = ((g + 1u) & (cp.gpr - 1u)) == 0u;
                REQUIRE(f0 / CH < cp.chunks && (b * cp.chunks + f0 / CH + 1) * row <= n_chunk_ws, "the pointer every group of the run forms stays inside");
                const bool wide = M >= kFftBlock;
                auto lane_bin = [&](uint32_t tid, uint32_t i, uint32_t k) {                     // accumulators i of lane tid own bin k
                    REQUIRE(i < cp.acc && i < kCsdFftMaxAcc && k <= M, "accumulator %u of %u, bin %u", i, cp.acc, k);
                    double *S = &acc[((size_t)tid * kCsdFftMaxAcc + i) * NC];
                    for (uint32_t sl = 0; sl < n; ++sl) add(S, b, f0 + sl, k);
                    if (last) {
                        REQUIRE((f0 + pairs) % CH == 0 && f0 / CH * CH < F, "the run's chunk exists");
                        store(b, f0 / CH, k, S);
                        for (uint32_t c = 0; c < NC; ++c) S[c] = 0.0;
                    }
                };
                for (uint32_t tid = 0; tid < kFftBlock; ++tid) {
                    for (uint32_t i = 0; i < kCsdFftMaxAcc - 1u; ++i) {
                        const uint32_t k = tid + i * kFftBlock;
                        if (wide ? k < M : k <= M) lane_bin(tid, i, k);
                    }
                    if (wide && tid == 0u) lane_bin(0, M / kFftBlock, M);                   // acc_m: lane 0's last, aside from acc[]
                }
            }
        }
        for (double a : acc) REQUIRE(a == 0.0, "nothing is carried out of a workgroup's last run");
    }
    for (uint64_t g = 0; g < pl.groups; ++g) REQUIRE(group_hit[g] == 1, "group %" PRIu64 " visited %d times", g, group_hit[g]);
    for (size_t i = 0; i < t_hit.size(); ++i) REQUIRE(t_hit[i] == 1, "term %zu added %d times", i, t_hit[i]);
    for (uint64_t i = 0; i < n_chunk_ws; ++i) REQUIRE(ws_hit[i] == 1, "chunk sum %" PRIu64 " written %d times", i, ws_hit[i]);
    // ascending f from +0.0 inside every chunk: the stored sums are the plain loops'
    for (uint64_t b = 0; b < B; ++b)
        for (uint64_t c = 0; c < cp.chunks; ++c)
            for (uint32_t ch = 0; ch < NC; ++ch)
                for (uint64_t k = 0; k < K; k += (K > 40 ? 37 : 1)) {
                    double Ac = 0.0;
                    for (uint64_t f = c * CH; f < F && f < (c + 1) * CH; ++f) Ac += t[ch][(b * F + f) * K + k];
                    REQUIRE(memcmp(&Ac, &chunk_ws[(b * cp.chunks + c) * row + ch * K + k], 8) == 0, "chunk sum (%" PRIu64 ", %" PRIu64 ", %u, %" PRIu64 ")", b, c, ch, k);
                }
    // the join
    const uint64_t os = cp.o_stride;
    std::vector<float> out[kCsdOutputs];
    std::vector<int> out_hit[kCsdOutputs];
    for (uint32_t i = 0; i < kCsdOutputs; ++i)
        if (cp.flags & kBits[i]) {                                                              // an output not asked for has no array at all
            out[i].assign(((B - 1) * os + K) * kWidth[i], -1.0f);
            out_hit[i].assign((B - 1) * os + K, 0);
        }
    std::vector<double> last_in(ws.begin(), ws.begin() + n_chunk_ws);
    uint64_t n_in = cp.chunks;
    if (cp.blocks > 1) {
        std::vector<double> blk(ws.size() - n_chunk_ws);                                        // what follows the chunk sums, exactly
        std::vector<int> blk_hit(blk.size(), 0);
        REQUIRE(blk.size() == B * cp.blocks * row, "the block sums follow the chunk sums");
        replay_join_blocks(last_in, blk, blk_hit, B, row, cp.chunks, cp.blocks, cp.blocks_grid);
        for (size_t i = 0; i < blk.size(); ++i) REQUIRE(blk_hit[i] == 1, "block sum %zu written %d times", i, blk_hit[i]);
        last_in = blk;
        n_in = cp.blocks;
    } else {
        REQUIRE(cp.blocks_grid == 0 && n_in <= BLK / CH, "one block: the chunks go straight to the outputs");
    }
    // k_csd_fft_out, every lane of every workgroup
    REQUIRE(cp.out_grid * 256u >= B * K && (cp.out_grid - 1) * 256u < B * K, "out grid %" PRIu64, cp.out_grid);
    for (uint64_t wg = 0; wg < cp.out_grid; ++wg)
        for (uint32_t tt = 0; tt < 256; ++tt) {
            const uint64_t i = wg * 256u + tt;
            if (i >= B * K) continue;
            const uint64_t b = i / K, k = i - b * K;
            const uint64_t base = b * n_in * row + k;
            double S[NC] = {0.0, 0.0, 0.0, 0.0};
            constexpr uint32_t U = 4;
            for (uint64_t j = 0; j < n_in; j += U) {
                double v[U][NC];
                for (uint32_t u = 0; u < U; ++u)
                    for (uint32_t c = 0; c < NC; ++c) v[u][c] = last_in.at(base + (j + u < n_in ? j + u : n_in - 1u) * row + c * K);
                for (uint32_t u = 0; u < U; ++u)
                    if (j + u < n_in)
                        for (uint32_t c = 0; c < NC; ++c) S[c] += v[u][c];
            }
            float o[kCsdOutputs][2];
            contract_out(S, scale, cp.flags, k, K, s.n_fft, o);
            REQUIRE(k < os, "an output's row inside o_stride");
            for (uint32_t q = 0; q < kCsdOutputs; ++q)
                if (cp.flags & kBits[q]) {
                    for (uint32_t e = 0; e < kWidth[q]; ++e) out[q].at((b * os + k) * kWidth[q] + e) = o[q][e];
                    ++out_hit[q].at(b * os + k);
                }
        }
    for (uint64_t b = 0; b < B; ++b)
        for (uint64_t k = 0; k < os && b * os + k < (B - 1) * os + K; ++k) {
            double S[NC];
            float want[kCsdOutputs][2];
            if (k < K) {
                for (uint32_t c = 0; c < NC; ++c) S[c] = contract_sum(t[c], b, F, K, k);
                contract_out(S, scale, cp.flags, k, K, s.n_fft, want);
            }
            for (uint32_t q = 0; q < kCsdOutputs; ++q) {
                if (!(cp.flags & kBits[q])) continue;
                REQUIRE(out_hit[q][b * os + k] == (k < K ? 1 : 0), "output %u (%" PRIu64 ", %" PRIu64 ") written %d times", q, b, k, out_hit[q][b * os + k]);
                if (k < K) REQUIRE(memcmp(want[q], &out[q][(b * os + k) * kWidth[q]], 4 * kWidth[q]) == 0, "output %u (%" PRIu64 ", %" PRIu64 ")", q, b, k);
            }
        }
}

int main()
{
    char buf[1600];
    long replays = 0;
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_BH4, 12, 24);
    const uint64_t xa = 0x10000000ull, ya = 0x20000000ull, oa = 0x100000000000ull, wa = 0x200000000000ull, gap = 0x1000000000ull;
    const void *outs[kCsdOutputs];
    for (uint32_t i = 0; i < kCsdOutputs; ++i) outs[i] = (const void *)(oa + i * gap);
    static const uint32_t masks[] = {BHW_CSD_PXY, kCsdOutputMask, BHW_CSD_COHERENCE | BHW_CSD_H1, BHW_CSD_PXX | BHW_CSD_PYY};
    for (uint32_t lg = kFftMinLog; lg <= kCsdFftMaxLog; ++lg) {
        const uint64_t n = 1ull << lg, K = n / 2 + 1;
        for (uint64_t L : {(uint64_t)13, n})
            for (uint64_t hop : {(uint64_t)7, n + 5})
                for (uint64_t B : {1ull, 3ull})
                    for (uint64_t F : {1ull, 15ull, 16ull, 17ull, 33ull, 65ull, 256ull, 257ull, 531ull})
                        for (int framing = 0; framing < 3; ++framing) {                   // 0 Welch + detrend, 1 Welch, 2 centred reflect
                            const bool centred = framing >= 2;
                            const uint64_t pad = centred ? n / 2 : 0, col0 = centred ? (n - L) / 2 : 0;
                            const uint64_t reach = centred ? n : L;
                            uint64_t T = (F - 1) * hop + reach;
                            T = T > 2 * pad ? T - 2 * pad : 1;
                            if (centred && (T + 2 * pad < (F - 1) * hop + n || pad > T - 1)) continue;
                            const uint32_t flags = framing == 0 ? BHW_WELCH_DETREND_CONSTANT : 0u;
                            bhw_stft s = desc_of(B, T, F, hop, n, col0, pad, framing == 2 ? BHW_PAD_REFLECT : BHW_PAD_CONSTANT);
                            const uint64_t os = (B + F) % 3 == 0 ? K + 5 : 0;
                            const uint32_t cf = masks[(lg + F + B) % 4] | ((F & 1) ? BHW_CSD_ONESIDED : 0u) | (B > 1 && (F % 5) == 0 ? BHW_CSD_BROADCAST_X : 0u);
                            const uint64_t need = bhwp_csd_fft_workspace_bytes(&s);
                            REQUIRE(need == 4 * bhwp_welch_fft_workspace_bytes(&s), "four times the Welch workspace");
                            int rc = bhwp_csd_fft_checks(&p, L, &s, flags, 0.5, cf, os, nullptr, nullptr, nullptr, nullptr, 0, false);
                            REQUIRE(rc == BHW_OK, "checks rc %d: n %" PRIu64 " L %" PRIu64 " hop %" PRIu64 " B %" PRIu64 " F %" PRIu64 " framing %d: %s", rc, n, L, hop, B, F, framing, bhw_last_error());
                            REQUIRE(bhwp_welch_fft_checks(&p, L, &s, flags, 0.5, 1, os, nullptr, nullptr, nullptr, 0, false) == BHW_OK, "the Welch checks agree");
                            auto full = [&](const bhw_stft &d, double scale, uint32_t f2, uint64_t ostr, uint64_t x, uint64_t y, const void *const *o, uint64_t w, uint64_t wb) {
                                return bhwp_csd_fft_checks(&p, L, &d, flags, scale, f2, ostr, (const void *)x, (const void *)y, o, (const void *)w, wb);
                            };
                            REQUIRE(full(s, 0.5, cf, os, xa, ya, outs, wa, need) == BHW_OK, "pointer checks: %s", bhw_last_error());
                            REQUIRE(full(s, 0.5, cf, os, xa, xa, outs, wa, need + 8) == BHW_OK, "x and y may coincide");
                            REQUIRE(full(s, 0.5, cf, os, xa + 2, ya, outs, wa, need) == BHW_ERR_BADARG, "misaligned x");
                            REQUIRE(full(s, 0.5, cf, os, xa, ya + 1, outs, wa, need) == BHW_ERR_BADARG, "misaligned y");
                            REQUIRE(full(s, 0.5, cf, os, 0, ya, outs, wa, need) == BHW_ERR_BADARG && full(s, 0.5, cf, os, xa, 0, outs, wa, need) == BHW_ERR_BADARG, "NULL operands");
                            REQUIRE(full(s, 0.5, cf, os, xa, ya, outs, wa + 4, need) == BHW_ERR_BADARG, "misaligned workspace");
                            REQUIRE(full(s, 0.5, cf, os, xa, ya, outs, 0, need) == BHW_ERR_BADARG, "NULL workspace");
                            REQUIRE(full(s, 0.5, cf, os, xa, ya, outs, wa, need - 1) == BHW_ERR_WORKSPACE, "short workspace");
                            REQUIRE(full(s, 0.5, cf, os, xa, ya, outs, xa, need) == BHW_ERR_BADARG, "workspace on x");
                            REQUIRE(full(s, 0.5, cf, os, xa, ya, nullptr, wa, need) == BHW_ERR_BADARG, "no outputs given");
                            for (uint32_t i = 0; i < kCsdOutputs; ++i) {
                                const void *o2[kCsdOutputs];
                                memcpy(o2, outs, sizeof o2);
                                const bool asked = (cf & kBits[i]) != 0;
                                o2[i] = nullptr;
                                REQUIRE(full(s, 0.5, cf, os, xa, ya, o2, wa, need) == (asked ? BHW_ERR_BADARG : BHW_OK), "a NULL output %u", i);
                                o2[i] = (const void *)(oa + i * gap + (kWidth[i] == 2 ? 4 : 2));
                                REQUIRE(full(s, 0.5, cf, os, xa, ya, o2, wa, need) == (asked ? BHW_ERR_BADARG : BHW_OK), "a misaligned output %u", i);
                                o2[i] = (const void *)ya;
                                REQUIRE(full(s, 0.5, cf, os, xa, ya, o2, wa, need) == (asked ? BHW_ERR_BADARG : BHW_OK), "output %u on y", i);
                                o2[i] = (const void *)(wa + need - 4);
                                REQUIRE(full(s, 0.5, cf, os, xa, ya, o2, wa, need) == (asked ? BHW_ERR_BADARG : BHW_OK), "output %u on the workspace's end", i);
                                o2[i] = (const void *)(wa + need);
                                REQUIRE(full(s, 0.5, cf, os, xa, ya, o2, wa, need) == BHW_OK, "output %u behind the workspace", i);
                                o2[i] = outs[(i + 1) % kCsdOutputs];
                                REQUIRE(full(s, 0.5, cf, os, xa, ya, o2, wa, need) == (asked && (cf & kBits[(i + 1) % kCsdOutputs]) ? BHW_ERR_BADARG : BHW_OK), "two outputs on each other");
                            }
                            REQUIRE(full(s, 0.5, cf | 4u, os, xa, ya, outs, wa, need) == BHW_ERR_BADARG, "unknown csd_flags");
                            REQUIRE(full(s, 0.5, cf & ~kCsdOutputMask, os, xa, ya, outs, wa, need) == BHW_ERR_BADARG, "an empty mask");
                            REQUIRE(full(s, INFINITY, cf, os, xa, ya, outs, wa, need) == BHW_ERR_BADARG && full(s, NAN, cf, os, xa, ya, outs, wa, need) == BHW_ERR_BADARG, "scale");
                            REQUIRE(full(s, 0.5, cf, K - 1, xa, ya, outs, wa, need) == BHW_ERR_BADARG, "short o_stride");
                            REQUIRE(bhwp_csd_fft_checks(&p, L, &s, flags | 2u, 0.5, cf, os, nullptr, nullptr, nullptr, nullptr, 0, false) == BHW_ERR_BADARG, "flags");
                            bhw_stft bad = s;
                            bad.y_stride = n + 2;
                            REQUIRE(full(bad, 0.5, cf, os, xa, ya, outs, wa, need) == BHW_ERR_BADARG, "y_stride");
                            bad = s;
                            bad.y_batch_stride = F * (n + 2);
                            REQUIRE(full(bad, 0.5, cf, os, xa, ya, outs, wa, need) == BHW_ERR_BADARG, "y_batch_stride");
                            bad = s;
                            bad.channels = 2;
                            REQUIRE(full(bad, 0.5, cf, os, xa, ya, outs, wa, need) == BHW_ERR_UNSUPPORTED && strstr(bhw_last_error(), "bhw_stft_cfft_f32_"), "channels: %s", bhw_last_error());
                            bad = s;
                            bad.frames = 0;
                            REQUIRE(bhwp_csd_fft_checks(&p, L, &bad, flags, 0.5, cf, os, nullptr, nullptr, nullptr, nullptr, 0) == BHW_OK, "frames 0");
                            REQUIRE(bhwp_csd_fft_workspace_bytes(&bad) == 0, "frames 0 needs no workspace");
                            REQUIRE(bhwp_describe_csd_fft(&p, nullptr, L, &bad, flags, cf, buf, sizeof buf) == BHW_OK, "describe frames 0");
                            const BhwCsdFftPlan z = bhwp_csd_fft_plan(&p, L, &bad, flags, cf, os, false);
                            REQUIRE(z.fft.rows == 0 && z.fft.groups == 0 && z.fft.grid == 0 && z.runs == 0 && z.ws_bytes == 0 && z.out_grid == 0, "the plan of nothing");
                            const BhwCsdFftPlan cp = bhwp_csd_fft_plan(&p, L, &s, flags, cf, os, (B + F) % 2 == 0);
                            const BhwStftFftPlan fw = bhwp_stft_fft_plan(&p, L, &s, flags, (B + F) % 2 == 0);
                            REQUIRE(cp.fft.radix4 == fw.radix4 && cp.fft.radix2 == fw.radix2 && cp.fft.rows == fw.rows && cp.fft.m == fw.m &&
                                    cp.fft.x_stride == fw.x_stride && cp.fft.route == fw.route && cp.fft.detrend == fw.detrend, "the forward plan's schedule");
                            if (n <= 1024) REQUIRE(cp.fft.lpf == fw.lpf && cp.fft.fy == fw.fy && cp.fft.cpl == fw.cpl && cp.fft.lds_bytes == fw.lds_bytes, "the forward plan's lanes and LDS");
                            else           REQUIRE(cp.fft.lpf == 128 && cp.fft.fy == 2 && cp.fft.cpl == 16 && cp.fft.lds_bytes == 2u * 2u * 1024u * 8u + 1024u * 8u + 8u, "n_fft 2048 on 128 lanes a row");
                            REQUIRE(cp.ws_bytes == need && cp.o_stride == (os ? os : K) && cp.flags == cf, "workspace, o_stride, flags");
                            REQUIRE(bhwp_describe_csd_fft(&p, nullptr, L, &s, flags, cf, buf, sizeof buf) == BHW_OK && strlen(buf) > 80 && strlen(buf) < sizeof buf - 1, "describe");
                            REQUIRE(strstr(buf, "accumulator") && strstr(buf, "chunk 16 frames") && strstr(buf, "workspace") && strstr(buf, "frame pair"), "the line's own fields in %s", buf);
                            if (hop == 7 && (L == n || F == 531) && (n <= 512 || F <= 65)) {
                                replay_call(cp, s, 1.0 / (3.7 * (double)F));
                                ++replays;
                            }
                        }
    }
    {   // more runs than workgroups, 513 blocks through the join: 16 / 16 / 2, one pair of 131 142 frames
        bhw_stft s = desc_of(1, 262298, 131142, 2, 16, 0, 0, 0);
        REQUIRE(bhwp_csd_fft_checks(&p, 16, &s, 0, 1.0, kCsdOutputMask | BHW_CSD_ONESIDED, 0, nullptr, nullptr, nullptr, nullptr, 0, false) == BHW_OK, "the long case: %s", bhw_last_error());
        const BhwCsdFftPlan cp = bhwp_csd_fft_plan(&p, 16, &s, 0, kCsdOutputMask | BHW_CSD_ONESIDED, 0, false);
        REQUIRE(cp.runs > kFftMaxGrid && cp.fft.grid == kFftMaxGrid && cp.blocks == 513, "runs %" PRIu64 " blocks %" PRIu64, cp.runs, cp.blocks);
        replay_call(cp, s, 0.25);
        ++replays;
        // and a signal of 2^24 samples at 2048 / 512: the plan alone
        bhw_stft t2 = desc_of(1, 1ull << 24, 32765, 512, 2048, 0, 0, 0);
        const BhwCsdFftPlan w2 = bhwp_csd_fft_plan(&p, 2048, &t2, BHW_WELCH_DETREND_CONSTANT, BHW_CSD_PXY, 0, true);
        REQUIRE(w2.runs == 2048 && w2.fft.grid == 2048 && w2.chunks == 2048 && w2.blocks == 128 && w2.acc == 5 && w2.gpr == 16 && w2.pairs == 1, "T2's plan");
    }
    REQUIRE(bhwp_csd_fft_checks(&p, 16, nullptr, 0, 1.0, BHW_CSD_PXY, 0, nullptr, nullptr, nullptr, nullptr, 0, false) == BHW_ERR_BADARG, "NULL descriptor");
    REQUIRE(bhwp_csd_fft_workspace_bytes(nullptr) == 0, "NULL descriptor needs nothing");
    {   // what the params alone are refused for comes first, with the fused Welch PSD's code and words, whatever the descriptor holds:
        // a NULL one is never looked at, and the refusals this call renames (channels, n_fft) do not take the words over
        bhw_params bad[3] = {p, p, p};
        bad[0].sin_type = BHW_SIN_TAYLOR;
        bad[1].model = BHW_MODEL_DDS48;
        bad[2].phi_width = 8;                                                                 // L = 400 is no length of this window
        bhw_stft good = desc_of(2, 16000, 98, 160, 512, 0, 0, 0);
        bhw_stft big = desc_of(2, 160000, 9, 160, 4096, 0, 0, 0), mixed = desc_of(2, 16000, 98, 160, 500, 0, 0, 0), iq = good;
        iq.channels = 2;
        const bhw_stft *descs[5] = {&good, &big, &mixed, &iq, nullptr};
        int unsupported = 0;
        for (const bhw_params &q : bad) {
            const int code = bhwp_welch_fft_checks(&q, 400, &good, 0, 1.0, 1, 0, nullptr, nullptr, nullptr, 0, false);
            char want[512];
            snprintf(want, sizeof want, "%s", bhw_last_error());
            REQUIRE(code == BHW_ERR_UNSUPPORTED || code == BHW_ERR_BADARG, "the params are refused: %d", code);
            unsupported += code == BHW_ERR_UNSUPPORTED;
            for (const bhw_stft *d : descs)
                for (int pointers = 0; pointers < 2; ++pointers) {
                    const int rc = bhwp_csd_fft_checks(&q, 400, d, 0, 1.0, kCsdOutputMask, 0, (const void *)xa, (const void *)ya, outs, (const void *)wa,
                                                       1ull << 40, pointers != 0);
                    REQUIRE(rc == code && strcmp(bhw_last_error(), want) == 0, "refused params: rc %d (%d), '%s' for '%s'", rc, code, bhw_last_error(), want);
                }
        }
        REQUIRE(unsupported >= 1, "an unsupported source or model among them");
        REQUIRE(bhwp_csd_fft_checks(&p, 400, nullptr, 0, 1.0, kCsdOutputMask, 0, nullptr, nullptr, nullptr, nullptr, 0, false) == BHW_ERR_BADARG &&
                strcmp(bhw_last_error(), "stft descriptor is NULL") == 0, "a NULL descriptor with good params: %s", bhw_last_error());
    }
    for (uint64_t n : {8ull, 48ull, 400ull, 1000ull, 4096ull, 8192ull}) {
        bhw_stft s = desc_of(1, 1ull << 33, 2, 1, n, 0, 0, 0);
        REQUIRE(bhwp_csd_fft_checks(&p, 1, &s, 0, 1.0, BHW_CSD_PXY, 0, nullptr, nullptr, nullptr, nullptr, 0, false) == BHW_ERR_UNSUPPORTED, "n_fft %" PRIu64, n);
        if (n == 4096) REQUIRE(strstr(bhw_last_error(), "bhw_stft_fft_f32_* + bhw_welch_csd_f32"), "4096 names the two-call route: %s", bhw_last_error());
        if (n == 400 || n == 1000 || n == 48) REQUIRE(strstr(bhw_last_error(), "bhw_stft_mfft_f32_* + bhw_welch_csd_f32"), "mixed radix names its route: %s", bhw_last_error());
    }
    REQUIRE(replays >= 60, "replays %ld", replays);
    printf("ok %ld checks, %ld call replays\n", g_checks, replays);
    return 0;
}
