// san_csd.cpp -- the planner's part of the Welch cross spectra (bhw_plan.cpp: bhwp_csd_checks / bhwp_csd_plan / bhwp_describe_csd) swept
// under AddressSanitizer + UBSan over B, F (1, 2, BLOCK - 1, BLOCK, BLOCK + 1, many), K, strides, every single-output mask, mixed masks,
// the full mask and the broadcast flag.  Besides "no report", it replays on the host the ownership of k_welch_csd / k_welch_csd_join
// (bhw_welch_csd.hip):
//   - the passes of four waves through LDS: every (b, f, k) of X and of Y loaded once (under broadcast X's (f, k) once per signal of Y),
//     every load -- clamped past the block's end, idle lanes at the last bin -- inside its operand;
//   - every (b, f, k) enters each of the plan's chains once, in ascending f within its block, added by the wave that owns the chain from
//     the LDS row the loading wave wrote;
//   - the block sums at distinct workspace slots inside the workspace, joined per chain in ascending block order;
//   - every requested output element written once, inside its row; the plan's LDS within 64 KiB and two workgroups within a CU's 160 KiB.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "bhw_plan.h"

static long g_checks = 0;
#define REQUIRE(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static bhw_csd csd_of(uint64_t B, uint64_t F, uint64_t K, uint64_t n_fft, uint32_t flags, uint64_t xs, uint64_t xbs, uint64_t ys, uint64_t ybs,
                      uint64_t os)
{
    bhw_csd d;
    memset(&d, 0, sizeof d);
    d.struct_size = sizeof d;
    d.flags = flags;
    d.batch = B;
    d.frames = F;
    d.bins = K;
    d.n_fft = n_fft;
    d.x_stride = xs;
    d.x_batch_stride = xbs;
    d.y_stride = ys;
    d.y_batch_stride = ybs;
    d.o_stride = os;
    d.scale = 0.25;
    return d;
}

// k_welch_csd over its grid, then k_welch_csd_join
static void replay_csd(const BhwCsdPlan &pl, const bhw_csd &d)
{
    const uint64_t B = d.batch, F = d.frames, K = d.bins, CH = pl.chains;
    const bool bcast = (d.flags & BHW_CSD_BROADCAST_X) != 0;
    const uint64_t XB = bcast ? 1 : B;
    std::vector<int> xloads(XB * F * K, 0), yloads(B * F * K, 0), adds(B * F * K * CH, 0), slots(B * pl.blocks * CH * K, 0), outs(B * K, 0);
    REQUIRE(pl.blocks == (F + BHW_WELCH_BLOCK - 1) / BHW_WELCH_BLOCK && pl.grid == B * pl.blocks * pl.tiles, "plan");
    REQUIRE((pl.blocks == 1) == (pl.ws_bytes == 0) && (pl.blocks == 1 || pl.ws_bytes == B * pl.blocks * K * CH * 8), "workspace %" PRIu64, pl.ws_bytes);
    REQUIRE(CH == ((d.flags & kCsdOutputMask) == BHW_CSD_PXY ? 2u : 4u) && CH <= kPsdWaves, "chains %" PRIu64, CH);
    const uint32_t U = pl.unroll, pass = kPsdWaves * U;
    REQUIRE(U >= 1 && pl.lds_bytes == pass * kPsdLanes * CH * 8 && pl.lds_bytes == kCsdPassBytes, "LDS %u", pl.lds_bytes);
    REQUIRE(pl.lds_bytes <= 64u * 1024u && 2u * pl.lds_bytes <= 160u * 1024u, "LDS %u", pl.lds_bytes);
    REQUIRE(bcast ? pl.x_bstride == 0 : pl.x_bstride >= (F - 1) * pl.x_stride + K, "x_bstride");
    const uint64_t xext = (XB - 1) * pl.x_bstride + (F - 1) * pl.x_stride + K;
    const uint64_t yext = (B - 1) * pl.y_bstride + (F - 1) * pl.y_stride + K;
    std::vector<uint64_t> row_frame(pass);
    std::vector<int> row_written(pass);
    for (uint64_t unit = 0; unit < pl.grid; ++unit)
        for (uint32_t lane = 0; lane < kPsdLanes; ++lane) {
            const uint64_t tile = unit % pl.tiles, rest = unit / pl.tiles, blk = rest % pl.blocks, b = rest / pl.blocks;
            const uint64_t k = tile * kPsdLanes + lane;
            const bool active = k < K;
            const uint64_t kk = active ? k : K - 1;                                     // an idle lane loads the last bin
            REQUIRE(b < B, "unit %" PRIu64, unit);
            const uint64_t f0 = blk * BHW_WELCH_BLOCK, f1 = f0 + BHW_WELCH_BLOCK < F ? f0 + BHW_WELCH_BLOCK : F;
            REQUIRE(f0 < f1 && f1 - f0 <= BHW_WELCH_BLOCK, "block %" PRIu64, blk);
            std::vector<int64_t> last(CH, -1);
            for (uint64_t p0 = f0; p0 < f1; p0 += pass) {
                // the loads of the pass: wave w, slot u -> LDS row w * U + u of every chain holds the terms of frame p0 + row
                for (uint32_t i = 0; i < pass; ++i) row_written[i] = 0;
                for (uint32_t wave = 0; wave < kPsdWaves; ++wave)
                    for (uint32_t u = 0; u < U; ++u) {
                        const uint64_t fr = p0 + wave * U + u, fc = fr < f1 ? fr : f1 - 1;
                        const uint64_t xi = b * pl.x_bstride + fc * pl.x_stride + kk, yi = b * pl.y_bstride + fc * pl.y_stride + kk;
                        REQUIRE(xi < xext && yi < yext, "X index %" PRIu64 " Y index %" PRIu64, xi, yi);
                        if (active && fr < f1) {
                            if (!bcast || b == 0) ++xloads[((bcast ? 0 : b) * F + fr) * K + k];
                            ++yloads[(b * F + fr) * K + k];
                        }
                        const uint32_t row = wave * U + u;
                        REQUIRE(row < pass, "LDS row %u", row);
                        row_frame[row] = fr;
                        ++row_written[row];
                    }
                for (uint32_t i = 0; i < pass; ++i) REQUIRE(row_written[i] == 1, "LDS row %u written %d times", i, row_written[i]);
                // wave c < CH adds rows 0 .. n - 1 of chain c in ascending order
                const uint32_t n = f1 - p0 < pass ? (uint32_t)(f1 - p0) : pass;
                for (uint32_t wave = 0; wave < kPsdWaves; ++wave) {
                    if (wave >= CH) continue;
                    for (uint32_t i = 0; i < n; ++i) {
                        const uint64_t f = row_frame[i];
                        REQUIRE(f == p0 + i && f < f1 && (int64_t)f > last[wave], "chain %u frame order: row %u holds %" PRIu64, wave, i, f);
                        last[wave] = (int64_t)f;
                        if (active) ++adds[((b * F + f) * K + k) * CH + wave];
                    }
                }
            }
            if (!active) continue;
            if (pl.blocks > 1) {
                for (uint64_t c = 0; c < CH; ++c) {
                    const uint64_t wi = ((b * pl.blocks + blk) * CH + c) * K + k;
                    REQUIRE((wi + 1) * 8 <= pl.ws_bytes, "workspace slot %" PRIu64, wi);
                    ++slots[wi];
                }
            } else {
                REQUIRE(b * pl.o_stride + k < (B - 1) * pl.o_stride + K, "output index");
                ++outs[b * K + k];
            }
        }
    if (pl.blocks > 1) {
        REQUIRE(pl.join_grid * 256u >= B * K && (pl.join_grid - 1) * 256u < B * K, "join grid");
        for (uint64_t i = 0; i < pl.join_grid * 256u; ++i) {
            if (i >= B * K) continue;
            const uint64_t b = i / K, k = i - b * K;
            for (uint64_t c = 0; c < CH; ++c) {
                uint64_t prev = 0;
                for (uint64_t blk = 0; blk < pl.blocks; ++blk) {
                    const uint64_t wi = b * pl.blocks * CH * K + k + (blk * CH + c) * K;          // wp[(blk * CH + c) * bins]
                    REQUIRE(wi == ((b * pl.blocks + blk) * CH + c) * K + k && (blk == 0 || wi > prev) && slots[wi] == 1, "join slot %" PRIu64, wi);
                    prev = wi;
                }
            }
            REQUIRE(b * pl.o_stride + k < (B - 1) * pl.o_stride + K, "output index");
            ++outs[b * K + k];
        }
        for (uint64_t i = 0; i < slots.size(); ++i) REQUIRE(slots[i] == 1, "workspace slot %" PRIu64 " written %d times", i, slots[i]);
    }
    for (uint64_t i = 0; i < xloads.size(); ++i) REQUIRE(xloads[i] == 1, "X element %" PRIu64 " loaded %d times", i, xloads[i]);
    for (uint64_t i = 0; i < yloads.size(); ++i) REQUIRE(yloads[i] == 1, "Y element %" PRIu64 " loaded %d times", i, yloads[i]);
    for (uint64_t i = 0; i < adds.size(); ++i) REQUIRE(adds[i] == 1, "term %" PRIu64 " added %d times", i, adds[i]);
    for (uint64_t i = 0; i < outs.size(); ++i) REQUIRE(outs[i] == 1, "output element %" PRIu64 " written %d times", i, outs[i]);
}

int main()
{
    char buf[900];
    long replays = 0;
    const unsigned long long BL = BHW_WELCH_BLOCK;
    REQUIRE(BL == 256 && sizeof(bhw_csd) == 96, "BHW_WELCH_BLOCK %llu, sizeof(bhw_csd) %zu", BL, sizeof(bhw_csd));
    const uint32_t masks[] = {BHW_CSD_PXY, BHW_CSD_PXX, BHW_CSD_PYY, BHW_CSD_COHERENCE, BHW_CSD_H1, BHW_CSD_PXY | BHW_CSD_COHERENCE,
                              BHW_CSD_PXX | BHW_CSD_PYY, kCsdOutputMask};
    const uint64_t Xa = 0x10000000ull, Ya = 0x100000000000ull, Wa = 0x200000000000ull;
    const void *outs[kCsdOutputs];
    for (uint32_t i = 0; i < kCsdOutputs; ++i) outs[i] = (const void *)(0x300000000000ull + i * 0x10000000000ull);
    for (uint64_t B : {1ull, 3ull, 64ull})
        for (uint64_t F : {1ull, 2ull, BL - 1, BL, BL + 1, 3 * BL + 7})
            for (uint64_t n_fft : {1ull, 64ull, 65ull, 512ull})
                for (uint32_t onesided = 0; onesided <= 1; ++onesided)
                    for (int strided = 0; strided <= 1; ++strided)
                        for (uint32_t bcast = 0; bcast <= 1; ++bcast)
                            for (uint32_t mask : masks) {
                                const uint64_t K = onesided ? n_fft / 2 + 1 : n_fft;
                                const uint64_t xs = strided ? K + 1 : 0, xbs = strided && !bcast ? (F - 1) * (K + 1) + K + 7 : 0;
                                const uint64_t ys = strided ? K + 3 : 0, ybs = strided ? (F - 1) * (K + 3) + K + 5 : 0, os = strided ? K + 2 : 0;
                                const uint32_t flags = mask | (onesided ? BHW_CSD_ONESIDED : 0u) | (bcast ? BHW_CSD_BROADCAST_X : 0u);
                                bhw_csd d = csd_of(B, F, K, n_fft, flags, xs, xbs, ys, ybs, os);
                                int rc = bhwp_csd_checks(&d, nullptr, nullptr, nullptr, nullptr, 0, false);
                                REQUIRE(rc == BHW_OK, "csd checks rc %d", rc);
                                const BhwCsdPlan pl = bhwp_csd_plan(&d);
                                REQUIRE(bhw_welch_csd_workspace_bytes(&d) == pl.ws_bytes, "workspace bytes");
                                rc = bhwp_csd_checks(&d, (const void *)Xa, (const void *)Ya, outs, (const void *)Wa, pl.ws_bytes);
                                REQUIRE(rc == BHW_OK, "csd pointer checks rc %d", rc);
                                rc = bhwp_csd_checks(&d, (const void *)Xa, (const void *)Xa, outs, (const void *)Wa, pl.ws_bytes);
                                REQUIRE(rc == BHW_OK, "X and Y may coincide: rc %d", rc);
                                if (pl.ws_bytes) {
                                    REQUIRE(bhwp_csd_checks(&d, (const void *)Xa, (const void *)Ya, outs, (const void *)Wa, pl.ws_bytes - 1) == BHW_ERR_WORKSPACE, "short");
                                    REQUIRE(bhwp_csd_checks(&d, (const void *)Xa, (const void *)Ya, outs, nullptr, 0) == BHW_ERR_BADARG, "NULL");
                                    REQUIRE(bhwp_csd_checks(&d, (const void *)Xa, (const void *)Ya, outs, (const void *)Ya, pl.ws_bytes) == BHW_ERR_BADARG, "overlap");
                                }
                                // each requested output in turn: NULL, inside Y, on top of the next requested one
                                static const uint32_t bits[kCsdOutputs] = {BHW_CSD_PXY, BHW_CSD_PXX, BHW_CSD_PYY, BHW_CSD_COHERENCE, BHW_CSD_H1};
                                for (uint32_t i = 0; i < kCsdOutputs; ++i) {
                                    const void *alt[kCsdOutputs];
                                    memcpy(alt, outs, sizeof alt);
                                    alt[i] = nullptr;
                                    rc = bhwp_csd_checks(&d, (const void *)Xa, (const void *)Ya, alt, (const void *)Wa, pl.ws_bytes);
                                    REQUIRE(rc == ((mask & bits[i]) ? BHW_ERR_BADARG : BHW_OK), "output %u NULL: rc %d", i, rc);
                                    alt[i] = (const void *)Ya;
                                    rc = bhwp_csd_checks(&d, (const void *)Xa, (const void *)Ya, alt, (const void *)Wa, pl.ws_bytes);
                                    REQUIRE(rc == ((mask & bits[i]) ? BHW_ERR_BADARG : BHW_OK), "output %u in Y: rc %d", i, rc);
                                    for (uint32_t j = 0; j < kCsdOutputs; ++j)
                                        if (j != i && (mask & bits[i]) && (mask & bits[j])) {
                                            alt[i] = outs[j];
                                            REQUIRE(bhwp_csd_checks(&d, (const void *)Xa, (const void *)Ya, alt, (const void *)Wa, pl.ws_bytes) == BHW_ERR_BADARG,
                                                    "outputs %u and %u coincide", i, j);
                                        }
                                }
                                REQUIRE(bhw_describe_csd(&d, buf, sizeof buf) == BHW_OK && strstr(buf, pl.chains == 2 ? "k_welch_csd<2," : "k_welch_csd<4,"), "describe");
                                if (bcast) {
                                    bhw_csd bad = d;
                                    bad.x_batch_stride = F * (xs ? xs : K);
                                    REQUIRE(bhwp_csd_checks(&bad, nullptr, nullptr, nullptr, nullptr, 0, false) == BHW_ERR_BADARG, "broadcast with a batch stride");
                                }
                                bhw_csd bad = d;
                                bad.flags &= ~kCsdOutputMask;
                                REQUIRE(bhwp_csd_checks(&bad, nullptr, nullptr, nullptr, nullptr, 0, false) == BHW_ERR_BADARG, "empty mask");
                                bad = d;
                                bad.flags |= 0x200u;
                                REQUIRE(bhwp_csd_checks(&bad, nullptr, nullptr, nullptr, nullptr, 0, false) == BHW_ERR_BADARG, "unknown flag");
                                if (B * F * K <= 150000) {
                                    replay_csd(pl, d);
                                    ++replays;
                                }
                            }
    REQUIRE(replays > 1000, "replays %ld", replays);
    printf("ok %ld checks, %ld cross-spectra replays\n", g_checks, replays);
    return 0;
}
