// san_resident.cpp -- the planner's part of the resident tables (bhw_plan.cpp: creation checks, key match, layout, format candidates,
// the kernel of every piece, bhw_table_describe's text) swept under AddressSanitizer + UBSan over models, rules, widths, precisions,
// table formats and call shapes.  Besides "no report", it checks that the size a table is held in is the whole-period workspace rule.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bhw_plan.h"

extern "C" {
uint64_t bhw_workspace_bytes_ex(const bhw_params *p, uint64_t n0, uint64_t count, const bhw_exec *ex);
int bhw_dbg_table_format_verdict(const bhw_params *p, uint32_t dlog, int set);
int bhw_dbg_table_key_matches(const bhw_params *p_table, const bhw_params *p_call);
int bhw_dbg_describe_from_table(const bhw_params *p_table, uint32_t table_format, const bhw_params *p_call, uint64_t n0, uint64_t count,
                                char *buf, uint64_t len);
}

static long g_checks = 0;
#define REQUIRE(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

int main()
{
    static const uint32_t kWins[6] = {BHW_WIN_HAMMING, BHW_WIN_HANN, BHW_WIN_BH3, BHW_WIN_BH4, BHW_WIN_BH5, BHW_WIN_BH7};
    char buf[384], tiny[1], small[24];
    for (uint32_t model = 0; model <= BHW_MODEL_SCALED; ++model)
        for (uint32_t pw = 3; pw <= 31; ++pw)
            for (uint32_t W = 7; W <= 33; W += (W < 12 || W > 28) ? 1 : 4)
                for (uint32_t prec = (model == BHW_MODEL_VHDL ? 0 : 1); prec <= (model == BHW_MODEL_VHDL ? 8u : 1u); prec += 2)
                    for (uint32_t sin_type = 0; sin_type <= 2; sin_type += 2)
                        for (uint32_t fmt = 0; fmt <= 6; ++fmt) {
                            bhw_params p;
                            memset(&p, 0, sizeof p);
                            bhw_params_init(&p, BHW_WIN_BH7, pw, W);
                            p.model = model;
                            p.precision = prec;
                            p.sin_type = sin_type;
                            const int rc = bhwp_table_create_checks(&p, fmt);
                            REQUIRE(rc == BHW_OK || rc == BHW_ERR_BADARG || rc == BHW_ERR_UNSUPPORTED, "rc %d", rc);
                            if (sin_type != BHW_SIN_CORDIC || model > BHW_MODEL_VHDL) REQUIRE(rc != BHW_OK, "no table of this source / model");
                            if (rc) continue;
                            BhwCordicCfg c;
                            bool tiled;
                            bhwp_resident_layout(&p, c, &tiled);
                            REQUIRE(c.tab_split == 0u || (tiled && c.z_shr == 0), "split layout only for tiled tables at z_shr 0");
                            uint32_t cand[kMaxFormats];
                            const int n = bhwp_table_format_candidates(c, tiled, fmt, cand);
                            REQUIRE(n >= 1 && cand[n - 1] == 0u, "plain is the last candidate");
                            // every candidate exact: the table is the first one, and its size is the whole-period workspace rule
                            for (int i = 0; i < n; ++i) if (cand[i]) bhw_dbg_table_format_verdict(&p, cand[i], 1);
                            bhw_exec ex;
                            memset(&ex, 0, sizeof ex);
                            ex.struct_size = sizeof ex;
                            ex.algo = BHW_ALGO_TABLE;
                            ex.table_format = fmt;
                            const uint64_t N = 1ull << pw;
                            REQUIRE(bhw_workspace_bytes_ex(&p, 0, N, &ex) == bhwp_table_layout(bhwp_table_entries(c), cand[0]).bytes, "bytes");
                            for (int i = 0; i < n; ++i) if (cand[i]) bhw_dbg_table_format_verdict(&p, cand[i], 3);   // (forget: unknown again)
                            for (uint32_t win : kWins)
                                for (uint32_t combine = 0; combine <= 1; ++combine) {
                                    bhw_params q = p;
                                    bhw_params_init(&q, win, pw, W);
                                    q.model = model;
                                    q.precision = prec;
                                    q.combine = combine;
                                    if (bhw_params_validate(&q)) continue;
                                    REQUIRE(bhw_dbg_table_key_matches(&p, &q) == BHW_OK, "ports are free");
                                    const uint64_t shapes[][2] = {{0, N}, {1, 1}, {N - 1, 2}, {5, 3 * N + 7}, {N / 8, N / 4}, {(1ull << 40) + 3, N - 8}, {0, 0}};
                                    for (const auto &s : shapes) {
                                        REQUIRE(bhw_dbg_describe_from_table(&p, fmt, &q, s[0], s[1], buf, sizeof buf) == BHW_OK, "describe");
                                        REQUIRE(strncmp(buf, "resident table[", 15) == 0, "%s", buf);
                                        const bool whole = s[1] >= (N - s[0] % N) % N + N;
                                        if (s[1] && !whole && !strstr(buf, "image subset")) REQUIRE(strstr(buf, "k_range_combine<") != nullptr, "%s", buf);
                                        REQUIRE(bhw_dbg_describe_from_table(&p, fmt, &q, s[0], s[1], tiny, sizeof tiny) == BHW_OK && tiny[0] == 0, "truncated");
                                        REQUIRE(bhw_dbg_describe_from_table(&p, fmt, &q, s[0], s[1], small, sizeof small) == BHW_OK, "truncated");
                                    }
                                    bhw_params r = q;
                                    r.dat_width = W == 32 ? 31 : W + 1;
                                    if (!bhw_params_validate(&r)) REQUIRE(bhw_dbg_table_key_matches(&p, &r) == BHW_ERR_BADARG && strstr(bhw_last_error(), "dat_width"), "dat_width");
                                    r = q;
                                    r.phi_width = pw == 4 ? 5 : pw - 1;
                                    if (!bhw_params_validate(&r)) REQUIRE(bhw_dbg_table_key_matches(&p, &r) == BHW_ERR_BADARG && strstr(bhw_last_error(), "phi_width"), "phi_width");
                                    if (model == BHW_MODEL_VHDL) {
                                        r = q;
                                        r.precision = prec == 7 ? 1 : prec + 1;
                                        REQUIRE(bhw_dbg_table_key_matches(&p, &r) == BHW_ERR_BADARG && strstr(bhw_last_error(), "precision"), "precision");
                                    }
                                }
                        }
    printf("ok %ld\n", g_checks);
    return 0;
}
