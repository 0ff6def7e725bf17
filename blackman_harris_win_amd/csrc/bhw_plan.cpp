// bhw_plan.cpp -- the HIP-free half of the host side (see bhw_plan.h): validation, resolution of (model, widths) into kernel
// constants, strategy / format / shape decisions, ownership segments, scratch sizing, bhw_describe_plan.  Plain C++: no hip*
// include, no device state; swept under AddressSanitizer + UBSan by tests/test_sanitizers.py.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "bhw_plan.h"
#include "bhw_tables.inc"

namespace {

thread_local std::string g_last_error;

// Built-in float weights: hls/windows/win_function.cpp:173-174,191-192,206-208,253-256,306-310,341-347.
const double kHamming[2] = {0.5434783, 1 - 0.5434783};
const double kHann[2] = {0.5, 0.5};
const double kBh3[3] = {0.21, 0.25, 0.04};
const double kBh4[4] = {0.35875, 0.48829, 0.14128, 0.01168};
const double kBh5[5] = {0.3232153788877343, 0.4714921439576260, 0.1755341299601972, 0.0284969901061499,
                        0.0012613570882927};
const double kBh7[7] = {0.271220360585039, 0.433444612327442, 0.218004122892930, 0.065785343295606,
                        0.010761867305342, 0.000770012710581, 0.000013680883060};

const uint32_t kSelSize[25] = {15, 15, 15, 18, 21, 22, 23, 26, 30, 31, 32, 33,           // src/cordic_dds_scaled.vhd:102-107
                               38, 38, 38, 42, 42, 45, 47, 47, 47, 48, 48, 48, 48};

std::mutex g_fmt_mu;
std::map<uint64_t, int> g_fmt_verdict;

uint64_t fmt_key(const bhw_params *p, uint32_t dlog)
{
    return ((uint64_t)p->model << 40) | ((uint64_t)p->phi_width << 32) | ((uint64_t)p->dat_width << 24) |
           ((uint64_t)(p->model == BHW_MODEL_VHDL ? p->precision : 0u) << 16) | dlog;
}

uint64_t align256(uint64_t v) { return (v + 255ull) & ~255ull; }

// Whole periods up to this length go through the fused kernel under AUTO: one launch of 5/8 .. 9/8 chains per coefficient beats
// two dependent launches around a table of 1/4 chain per coefficient while the call is launch- and latency-bound.  Measured per
// call (profiles/r02_small_windows.json): BH-4/24-bit fused 8.0 / 12.1 / 17.0 us at 2^20 / 2^21 / 2^22 against 11.7 / 14.6 /
// 19.9 us for the table strategy; BH-7/32-bit 9.0 (2^16) / 13.3 / 21.8 / 33.5 us against 11.9 / 11.9 / 16.8 / 27.5 us.
uint32_t fused_max_pw(uint32_t n_terms) { return n_terms <= 5 ? 22u : 19u; }

uint32_t inv_mod_pow2(uint32_t a, uint32_t log2m)
{
    uint32_t x = a;                      // Newton iteration: x <- x (2 - a x), doubles the correct bits
    for (int i = 0; i < 6; ++i) x *= 2u - a * x;
    return log2m >= 32 ? x : (x & ((1u << log2m) - 1u));
}

} // namespace

int bhwp_fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

int bhwp_terms_of(uint32_t win_type)
{
    switch (win_type) {
    case BHW_WIN_HAMMING: case BHW_WIN_HANN: return 2;
    case BHW_WIN_BH3: return 3;
    case BHW_WIN_BH4: return 4;
    case BHW_WIN_BH5: return 5;
    case BHW_WIN_BH7: return 7;
    default: return 0;
    }
}

int bhwp_validate(const bhw_params *p, bool sincos_only)
{
    if (!p) return bhwp_fail(BHW_ERR_BADARG, "params is NULL");
    if (p->struct_size != sizeof(bhw_params))
        return bhwp_fail(BHW_ERR_BADARG, "struct_size %u != %zu", p->struct_size, sizeof(bhw_params));
    if (p->model > BHW_MODEL_SCALED) return bhwp_fail(BHW_ERR_BADARG, "model %u", p->model);
    if (p->model > BHW_MODEL_VHDL && !sincos_only)
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "cordic_dds48 / cordic_dds_scaled feed no window entity: bhw_sincos_* only");
    if (p->combine > BHW_COMBINE_VHDL) return bhwp_fail(BHW_ERR_BADARG, "combine %u", p->combine);
    if (p->sin_type > BHW_SIN_TAYLOR_ALL) return bhwp_fail(BHW_ERR_BADARG, "sin_type %u", p->sin_type);
    const uint32_t K = p->n_terms;
    if (!(K == 2 || K == 3 || K == 4 || K == 5 || K == 7)) return bhwp_fail(BHW_ERR_BADARG, "n_terms %u (2,3,4,5,7)", K);
    const uint32_t PW = p->phi_width, W = p->dat_width;
    if (PW < 4 || PW > 30) return bhwp_fail(BHW_ERR_BADARG, "phi_width %u outside 4..30", PW);
    if (W < 8 || W > 32) return bhwp_fail(BHW_ERR_BADARG, "dat_width %u outside 8..32", W);
    if (p->sin_type != BHW_SIN_CORDIC) {
        // win_selector wires the Taylor source only to HAMMING and BH3TERM: src/win_selector.vhd:93-135
        if (K > 3 && p->sin_type == BHW_SIN_TAYLOR)
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "Taylor source exists only for 2- and 3-term windows (BHW_SIN_TAYLOR_ALL is the extension)");
        const uint32_t L = p->lut_size;
        if (L < 1 || L > 16) return bhwp_fail(BHW_ERR_BADARG, "lut_size %u outside 1..16", L);
        // generators in use: PHASE_WIDTH - v, v = 0 .. vmax  (bh_win_3term.vhd:221-226; k = 4 needs v = 2)
        const uint32_t vmax = K > 4 ? 2u : K > 2 ? 1u : 0u;
        if (PW < 3 + vmax) return bhwp_fail(BHW_ERR_UNSUPPORTED, "phi_width %u too short for the PHASE_WIDTH-%u generator", PW, vmax);
        const uint32_t pw_min = PW - vmax;
        for (uint32_t pw = pw_min; pw <= PW; ++pw) {
            const int d = (int)pw - (int)L;
            if (d > 2) {
                if (d - 3 > 15) return bhwp_fail(BHW_ERR_UNSUPPORTED, "Taylor STAGE %d > 15 (tay1_order cnt_exp is 16 bits)", d - 3);
                if (W < 19 && 19 + L + W > 48) return bhwp_fail(BHW_ERR_UNSUPPORTED, "Taylor narrow path: 19+L+W > 48 DSP bits");
                if (W > 18 && 19 + L + W > 62) return bhwp_fail(BHW_ERR_UNSUPPORTED, "Taylor wide path: 19+L+W > 62 product bits");
            }
        }
        return BHW_OK;
    }
    if (p->model == BHW_MODEL_HLS && PW > W + 2)
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "HLS model is ill-defined for phi_width > dat_width + 2 (init_t truncation)");
    if (p->model == BHW_MODEL_VHDL && (p->precision < 1 || p->precision > 7))
        return bhwp_fail(BHW_ERR_BADARG, "precision %u outside 1..7", p->precision);
    return BHW_OK;
}

int bhwp_validate_atan2(const bhw_atan2_params *p)
{
    if (!p) return bhwp_fail(BHW_ERR_BADARG, "params is NULL");
    if (p->struct_size != sizeof(bhw_atan2_params))
        return bhwp_fail(BHW_ERR_BADARG, "struct_size %u != %zu", p->struct_size, sizeof(bhw_atan2_params));
    if (p->precision < 1 || p->precision > 7) return bhwp_fail(BHW_ERR_BADARG, "precision %u outside 1..7", p->precision);
    if (p->angle_width < 4 || p->angle_width > 32) return bhwp_fail(BHW_ERR_BADARG, "angle_width %u outside 4..32", p->angle_width);
    if (p->input_width > 32) return bhwp_fail(BHW_ERR_BADARG, "input_width %u > 32", p->input_width);
    if (p->input_width + 1 < p->angle_width)   // VEC_DX(ii) for ii = 0 .. ANGLE_WIDTH-2: src/cordic_atan2.vhd:142-145
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "input_width %u < angle_width-1: the entity indexes input bits 0..ANGLE_WIDTH-2", p->input_width);
    return BHW_OK;
}

// Resolve the CORDIC constants.
void bhwp_resolve_cordic(const bhw_params *p, BhwCordicCfg &c)
{
    memset(&c, 0, sizeof c);
    const uint32_t PW = p->phi_width, W = p->dat_width;
    c.phi_width = PW;
    c.dat_width = W;
    uint32_t n_lut = W - 1;
    switch (p->model) {
    case BHW_MODEL_HLS:  // hls/windows/win_function.cpp:77-96
        for (uint32_t i = 0; i < n_lut; ++i) c.lut[i] = kAtanT4[i] >> (47 - W);
        c.x0 = kGain46 >> (46 - W);
        c.n_iter = W;
        if (PW - 1 < W) { c.z_shr = 0; c.z_shl = W - PW + 2; } else { c.z_shr = PW - W; c.z_shl = 2; }
        c.out_shr = 2;
        c.ones_neg = 0;
        c.wide = (W + 2 > 32);
        break;
    case BHW_MODEL_CPP:  // cpp/cordic_sincos.cpp:15-36
        for (uint32_t i = 0; i < n_lut; ++i) c.lut[i] = kAtanT2[i] >> (47 - W);
        c.x0 = kGain46 >> (46 - W);
        c.n_iter = W;
        if (PW - 1 < W) { c.z_shr = 0; c.z_shl = W - PW + 1; } else { c.z_shr = PW - W; c.z_shl = 1; }
        c.out_shr = 2;
        c.ones_neg = 1;
        c.wide = (W + 2 > 32);
        break;
    default: {           // src/cordic_dds.vhd:97-131,159-166
        const uint32_t P = p->precision, Wi = W + P;
        for (uint32_t i = 0; i < n_lut; ++i) c.lut[i] = kAtanT4[i] >> (49 - Wi);
        c.x0 = kGain47 >> (49 - Wi);
        c.n_iter = W - 1;
        if (PW >= W) { c.z_shr = PW - W; c.z_shl = P; } else { c.z_shr = 0; c.z_shl = W - PW + P; }
        c.out_shr = P;
        c.ones_neg = 0;
        c.wide = (Wi > 32);
        break;
    }
    }
}

void bhwp_resolve_window(const bhw_params *p, BhwWinCfg &w)
{
    memset(&w, 0, sizeof w);
    for (int k = 0; k < 7; ++k) w.aa[k] = p->aa[k];
    w.n_terms = p->n_terms;
    w.combine = p->combine;
}

// cordic_dds48: SIZE = DWPH = 48 (src/cordic_dds48.vhd:143-153); cordic_dds_scaled: SIZE = SEL_SIZE(DATA_WIDTH-8),
// DWPH = max(SIZE, PHASE_WIDTH) (src/cordic_dds_scaled.vhd:109,133-143)
void bhwp_resolve_prerot(const bhw_params *p, BhwPrerotCfg &c)
{
    memset(&c, 0, sizeof c);
    c.phi_width = p->phi_width;
    c.dat_width = p->dat_width;
    c.size = p->model == BHW_MODEL_DDS48 ? 48u : kSelSize[p->dat_width - 8];
    c.dwph = c.size < p->phi_width ? p->phi_width : c.size;
    c.gain = kGain46 >> (48 - c.size);                                          // GAIN48(47 downto 48-SIZE)
    for (uint32_t i = 0; i + 1 < p->dat_width; ++i) c.lut[i] = kAtanT2[i] >> (48 - c.dwph);   // ROM_LUT(ii)(47 downto 48-DWPH)
}

void bhwp_resolve_atan2(const bhw_atan2_params *p, BhwAtan2Cfg &c)
{
    memset(&c, 0, sizeof c);
    c.precision = p->precision;
    c.input_width = p->input_width;
    c.angle_width = p->angle_width;
    const uint32_t B = p->angle_width + p->precision;
    for (uint32_t i = 0; i + 1 < p->angle_width; ++i) c.lut[i] = kAtanT4[i] >> (49 - B);   // src/cordic_atan2.vhd:100-103
}

bool bhwp_has_whole_period(const bhw_params *p, uint64_t n0, uint64_t count)
{
    const uint64_t N = 1ull << p->phi_width;
    return count >= (N - n0 % N) % N + N;
}

int bhwp_apply_checks(uint64_t count, const void *d_x, const void *d_y, uint32_t shift)
{
    if (count && (!d_x || !d_y)) return bhwp_fail(BHW_ERR_BADARG, "d_x / d_y is NULL");
    if (shift > 62) return bhwp_fail(BHW_ERR_BADARG, "shift %u > 62", shift);
    const uintptr_t xa = (uintptr_t)d_x, ya = (uintptr_t)d_y, bytes = (uintptr_t)count * 4u;
    if (count && xa < ya + bytes && ya < xa + bytes)
        return bhwp_fail(BHW_ERR_BADARG, "d_y must not overlap d_x (tile seams recompute a few samples)");
    return BHW_OK;
}

// AUTO: the fused kernel for short whole periods; else build the shared table when it replaces clearly more CORDIC chains
// than it costs; else one chain per harmonic per coefficient.
uint32_t bhwp_pick_algo(const bhw_params *p, const BhwCordicCfg &c, const BhwWinCfg &w, uint64_t n0, uint64_t count, uint32_t requested)
{
    if (p->sin_type != BHW_SIN_CORDIC) return BHW_ALGO_DIRECT;
    const bool fused_ok = bhwk_fold_direct_applicable(c) && bhwp_has_whole_period(p, n0, count);
    if (requested == BHW_ALGO_FUSED) return fused_ok ? BHW_ALGO_FUSED : BHW_ALGO_TABLE;
    if (requested == BHW_ALGO_DIRECT || requested == BHW_ALGO_TABLE) return requested;
    // With dropped phase bits the table has only 2^(W-2) entries and the run-length kernel runs at the store rate: the crossover
    // above was measured at z_shr == 0 only, so windows that kernel takes keep the table strategy.  Where it does not apply
    // (small z_shr: fewer than (K-1) * 16 coefficients per entry; the VHDL sum beyond 28 bits) the table strategy would fall to
    // build + quadrant fold, which the fused kernel beats at these lengths (11.7 against 8.0 us at 2^20, round 2): fused.
    if (fused_ok && p->phi_width <= fused_max_pw(p->n_terms) &&
        (c.z_shr == 0 || p->phi_width < 15 || !bhwk_runlength_applicable(c, w, nullptr)))
        return BHW_ALGO_FUSED;
    const uint64_t chains_direct = count * (p->n_terms - 1);
    return chains_direct >= 2 * bhwp_table_entries(c) ? BHW_ALGO_TABLE : BHW_ALGO_DIRECT;
}

uint32_t bhwp_exec_table_format(const bhw_exec *ex)
{
    return (ex && ex->struct_size >= sizeof(bhw_exec)) ? ex->table_format : (uint32_t)BHW_TABLE_BEST;
}

int bhwp_check_exec(const bhw_exec *ex)
{
    if (!ex) return BHW_OK;
    if (ex->struct_size != sizeof(bhw_exec) && ex->struct_size != 32u)       // 32 = the ABI-1 layout (no table_format)
        return bhwp_fail(BHW_ERR_BADARG, "bhw_exec.struct_size %u", ex->struct_size);
    if (ex->struct_size >= sizeof(bhw_exec) && (ex->table_format > BHW_TABLE_NIBBLE_ESC || ex->reserved != 0))
        return bhwp_fail(BHW_ERR_BADARG, "bhw_exec.table_format %u / reserved %u", ex->table_format, ex->reserved);
    return BHW_OK;
}

// ---- table formats ----------------------------------------------------------------------------------------------------------------

// Packed (delta16) table format applies when the (c, s) drift across a 64-entry block fits int16 with margin:
// 63 * 2 pi * 2^(W-2-PW) + noise < 2^15  <=>  W - PW <= 8  (25.4 k at W - PW = 8).  Amplitude is 2^(W-2) for every model.
bool bhwk_packed_ok(const BhwCordicCfg &c)
{
    if (c.z_shr != 0 || c.phi_width < 8) return false;
    return (int)c.dat_width - (int)c.phi_width <= 8;
}

// Residual format: largest d <= 9 for which the straight line between records 2^d entries apart stays within half an LSB of
// the true curve: (2 pi 2^d / 2^PW)^2 / 8 * 2^(W-2) <= 0.5.  0 = not applicable (d = 6 is left to delta16).
uint32_t bhwk_resid_dlog(const BhwCordicCfg &c)
{
    if (c.z_shr != 0 || c.phi_width < 20 || c.dat_width + c.out_shr > 34 || c.n_iter < 7) return 0;
    const int amp_bits = (int)c.dat_width - 2;                       // |c|, |s| <= 2^(W-2) (+1)
    const int twice_d = 2 * (int)c.phi_width - amp_bits - 4;         // 4.93 * 2^(2d - 2PW + W - 2) <= 0.5
    int d = twice_d / 2;
    if (d > 9) d = 9;
    if (d <= (int)kPackLog) return 0;                                // a 64-leaf build group must sit inside one cell
    if ((int)c.phi_width - 2 - d < 2) return 0;
    return (uint32_t)d;
}

// octant mirror (k_table_build_mirror): residual / nibble entries, tables of 2^20 entries and more, and the
// exact quarter turn 2 * lut[0] == E << z_shl the symmetry rests on (true for every model at z_shr == 0; checked, not assumed)
bool bhwk_build_mirror_applies(const BhwCordicCfg &c, uint32_t entries)
{
    const int fmt = fmt_of(c.tab_dlog);
    return (fmt == 2 || fmt == 3 || fmt == 5) && (c.tab_split || fmt != 2) && c.z_shr == 0 && entries >= (1u << 20) && c.n_iter >= 21 &&
           c.dat_width + c.out_shr <= 34 && 2ull * (uint64_t)(uint32_t)c.lut[0] == ((uint64_t)entries << c.z_shl);
}

// Workgroup size of the mirror kernel: 1 024 threads (16 waves, every wave walks 16 groups) where that still gives every CU of
// a 256-CU device its two workgroups (tables of 2^24 entries and more), 256 threads below (profiles/r04_ab_build_wg.txt)
unsigned bhwk_build_mirror_threads(uint32_t entries)
{
    return entries >= (1u << 24) ? 1024u : 256u;
}

BhwTableLayout bhwp_table_layout(uint64_t E, uint32_t tab_dlog)
{
    const int fmt = fmt_of(tab_dlog);
    const uint64_t entry_bytes = fmt == 0 ? 8ull : fmt == 1 ? 4ull : fmt == 2 ? 2ull : 1ull;
    const uint64_t coarse_bytes = fmt == 0 ? 0ull : fmt == 1 ? (E >> kPackLog) * 8ull : (E >> fmt_cell_log(tab_dlog)) * 16ull;
    BhwTableLayout l;
    l.coarse_off = align256(E * entry_bytes);
    l.esc_off = 0;
    l.esc_wg_log = 0;
    l.check_off = l.coarse_off + align256(coarse_bytes);
    if (fmt == 5) {
        // one list per workgroup of the mirror build kernel: it owns 64 x (threads / 4) entries of [0, E/2) and their images
        const uint32_t gpw = bhwk_build_mirror_threads((uint32_t)E) / 4u;
        uint32_t lg = 6;
        while ((1u << (lg - 6)) < gpw) ++lg;
        l.esc_wg_log = lg;
        const uint64_t n_wg = ((E >> 1) + (1ull << lg) - 1ull) >> lg;
        l.esc_off = l.check_off;
        l.check_off = l.esc_off + align256(n_wg * kEscSlots * 16ull);
    }
    l.bytes = fmt == 0 ? E * 8ull : l.check_off + 256ull;          // plain tables carry neither records nor a check word
    return l;
}

// Table formats a tiled whole-period call may use, narrowest first (tab_dlog values: 16 + d nibble, 48 + d nibble + escapes,
// d = 7..9 residual, 6 delta16, 0 plain).  The packed build variants exist from 21 rotations on (always true at PW >= 22).  Residual / nibble tables are built
// by the octant-mirror kernel only, so they are proposed only where it applies.
int bhwp_table_format_candidates(const BhwCordicCfg &c, bool tiled, uint32_t limit, uint32_t out[kMaxFormats])
{
    int n = 0;
    if (tiled && c.n_iter >= 21) {
        uint32_t d = bhwk_resid_dlog(c);
        if (d) {
            BhwCordicCfg probe = c;
            probe.tab_dlog = d;
            probe.tab_split = 1u;
            if (!bhwk_build_mirror_applies(probe, (uint32_t)bhwp_table_entries(c))) d = 0;
        }
        if (d && (limit == BHW_TABLE_BEST || limit == BHW_TABLE_NIBBLE)) out[n++] = kNibbleFlag + d;
        // the same one-byte entries with the rare deviation that does not fit listed exactly (models whose CORDIC noise is wider than
        // the 4-bit fields: cpp, VHDL at 32 bits)
        if (d && (limit == BHW_TABLE_BEST || limit == BHW_TABLE_NIBBLE || limit == BHW_TABLE_NIBBLE_ESC)) out[n++] = kEscFlag + kNibbleFlag + d;
        if (d && (limit == BHW_TABLE_BEST || limit == BHW_TABLE_NIBBLE || limit == BHW_TABLE_NIBBLE_ESC || limit == BHW_TABLE_RESIDUAL)) out[n++] = d;
        if (bhwk_packed_ok(c) && limit != BHW_TABLE_PLAIN) out[n++] = kPackLog;
    }
    out[n++] = 0u;
    return n;
}

int bhwp_fmt_verdict(const bhw_params *p, uint32_t dlog)
{
    std::lock_guard<std::mutex> lk(g_fmt_mu);
    auto it = g_fmt_verdict.find(fmt_key(p, dlog));
    return it == g_fmt_verdict.end() ? kFmtUnknown : it->second;
}

void bhwp_fmt_set_verdict(const bhw_params *p, uint32_t dlog, int v)
{
    std::lock_guard<std::mutex> lk(g_fmt_mu);
    if (v == kFmtOk || v == kFmtBad) g_fmt_verdict[fmt_key(p, dlog)] = v;
    else g_fmt_verdict.erase(fmt_key(p, dlog));                  // anything else: forget it (unknown again)
}

BhwFormatWalk bhwp_format_walk(const bhw_params *p, const BhwCordicCfg &c, bool tiled, uint32_t limit, bool capturing)
{
    uint32_t cand[kMaxFormats];
    const int n = bhwp_table_format_candidates(c, tiled, limit, cand);
    const uint64_t E = bhwp_table_entries(c);
    BhwFormatWalk fw{};
    for (int i = 0; i < n; ++i) {
        const int v = cand[i] ? bhwp_fmt_verdict(p, cand[i]) : (int)kFmtOk;
        if (v == kFmtBad || (v == kFmtUnknown && capturing)) continue;
        const uint64_t b = bhwp_table_layout(E, cand[i]).bytes;
        if (b > fw.scratch_bytes) fw.scratch_bytes = b;
        if (v == kFmtOk) {
            fw.kept = cand[i];
            break;
        }
        fw.open[fw.n_open++] = cand[i];
    }
    return fw;
}

const char *bhwp_format_name(uint32_t tab_dlog)
{
    return tab_dlog == 0 ? "plain" : tab_dlog == kPackLog ? "delta16" : tab_dlog >= kEscFlag ? "nibble+esc" : tab_dlog >= kNibbleFlag ? "nibble" : "residual";
}

// ---- combine pass: tile plan ------------------------------------------------------------------------------------------------------

bool bhwk_tile_applicable(const BhwCordicCfg &c, const BhwWinCfg &w)
{
    // With dropped phase bits (z_shr > 0) consecutive lanes share table entries, so the gathers are dense on their
    // own: such tables take the one-run form of the kernel over the natural layout.
    (void)w;
    // below 2^22 coefficients a grid of 960-thread tiles leaves CUs idle; the one-lane-per-four fold kernel has many more,
    // smaller workgroups and wins there (2^20: 15.0 vs 18.7 us, 2^21: 20.5 vs 21.2, 2^22: 36.0 vs 25.8; BH-7)
    return c.phi_width >= 22 && c.phi_width <= 30;
}

void bhwp_tile_plan(const BhwCordicCfg &c, const BhwWinCfg &w, BhwTilePlan &tp, int &nb, uint32_t &lanes)
{
    const uint32_t lq = c.phi_width - 2, E = 1u << (lq - 1);   // the lane ring is [0, N/8): each lane owns r and r + N/8
    const uint32_t inv3 = inv_mod_pow2(3, lq - 1), inv5 = inv_mod_pow2(5, lq - 1);
    const int nb3 = (c.z_shr == 0 && w.n_terms > 3) ? 3 : 1, nb5 = (c.z_shr == 0 && w.n_terms > 5) ? 5 : 1;
    nb = nb3 * nb5;
    uint32_t sorted[15];
    for (int i5 = 0; i5 < nb5; ++i5)
        for (int i3 = 0; i3 < nb3; ++i3) {
            const uint32_t o = (uint32_t)(((uint64_t)i3 * inv3 + (uint64_t)i5 * inv5) & (E - 1u));
            // 3 thread groups: group p holds the five inv5-siblings of i3 = p (k = 5 dense per thread);
            // 5 thread groups (kTileThreads = 5 * kTileLanes): group p holds the three inv3-siblings of i5 = p
            if (kTileThreads / kTileLanes == 5 && nb == 15) tp.offs[i3 + nb3 * i5] = o;
            else tp.offs[i5 + nb5 * i3] = o;
            sorted[i3 + nb3 * i5] = o;
        }
    for (int i = nb; i < 16; ++i) tp.offs[i] = tp.offs[nb - 1];
    // tiles needed so that every run class sweeps past the start of the next one around the ring
    for (int i = 1; i < nb; ++i)
        for (int j = i; j > 0 && sorted[j - 1] > sorted[j]; --j) { uint32_t t = sorted[j]; sorted[j] = sorted[j - 1]; sorted[j - 1] = t; }
    uint64_t maxgap = 0;
    for (int i = 0; i < nb; ++i) {
        const uint64_t nxt = (i + 1 < nb) ? sorted[i + 1] : (uint64_t)sorted[0] + E;
        if (nxt - sorted[i] > maxgap) maxgap = nxt - sorted[i];
    }
    lanes = (nb >= 15) ? (uint32_t)kTileLanes : (uint32_t)kTileThreads;
    tp.n_tiles = (uint32_t)((maxgap + lanes - 1) / lanes);
    tp.tile0 = 0;
    tp.img_mask = 0xFFu;
    tp.n0mod = 0u;
}

// one-instruction products (tile_harmonic FAST): 15-run tiles, every harmonic weight below 2^(W-3) in magnitude (the built-in
// weights are: a_k <= 0.49 * 2^(W-1 or W-2)); caller-scaled weights beyond that take the 64-bit products.  VHDL rule, one-word
// sums: |sum of the terms| <= sum of (|a_k| + 1) must also stay below 2^31 (the built-in weights: < 2^(W-1))
bool bhwp_tile_fast(const BhwCordicCfg &c, const BhwWinCfg &w, int nb)
{
    bool fast = nb == 15 && c.dat_width >= 3;
    for (uint32_t k = 1; k < w.n_terms && fast; ++k) {
        const int64_t lim = (int64_t)1 << (c.dat_width - 3);
        fast = (int64_t)w.aa[k] < lim && (int64_t)w.aa[k] > -lim;       // (> : the kernel also multiplies by the negated pre-shifted weight)
    }
    if (w.combine != BHW_COMBINE_HLS && fast) {
        int64_t bound = 0;
        for (uint32_t k = 0; k < w.n_terms; ++k) bound += (w.aa[k] < 0 ? -(int64_t)w.aa[k] : (int64_t)w.aa[k]) + 1;
        fast = bound < ((int64_t)1 << 31);
    }
    return fast;
}

// Measured per instance (profiles/r05_kernel_stats_all_legs_tile9_everywhere.csv against round 4's): plain nibbles 60.6 us (HLS rule,
// 61.3 before) and 61.3 us (VHDL rule at 32 bits, 71.7 before); nibble + escapes 69.7 us with the VHDL rule at 32 bits (74.2 before)
// but 68.9 - 70.8 us with the HLS rule, against 64 - 67 in k_table_combine_tile: those stay where they were (-DBHW_T9_ALLFMT5 sends
// them here for the A/B harness).  What those tables cost is not the escape test -- with the marker never looked for, or the very
// code of the plain-nibble instance run over them, the pass stays 6 us slower than over an HLS-model table
// (profiles/r05_ab_tile9_cpp_model_fmt5.txt, r05_ab_tile9_fmt5_code_vs_table.txt): unexplained, recorded as such.
bool bhwk_tile9_applicable(const BhwCordicCfg &c, const BhwWinCfg &w, int nb, bool fast, bool masked)
{
    const int fmt = fmt_of(c.tab_dlog);
    if (!(nb == 15 && fast && !masked && fmt_cell_log(c.tab_dlog) == kTile9CellLog && c.z_shr == 0)) return false;
#ifdef BHW_T9_ALLFMT5
    return fmt == 3 || fmt == 5;                                     // (development: every nibble + escapes instance, for the A/B harness)
#else
    return fmt == 3 || (fmt == 5 && w.combine != BHW_COMBINE_HLS && c.dat_width == 32u);
#endif
}

// A contiguous index range that is a whole number of eighths of the window (and less than all of it) can be produced by the
// tile kernel as a subset of its eight images: `*img_mask` = the images, `*n0mod` = n0 mod N (see BhwTilePlan).
bool bhwk_tile_images_applicable(const BhwCordicCfg &c, const BhwWinCfg &w, uint64_t n0, uint64_t count, uint32_t *img_mask, uint32_t *n0mod)
{
    if (!bhwk_tile_applicable(c, w) || c.z_shr != 0 || w.apply_x != nullptr || w.n_terms <= 5) return false;   // 15-run tiles only
    const uint64_t N = 1ull << c.phi_width, eighth = N >> 3;
    if (count == 0 || count >= N || (count % eighth) != 0 || (n0 % eighth) != 0) return false;
    const uint32_t m0 = (uint32_t)((n0 % N) / eighth), n_img = (uint32_t)(count / eighth);
    uint32_t mask = 0;
    for (uint32_t i = 0; i < n_img; ++i) mask |= 1u << ((m0 + i) & 7u);
    *img_mask = mask;
    *n0mod = (uint32_t)(n0 % N);
    return true;
}

BhwTableCall bhwp_table_call(const bhw_params *p, const BhwCordicCfg &c, const BhwWinCfg &w, uint64_t n0, uint64_t count, bool apply)
{
    BhwTableCall t;
    t.has_period = bhwp_has_whole_period(p, n0, count);
    t.img_mask = 0xFFu;
    t.n0mod = 0u;
    BhwWinCfg probe = w;
    if (apply && !probe.apply_x) probe.apply_x = reinterpret_cast<const int32_t *>(uintptr_t(1));   // "an input exists"
    t.images = !t.has_period && bhwk_tile_images_applicable(c, probe, n0, count, &t.img_mask, &t.n0mod);
    t.tiled = (t.has_period && bhwk_tile_applicable(c, w)) || t.images;
    return t;
}

// Run-length kernel: z_shr > 0, at most one entry step per harmonic inside a 16-lane run, ring a multiple of the workgroup's
// 2048 lanes, plain natural table, 16-byte aligned output, no fused apply; VHDL rule in int32 needs W + 2 <= 30.
bool bhwk_runlength_applicable(const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *d_out)
{
    if (c.z_shr == 0 || c.tab_dlog != 0 || c.tab_split != 0 || w.apply_x != nullptr) return false;
    if (c.phi_width < 15 || c.phi_width > 30) return false;                       // ring (2^(PW-3)) >= 2048 lanes
    if (((w.n_terms - 1u) * (uint32_t)kRlRun) > (1u << c.z_shr)) return false;
    if (c.phi_width - 2u - c.z_shr < 2u) return false;                            // H a multiple of 2^z_shr
    if (w.combine != BHW_COMBINE_HLS && c.dat_width > 28) return false;
    return (((uintptr_t)d_out) & 15u) == 0;                                       // (NULL: the caller asks about the configuration only)
}

// ---- fused kernel -------------------------------------------------------------------------------------------------------------------

bool bhwk_fold_direct_applicable(const BhwCordicCfg &c)
{
    // rot_step's forms: |x| < 2^33 and a quarter circle <= 2^32; ring of at least one wave
    return c.dat_width + c.out_shr <= 34 && c.phi_width >= 9 && c.phi_width <= 30 && c.n_iter >= 2;
}

int bhwp_fold_form(const BhwCordicCfg &c, const BhwWinCfg &w, uint64_t total)
{
    // on 32-bit state with in-wave prefixes when x, y (|.| < 2^(W + out_shr - 1)) and z (the quarter circle) fit signed words -- at
    // every launch size: where the chip is full the form still wins a little over the 64-bit one with its own split level per chain
    // (BH-4 2^22 / 24-bit 16.1 -> 15.2 us, BH-5 17.7 -> 17.4)
    const bool narrow = c.dat_width + c.out_shr <= 30u && c.phi_width - 2u - c.z_shr + c.z_shl <= 30u;
    // short launches, form of the kernel: one chain per wave over the same 64 lanes (k_fold_split), lockstep, or sequential.
    // measured per call (profiles/r02_ab_fused_lockstep.txt): split 7.8 / lockstep 9.0 us at 2^13 lanes (BH-7 2^16), 6.9 / 7.7 at
    // 2^15 (BH-5 2^18), 9.7 / 9.7 at 2^16, 9.0 / 8.2 at 2^17 (BH-4 2^20): split up to 2^15 lanes, lockstep up to 2^18
    // (round 3, tools/bench_short_graph.py: where the narrow form applies it beats the split one at every size for windows of up to
    // five terms -- 4.4 / 4.5 / 4.8 against 5.1 / 5.2 / 5.5 us at 2^14 / 2^16 / 2^18 points of BH-4 -- and loses to it with the nine
    // chains of a 7-term window, 6.8 against 6.6 us at 2^16)
    // (round 5, one chain per wave in the split form -- profiles/r05_short_windows_split*.txt: 7.1 -> 5.0 us for BH-7 2^16 at 32 bits; it
    // now also wins one size up for windows of up to five terms, 2^16 lanes: BH-4 2^19 / 32-bit 7.07 -> 6.23 us, BH-3 5.96 -> 5.00, BH-5
    // 7.35 -> 6.85, while the nine chains of a 7-term window lose there, 9.01 -> 9.50, and everything loses at 2^17 lanes)
    const uint64_t split_max = w.n_terms <= 5 ? (1u << 16) : (1u << 15);
    if (total <= split_max && !(narrow && w.n_terms <= 5)) return BHWP_FOLD_SPLIT;
    if (narrow) return BHWP_FOLD_NARROW;
    // fewer than ~4 waves per SIMD in the whole launch: latency-bound, walk the chains in lockstep
    return total <= (1u << 18) ? BHWP_FOLD_LOCKSTEP : BHWP_FOLD_SEQUENTIAL;
}

uint32_t bhwp_fold_k24(const BhwCordicCfg &c)
{
    // |x|, |y| < 2^B, B = W + out_shr - 1: (x >> k) fits 24 signed bits from k = B - 23 on; twice the ROM word (the kernel carries the
    // angle doubled: rot_mad24) from the first lut[k] < 2^22 on
    const int B = (int)(c.dat_width + c.out_shr) - 1;
    uint32_t k24 = B > 23 ? (uint32_t)(B - 23) : 1u;
    while (k24 < c.n_iter && k24 < 32u && (uint32_t)c.lut[k24] >= (1u << 22)) ++k24;
    return k24;
}

// ---- ownership parts ----------------------------------------------------------------------------------------------------------------

// Interleaved ownership (bhw_generate_part_device): the ring lanes of part `part` of `n_parts`, as runs of consecutive r.
// Where the tile kernel applies the parts are contiguous ranges of its tiles, i.e. the plan's sibling runs (so a part can be
// produced by the tile kernel over the full table or by the fused kernel, with the same ownership); elsewhere they are
// contiguous ranges of the ring in 64-lane units.  Runs that wrap the ring are split; neighbouring parts overlap by the few
// lanes the tile plan covers twice at its seams (identical values).
int bhwk_part_runs(const BhwCordicCfg &c, const BhwWinCfg &w, uint32_t part, uint32_t n_parts, BhwFoldRun *runs, uint32_t *tile0, uint32_t *tile_count)
{
    const uint32_t H = 1u << (c.phi_width - 3);
    *tile0 = *tile_count = 0;
    if (n_parts < 1) n_parts = 1;
    if (!bhwk_tile_applicable(c, w)) {
        const uint32_t units = (H + 63u) >> 6;
        const uint32_t a = (uint32_t)((uint64_t)units * part / n_parts) << 6, b = (uint32_t)((uint64_t)units * (part + 1u) / n_parts) << 6;
        runs[0] = BhwFoldRun{a < H ? a : H, b < H ? b : H};
        return runs[0].r_end > runs[0].r0 ? 1 : 0;
    }
    BhwTilePlan tp;
    int nb;
    uint32_t lanes;
    bhwp_tile_plan(c, w, tp, nb, lanes);
    const uint32_t t0 = (uint32_t)((uint64_t)tp.n_tiles * part / n_parts), t1 = (uint32_t)((uint64_t)tp.n_tiles * (part + 1u) / n_parts);
    *tile0 = t0;
    *tile_count = t1 - t0;
    if (t1 == t0) return 0;
    const uint64_t len = (uint64_t)(t1 - t0) * lanes;
    int n = 0;
    for (int b = 0; b < nb; ++b) {
        if (len >= H) { runs[0] = BhwFoldRun{0u, H}; return 1; }
        const uint32_t start = (uint32_t)(((uint64_t)t0 * lanes + tp.offs[b]) & (H - 1u));
        if (start + len <= H) runs[n++] = BhwFoldRun{start, (uint32_t)(start + len)};
        else {
            runs[n++] = BhwFoldRun{start, H};
            runs[n++] = BhwFoldRun{0u, (uint32_t)(start + len - H)};
        }
    }
    return n;
}

int bhwp_part_checks(const bhw_params *p, uint32_t part, uint32_t n_parts)
{
    int rc = bhwp_validate(p);
    if (rc) return rc;
    if (p->sin_type != BHW_SIN_CORDIC) return bhwp_fail(BHW_ERR_UNSUPPORTED, "interleaved parts exist for the CORDIC source only");
    if (n_parts < 1 || n_parts > 64 || part >= n_parts) return bhwp_fail(BHW_ERR_BADARG, "part %u of %u (1..64 parts)", part, n_parts);
    if (p->phi_width < 9) return bhwp_fail(BHW_ERR_UNSUPPORTED, "interleaved parts need phi_width >= 9 (a ring of 64 lanes)");
    // a part is produced by the fused kernel (CORDIC state within 34 bits) or by the tile kernel over the full table (N >= 2^22):
    // configurations with neither (e.g. VHDL model, W = 32, PRECISION >= 3 below 2^22) have no part kernel, and the segment
    // arithmetic must not promise what bhw_generate_part_device cannot deliver
    BhwCordicCfg c;
    bhwp_resolve_cordic(p, c);
    BhwWinCfg w;
    bhwp_resolve_window(p, w);
    if (!bhwk_fold_direct_applicable(c) && !bhwk_tile_applicable(c, w))
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "no kernel produces ownership parts of this configuration (CORDIC state beyond 34 bits and no tile plan)");
    return BHW_OK;
}

// Strategy of one ownership part.  Fused: chains = lanes x (chains per lane), no table.  Table: the full first-quadrant table (it
// does not shrink with the part) + this part's tiles.  Measured per part (BH-7 2^26 / 32-bit, profiles/r04_small_windows_and_parts.json):
// table 0.068 / 0.055 / 0.049 ms at 2 / 4 / 8 parts, fused 0.092 / 0.051 ms at 4 / 8 -- the build pass got 20 % faster this round and the
// crossover moved out: the fused kernel is taken once the part's own chains (9/8 per owned coefficient) are at most HALF the
// table's (more than 8 parts of this window).  (Round 3's file showed 0.1195 ms for AUTO at one part against 0.1123 for the same
// table plan: the first timing after a run of short kernels -- clocks, not the plan; the tool now ramps again before that section.)
bool bhwp_part_fused(const bhw_params *p, const BhwCordicCfg &c, const BhwFoldRun *runs, int n_runs, uint32_t tile_count, uint32_t requested, int *rc)
{
    *rc = BHW_OK;
    uint64_t lanes = 0;
    for (int i = 0; i < n_runs; ++i) lanes += runs[i].r_end - runs[i].r0;
    static const int kChains[8] = {0, 0, 2, 3, 5, 6, 0, 9};
    const uint64_t chains_fused = lanes * (uint64_t)kChains[p->n_terms];
    const bool fused_ok = bhwk_fold_direct_applicable(c);
    const bool table_ok = tile_count != 0;                     // tile-aligned ownership: the tile kernel can produce exactly this part
    bool fused;
    if (requested == BHW_ALGO_FUSED) fused = fused_ok;
    else if (requested == BHW_ALGO_TABLE) fused = !table_ok;
    else fused = fused_ok && (!table_ok || 2 * chains_fused <= bhwp_table_entries(c));
    if (fused && !fused_ok) *rc = bhwp_fail(BHW_ERR_UNSUPPORTED, "no kernel produces this part (CORDIC state beyond 34 bits and no tile plan)");
    if (!fused && !table_ok) *rc = bhwp_fail(BHW_ERR_UNSUPPORTED, "the table strategy produces whole tiles only and this window has no tile plan");
    return fused;
}

// Kernel names of the table strategy's two passes for a resolved configuration (bhw_describe_plan: profilers, bench labels).
// Mirrors the dispatch in bhwk_table_build / bhwk_table_combine_tile_range / bhwk_table_combine_fold.
void bhwk_describe_table(const BhwCordicCfg &c_in, const BhwWinCfg &w, bool tiled, bool images, char *build, char *combine, size_t len)
{
    const BhwCordicCfg c = table_layout(c_in);
    const uint32_t entries = 1u << (c.phi_width - 2 - c.z_shr);
    const bool fits = (c.dat_width + c.out_shr <= 34);
    const int fmt = fmt_of(c.tab_dlog);
    if (fits && c.n_iter >= 7 && entries < (1u << 20) && c.tab_dlog == 0 && !c.tab_split) snprintf(build, len, "k_table_build_plain<%u>", c.n_iter);
    else if (entries >= 64 && fits && c.n_iter >= 2) {
        if (bhwk_build_mirror_applies(c, entries)) snprintf(build, len, "k_table_build_mirror<%u,%d,%u>", c.n_iter, fmt, bhwk_build_mirror_threads(entries));
        else snprintf(build, len, "k_table_build_shared<%u,%d>", c.n_iter, fmt);
    } else snprintf(build, len, "k_table_build<%s>", c.wide ? "int64_t" : "int32_t");
    const int mode = mode_of(c, w);
    if (tiled) {
        const int nb3 = (c.z_shr == 0 && w.n_terms > 3) ? 3 : 1, nb5 = (c.z_shr == 0 && w.n_terms > 5) ? 5 : 1;
        // (`images`: a subset of the eight images, which k_table_combine_tile's MASKED instances produce)
        if (bhwk_tile9_applicable(c, w, nb3 * nb5, bhwp_tile_fast(c, w, nb3 * nb5), images)) snprintf(combine, len, "k_tile9<%d,%d>", mode, fmt);
        else snprintf(combine, len, "k_table_combine_tile<%d,%d,%d>", nb3 * nb5, mode, fmt);
    } else if (c.tab_dlog == 0 && !c.tab_split) snprintf(combine, len, "k_table_combine_fold_t<%u,%d>", w.n_terms, mode);
    else snprintf(combine, len, "k_table_combine_fold");
}

// ---- resident tables ------------------------------------------------------------------------------------------------------------

int bhwp_table_create_checks(const bhw_params *p, uint32_t table_format)
{
    if (!p) return bhwp_fail(BHW_ERR_BADARG, "params is NULL");
    const int rc = bhwp_validate(p);        // (cordic_dds48 / cordic_dds_scaled: UNSUPPORTED, they feed no window)
    if (rc) return rc;
    if (p->sin_type != BHW_SIN_CORDIC)
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "resident tables hold the CORDIC table; the Taylor ROM is cached by the library already");
    if (table_format > BHW_TABLE_NIBBLE_ESC) return bhwp_fail(BHW_ERR_BADARG, "table_format %u", table_format);
    return BHW_OK;
}

// The table depends on the CORDIC generics only -- the fields fmt_key() keys the format verdicts by.
int bhwp_table_key_check(const bhw_params *pt, const bhw_params *p)
{
    if (!pt || !p) return bhwp_fail(BHW_ERR_BADARG, "params is NULL");
    if (p->sin_type != BHW_SIN_CORDIC) return bhwp_fail(BHW_ERR_BADARG, "sin_type %u: a resident table serves the CORDIC source only", p->sin_type);
    if (p->model != pt->model) return bhwp_fail(BHW_ERR_BADARG, "model %u differs from the table's %u", p->model, pt->model);
    if (p->phi_width != pt->phi_width)
        return bhwp_fail(BHW_ERR_BADARG, "phi_width %u differs from the table's %u", p->phi_width, pt->phi_width);
    if (p->dat_width != pt->dat_width)
        return bhwp_fail(BHW_ERR_BADARG, "dat_width %u differs from the table's %u", p->dat_width, pt->dat_width);
    if (p->model == BHW_MODEL_VHDL && p->precision != pt->precision)
        return bhwp_fail(BHW_ERR_BADARG, "precision %u differs from the table's %u", p->precision, pt->precision);
    return BHW_OK;
}

void bhwp_resident_layout(const bhw_params *p, BhwCordicCfg &c, bool *tiled)
{
    bhwp_resolve_cordic(p, c);
    BhwWinCfg w;
    bhwp_resolve_window(p, w);
    *tiled = bhwk_tile_applicable(c, w);                  // (a property of phi_width alone: the weights do not enter)
    c.tab_split = (*tiled && c.z_shr == 0) ? 1u : 0u;
}

bool bhwp_range_form(const BhwCordicCfg &c, const BhwWinCfg &w, int *fmt, int *nt, int *mode)
{
    *fmt = fmt_of(c.tab_dlog);
    *nt = w.n_terms <= 3 ? 3 : w.n_terms <= 5 ? 5 : 7;
    *mode = mode_of(c, w);
    return *fmt == 0 || *fmt == 1 || *fmt == 2 || *fmt == 3 || *fmt == 5;
}

int bhwp_describe_from_table(const bhw_params *p, const BhwCordicCfg &ct, bool tiled, uint64_t n0, uint64_t count, char *buf, uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const BhwCordicCfg c = table_layout(ct);
    BhwWinCfg w;
    bhwp_resolve_window(p, w);
    const uint64_t N = 1ull << p->phi_width, E = bhwp_table_entries(c);
    char ragged[64], period[128], build[64], combine[96];
    int rf, rn, rm;
    if (bhwp_range_form(c, w, &rf, &rn, &rm)) snprintf(ragged, sizeof ragged, "k_range_combine<%d,%d,%d>", rf, rn, rm);
    else snprintf(ragged, sizeof ragged, "k_table_combine");
    const BhwTableCall t = bhwp_table_call(p, c, w, n0, count, false);
    bhwk_describe_table(c, w, tiled || t.images, t.images, build, combine, sizeof build);
    if (bhwk_runlength_applicable(c, w, nullptr))
        snprintf(period, sizeof period, "k_runlength_window<%u,%d,%s> (16-byte aligned output; else %s)", p->n_terms, mode_of(c, w),
                 rl_narrow(c) ? "true" : "false", combine);
    else snprintf(period, sizeof period, "%s", combine);
    const uint64_t head = (N - n0 % N) % N;
    const uint64_t periods = t.has_period ? (count - head) / N : 0, tail = t.has_period ? count - head - periods * N : 0;
    char calls[320];
    if (!count) snprintf(calls, sizeof calls, "nothing");
    else if (t.images) snprintf(calls, sizeof calls, "%s (image subset)", combine);
    else if (!t.has_period) snprintf(calls, sizeof calls, "%s", ragged);
    else {
        const std::string ends = head || tail ? std::string(" + ") + ragged + " on the ragged ends" : std::string();
        snprintf(calls, sizeof calls, "%s%s%s", period, periods > 1 ? " + k_replicate" : "", ends.c_str());
    }
    snprintf(buf, len, "resident table[%s, %s, %llu bytes]: %s", bhwp_format_name(c.tab_dlog), c.tab_split ? "split" : "natural",
             (unsigned long long)bhwp_table_layout(E, c.tab_dlog).bytes, calls);
    return BHW_OK;
}

// ---- overlapped-frame apply --------------------------------------------------------------------------------------------------

namespace {

// The kernel a launch from the resident table ct takes (`table`<fmt,nt,mode>, bhwp_range_form) or, with ct NULL, the direct chains
// (`direct`<direct_form>): the rules the launchers pick the instance by, with the _len suffix of the any-length kernels.
void kernel_name(const bhw_params *p, const BhwCordicCfg *ct, const char *direct, const char *table, bool any_len, char *out, size_t len)
{
    const char *sfx = any_len ? "_len" : "";
    if (ct) {
        BhwWinCfg w;
        bhwp_resolve_window(p, w);
        int fmt, nt, mode;
        bhwp_range_form(table_layout(*ct), w, &fmt, &nt, &mode);
        snprintf(out, len, "%s%s<%d,%d,%d>", table, sfx, fmt, nt, mode);
    } else {
        BhwCordicCfg c;
        bhwp_resolve_cordic(p, c);
        snprintf(out, len, "%s%s<%d>", direct, sfx, direct_form(c));
    }
}

// the describe line of a frames launch (bhwp_describe_frames, bhwp_describe_len): prefix, kernel, plan shape
// (direct / table: the kernel names, those of the float32 kernels for bhwp_describe_f32)
void frames_line(const char *prefix, const bhw_params *p, const BhwCordicCfg *ct, const bhw_frames *f, const BhwFramesPlan &pl, bool any_len,
                 char *buf, uint64_t len, const char *direct = "k_frames_direct", const char *table = "k_frames_table")
{
    char kern[64];
    kernel_name(p, ct, direct, table, any_len, kern, sizeof kern);
    snprintf(buf, len, "%s%s, %u channel%s, G = %llu frames per lane, grid %llu x %llu x %u lanes (%u along k)", prefix, kern, f->channels,
             f->channels == 2 ? "s" : "", (unsigned long long)pl.group, (unsigned long long)pl.grid_x, (unsigned long long)pl.grid_y,
             kFramesBlock, pl.kx);
}

// the describe line of an overlap-add launch with count > 0 (bhwp_describe_ola, bhwp_describe_len): prefix, kernel, plan shape
void ola_line(const char *prefix, const bhw_params *p, const BhwCordicCfg *ct, const bhw_ola *o, const BhwOlaPlan &pl, bool any_len, char *buf,
              uint64_t len, const char *direct = "k_ola_direct", const char *table = "k_ola_table")
{
    char kern[64];
    kernel_name(p, ct, direct, table, any_len, kern, sizeof kern);
    snprintf(buf, len, "%s%s, %u channel%s, Q = %u hops per lane, up to %llu frames per output, grid %llu x %llu x %u lanes (%u along r, "
             "%u along q)", prefix, kern, o->channels, o->channels == 2 ? "s" : "", pl.q, (unsigned long long)pl.jmax,
             (unsigned long long)pl.grid_x, (unsigned long long)pl.grid_y, kOlaBlock, pl.rx, pl.fy);
}

} // namespace

int bhwp_frames_checks(const bhw_params *p, const bhw_frames *f, const void *d_x, const void *d_y, bool pointers, uint64_t length)
{
    if (!p) return bhwp_fail(BHW_ERR_BADARG, "params is NULL");
    int rc = bhwp_validate(p);
    if (rc) return rc;
    if (!f) return bhwp_fail(BHW_ERR_BADARG, "frames descriptor is NULL");
    if (f->struct_size != sizeof(bhw_frames)) return bhwp_fail(BHW_ERR_BADARG, "bhw_frames.struct_size %u != %zu", f->struct_size, sizeof(bhw_frames));
    if (f->channels != 1 && f->channels != 2) return bhwp_fail(BHW_ERR_BADARG, "channels %u (1 or 2)", f->channels);
    if (f->hop == 0) return bhwp_fail(BHW_ERR_BADARG, "hop is 0");
    if (f->shift > 62) return bhwp_fail(BHW_ERR_BADARG, "shift %u > 62", f->shift);
    if (f->reserved) return bhwp_fail(BHW_ERR_BADARG, "bhw_frames.reserved must be 0");
    const uint64_t N = length ? length : 1ull << p->phi_width, NC = N * f->channels;
    if (f->y_stride && f->y_stride < NC)
        return bhwp_fail(BHW_ERR_BADARG, "y_stride %llu < N * channels = %llu", (unsigned long long)f->y_stride, (unsigned long long)NC);
    if (p->sin_type != BHW_SIN_CORDIC && f->channels == 2)
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "the Taylor sources take the per-frame route, which has no I/Q form (channels 2)");
    if (!f->frames) return BHW_OK;
    if (f->frames > (1ull << 34) / N)
        return bhwp_fail(BHW_ERR_BADARG, "frames * N = %llu * %llu > 2^34 per call", (unsigned long long)f->frames, (unsigned long long)N);
    if (!pointers) return BHW_OK;
    if (!d_x || !d_y) return bhwp_fail(BHW_ERR_BADARG, "d_x / d_y is NULL");
    // extents in int32 elements; hop and y_stride are free 64-bit values, so the products are taken in 128 bits
    const unsigned __int128 xe = ((unsigned __int128)(f->frames - 1) * f->hop + N) * f->channels;
    const unsigned __int128 ye = (unsigned __int128)(f->frames - 1) * (f->y_stride ? f->y_stride : NC) + NC;
    if (xe > (1ull << 60) || ye > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "x or y extent beyond 2^60 elements");
    const uint64_t xa = (uint64_t)(uintptr_t)d_x, ya = (uint64_t)(uintptr_t)d_y, xb = (uint64_t)xe * 4u, yb = (uint64_t)ye * 4u;
    if (xa > UINT64_MAX - xb || ya > UINT64_MAX - yb) return bhwp_fail(BHW_ERR_BADARG, "x or y range wraps the address space");
    if (xa < ya + yb && ya < xa + xb) return bhwp_fail(BHW_ERR_BADARG, "d_y must not overlap d_x");
    return BHW_OK;
}

BhwFramesPlan bhwp_frames_plan(const bhw_params *p, const bhw_frames *f, bool from_table, int force_route, uint64_t length, bool f32)
{
    BhwFramesPlan pl{};
    const uint64_t N = length ? length : 1ull << p->phi_width;
    pl.len = N;
    pl.y_stride = f->y_stride ? f->y_stride : N * f->channels;
    if (from_table) pl.route = BHWP_FRAMES_TABLE;
    else if (length || f32) pl.route = BHWP_FRAMES_DIRECT;                     // the any-length and float32 kernels have no per-frame route
    else if (f->channels == 2) pl.route = BHWP_FRAMES_DIRECT;                  // the existing apply has no I/Q form
    else if (p->sin_type != BHW_SIN_CORDIC) pl.route = BHWP_FRAMES_PER_FRAME;  // no frames kernel for the Taylor sources
    else {
        BhwCordicCfg c;
        bhwp_resolve_cordic(p, c);
        const uint64_t work = (uint64_t)(p->n_terms - 1) * c.n_iter;       // direct CORDIC rotations per coefficient
        const bool per_frame = f->frames * kFramesPerFrameRef < (uint64_t)bhwp_frames_crossover(p->phi_width) * work;
        pl.route = per_frame ? BHWP_FRAMES_PER_FRAME : BHWP_FRAMES_DIRECT;
    }
    if (force_route >= 0 && !from_table && !f32 && force_route != BHWP_FRAMES_TABLE &&
        !(force_route == BHWP_FRAMES_PER_FRAME && f->channels == 2) && !(force_route == BHWP_FRAMES_DIRECT && p->sin_type != BHW_SIN_CORDIC))
        pl.route = force_route;
    pl.kx = 1;                                                                 // N itself, or the power of two at or above L
    while (pl.kx < kFramesBlock && pl.kx < N) pl.kx *= 2;
    pl.fy = kFramesBlock / pl.kx;
    pl.grid_x = (N + pl.kx - 1) / pl.kx;
    if (pl.route == BHWP_FRAMES_PER_FRAME || !f->frames) return pl;
    // frame rows of fy frames; as many workgroups as kFramesTargetWg asks for, each lane then applies its coefficient to G rows
    const uint64_t rows = (f->frames + pl.fy - 1) / pl.fy;
    // (a long window fills the chip alone: cutting its frames into groups would only compute each coefficient again per group)
    const uint64_t gy_target = pl.grid_x >= kFramesOnePassGx ? 1 : (kFramesTargetWg + pl.grid_x - 1) / pl.grid_x;
    uint64_t G = (rows + gy_target - 1) / gy_target;
    const uint64_t g_min = (rows + kFramesMaxGridY - 1) / kFramesMaxGridY;
    if (G < g_min) G = g_min;
    if (G < 1) G = 1;
    pl.group = G;
    pl.grid_y = (rows + G - 1) / G;
    return pl;
}

int bhwp_describe_frames(const bhw_params *p, const BhwCordicCfg *ct, const bhw_frames *f, char *buf, uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const BhwFramesPlan pl = bhwp_frames_plan(p, f, ct != nullptr);
    const uint64_t N = 1ull << p->phi_width;
    if (pl.route == BHWP_FRAMES_PER_FRAME) {
        char one[256];
        const int rc = bhw_describe_plan(p, 0, N, nullptr, one, sizeof one);
        if (rc) return rc;
        snprintf(buf, len, "per-frame: %llu x bhw_apply_device [%s]", (unsigned long long)f->frames, one);
        return BHW_OK;
    }
    frames_line("frames kernel: ", p, ct, f, pl, false, buf, len);
    return BHW_OK;
}

// ---- weighted overlap-add ----------------------------------------------------------------------------------------------------

int bhwp_ola_checks(const bhw_params *p, const bhw_ola *o, const void *d_y, const void *d_x, bool pointers, uint64_t length)
{
    if (!p) return bhwp_fail(BHW_ERR_BADARG, "params is NULL");
    int rc = bhwp_validate(p);
    if (rc) return rc;
    if (!o) return bhwp_fail(BHW_ERR_BADARG, "overlap-add descriptor is NULL");
    if (o->struct_size != sizeof(bhw_ola)) return bhwp_fail(BHW_ERR_BADARG, "bhw_ola.struct_size %u != %zu", o->struct_size, sizeof(bhw_ola));
    if (o->reserved) return bhwp_fail(BHW_ERR_BADARG, "bhw_ola.reserved must be 0");
    if (o->channels != 1 && o->channels != 2) return bhwp_fail(BHW_ERR_BADARG, "channels %u (1 or 2)", o->channels);
    if (o->hop == 0) return bhwp_fail(BHW_ERR_BADARG, "hop is 0");
    if (o->shift > 62) return bhwp_fail(BHW_ERR_BADARG, "shift %u > 62", o->shift);
    const uint64_t N = length ? length : 1ull << p->phi_width, NC = N * o->channels;
    if (o->y_stride && o->y_stride < NC)
        return bhwp_fail(BHW_ERR_BADARG, "y_stride %llu < N * channels = %llu", (unsigned long long)o->y_stride, (unsigned long long)NC);
    if (p->sin_type != BHW_SIN_CORDIC)
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "the Taylor sources (sin_type %u) have no per-coefficient form to sum frames with: generate the "
                         "window and form the sums in the caller", p->sin_type);
    if (!o->count) return BHW_OK;
    if (!o->frames) return bhwp_fail(BHW_ERR_BADARG, "frames is 0 with count %llu > 0", (unsigned long long)o->count);
    if (o->frames > (1ull << 34) / N)
        return bhwp_fail(BHW_ERR_BADARG, "frames * N = %llu * %llu > 2^34 per call", (unsigned long long)o->frames, (unsigned long long)N);
    // hop is a free 64-bit value: the extent is taken in 128 bits
    const unsigned __int128 ext = (unsigned __int128)(o->frames - 1) * o->hop + N;
    if (ext > (1ull << 34)) return bhwp_fail(BHW_ERR_BADARG, "extent (frames - 1) * hop + N above 2^34 per call");
    if (o->t0 > (uint64_t)ext || o->count > (uint64_t)ext - o->t0)
        return bhwp_fail(BHW_ERR_BADARG, "t0 + count = %llu + %llu beyond the extent (frames - 1) * hop + N = %llu", (unsigned long long)o->t0,
                         (unsigned long long)o->count, (unsigned long long)ext);
    if (!pointers) return BHW_OK;
    if (!d_y || !d_x) return bhwp_fail(BHW_ERR_BADARG, "d_y / d_x is NULL");
    // extents in int32 elements: the rows of d_y read, the outputs of d_x written
    const unsigned __int128 ye = (unsigned __int128)(o->frames - 1) * (o->y_stride ? o->y_stride : NC) + NC;
    if (ye > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "y extent beyond 2^60 elements");
    const uint64_t ya = (uint64_t)(uintptr_t)d_y, xa = (uint64_t)(uintptr_t)d_x, yb = (uint64_t)ye * 4u, xb = o->count * o->channels * 4u;
    if (ya > UINT64_MAX - yb || xa > UINT64_MAX - xb) return bhwp_fail(BHW_ERR_BADARG, "x or y range wraps the address space");
    if (xa < ya + yb && ya < xa + xb) return bhwp_fail(BHW_ERR_BADARG, "d_x must not overlap d_y");
    return BHW_OK;
}

BhwOlaPlan bhwp_ola_plan(const bhw_params *p, const bhw_ola *o, bool from_table, uint32_t force_q, uint32_t force_rx, uint64_t length,
                         uint32_t q_max, uint64_t batch)
{
    BhwOlaPlan pl{};
    const uint64_t N = length ? length : 1ull << p->phi_width;
    pl.len = N;
    pl.route = from_table ? BHWP_OLA_TABLE : BHWP_OLA_DIRECT;
    pl.y_stride = o->y_stride ? o->y_stride : N * o->channels;
    pl.q0 = o->t0 / o->hop;
    pl.r0 = o->t0 % o->hop;
    pl.jmax = o->hop >= N ? 1 : (N + o->hop - 1) / o->hop;
    if (!o->count) return pl;
    pl.lanes = o->hop < o->count ? o->hop : o->count;
    pl.rows = (o->count + o->hop - 1) / o->hop;
    // lanes along the residue first (consecutive outputs and frame elements in a wave); short hops put the rest of the workgroup
    // side by side over rows
    pl.rx = 1;
    while (pl.rx < kOlaBlock && pl.rx < pl.lanes) pl.rx *= 2;
    if (force_rx && force_rx <= kOlaBlock && (force_rx & (force_rx - 1)) == 0) pl.rx = force_rx;
    pl.fy = kOlaBlock / pl.rx;
    pl.grid_x = (pl.lanes + pl.rx - 1) / pl.rx;
    // Q: as many workgroups as kOlaTargetWg asks for (a wide residue range fills the chip alone), and at least the frames that reach
    // one output, so that a lane computes no more coefficients than it writes outputs
    const uint64_t row_groups = (pl.rows + pl.fy - 1) / pl.fy;
    const uint64_t gx = pl.grid_x * batch;                         // the signals of a batch share the target
    const uint64_t gy_target = gx >= kOlaOnePassGx ? 1 : (kOlaTargetWg + gx - 1) / gx;
    uint64_t Q = (row_groups + gy_target - 1) / gy_target;
    if (Q < pl.jmax) Q = pl.jmax;
    if (Q > row_groups) Q = row_groups;
    if (Q > q_max) Q = q_max;
    if (Q < 1) Q = 1;
    if (force_q >= 1 && force_q <= q_max) Q = force_q;
    pl.q = (uint32_t)Q;
    pl.row_blocks = (pl.rows + (uint64_t)pl.fy * pl.q - 1) / ((uint64_t)pl.fy * pl.q);
    pl.grid_y = pl.row_blocks < kOlaMaxGridY ? pl.row_blocks : kOlaMaxGridY;
    return pl;
}

int bhwp_describe_ola(const bhw_params *p, const BhwCordicCfg *ct, const bhw_ola *o, char *buf, uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    if (!o->count) {
        snprintf(buf, len, "overlap-add: nothing (count 0)");
        return BHW_OK;
    }
    ola_line(ct ? "overlap-add table: " : "overlap-add direct: ", p, ct, o, bhwp_ola_plan(p, o, ct != nullptr), false, buf, len);
    return BHW_OK;
}

// ---- windows of any length ------------------------------------------------------------------------------------------------------

int bhwp_len_checks(const bhw_params *p, uint64_t length)
{
    if (!p) return bhwp_fail(BHW_ERR_BADARG, "params is NULL");
    const int rc = bhwp_validate(p);
    if (rc) return rc;
    const uint64_t N = 1ull << p->phi_width;
    if (length == 0 || length > N)
        return bhwp_fail(BHW_ERR_BADARG, "length %llu outside 1..2^phi_width = %llu", (unsigned long long)length, (unsigned long long)N);
    if (p->sin_type != BHW_SIN_CORDIC)
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "windows of any length take the CORDIC source only (sin_type %u)", p->sin_type);
    return BHW_OK;
}

int bhwp_describe_len(const bhw_params *p, const BhwCordicCfg *ct, bool tiled, uint64_t length, bool force, uint64_t n0, uint64_t count,
                      const bhw_frames *f, const bhw_ola *o, char *buf, uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    if (f && o) return bhwp_fail(BHW_ERR_BADARG, "pass a frames or an overlap-add descriptor, not both");
    char inner[384];
    int rc = BHW_OK;
    if (!bhwp_len_kernels(p, length, force)) {
        if (f)       rc = bhwp_describe_frames(p, ct, f, inner, sizeof inner);
        else if (o)  rc = bhwp_describe_ola(p, ct, o, inner, sizeof inner);
        else if (ct) rc = bhwp_describe_from_table(p, *ct, tiled, n0, count, inner, sizeof inner);
        else         rc = bhw_describe_plan(p, n0, count, nullptr, inner, sizeof inner);
        if (rc) return rc;
        snprintf(buf, len, "power-of-two route (L = 2^%u): %s", p->phi_width, inner);
        return BHW_OK;
    }
    if (f) {
        frames_line("", p, ct, f, bhwp_frames_plan(p, f, ct != nullptr, -1, length), true, inner, sizeof inner);
    } else if (o) {
        if (!o->count) snprintf(inner, sizeof inner, "overlap-add: nothing (count 0)");
        else           ola_line("", p, ct, o, bhwp_ola_plan(p, o, ct != nullptr, 0, 0, length), true, inner, sizeof inner);
    } else {
        char kern[64];
        kernel_name(p, ct, "k_direct", "k_range", true, kern, sizeof kern);
        snprintf(inner, sizeof inner, "%s, %llu coefficients from n0 mod L = %llu", kern, (unsigned long long)count,
                 (unsigned long long)(n0 % length));
    }
    snprintf(buf, len, "any-length route (L = %llu, phi_width %u): %s", (unsigned long long)length, p->phi_width, inner);
    return BHW_OK;
}

// ---- float32 frame apply and overlap-add ----------------------------------------------------------------------------------------

int bhwp_f32_checks(const bhw_params *p, uint64_t length, uint32_t flags)
{
    const int rc = bhwp_len_checks(p, length);
    if (rc) return rc;
    if (flags & ~BHW_OLA_NORMALIZE) return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x (0 or BHW_OLA_NORMALIZE)", flags);
    return BHW_OK;
}

int bhwp_describe_f32(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, bool force, const bhw_frames *f, const bhw_ola *o,
                      uint32_t flags, char *buf, uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    if (!f == !o) return bhwp_fail(BHW_ERR_BADARG, "pass a frames or an overlap-add descriptor (one of them)");
    if (f && flags) return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x: the frames call takes none", flags);
    const bool any = bhwp_len_kernels(p, length, force);
    char win[64], inner[384];
    if (any) snprintf(win, sizeof win, "L = %llu", (unsigned long long)length);
    else     snprintf(win, sizeof win, "L = 2^%u", p->phi_width);
    const char *route = ct ? "table" : "direct";
    if (f) {
        frames_line("", p, ct, f, bhwp_frames_plan(p, f, ct != nullptr, -1, any ? length : 0, true), any, inner, sizeof inner,
                    "k_frames_f32_direct", "k_frames_f32_table");
        snprintf(buf, len, "f32 frames %s (%s): %s", route, win, inner);
        return BHW_OK;
    }
    const char *norm = (flags & BHW_OLA_NORMALIZE) ? "normalised by the window envelope" : "not normalised";
    if (!o->count) snprintf(inner, sizeof inner, "nothing (count 0)");
    else           ola_line("", p, ct, o, bhwp_ola_plan(p, o, ct != nullptr, 0, 0, any ? length : 0,
                                                 (flags & BHW_OLA_NORMALIZE) ? kOlaQMaxNorm : kOlaQMax), any, inner, sizeof inner,
                            "k_ola_f32_direct", "k_ola_f32_table");
    snprintf(buf, len, "f32 overlap-add %s (%s), %s: %s", route, win, norm, inner);
    return BHW_OK;
}

// ---- batched, centred STFT framing and overlap-add ---------------------------------------------------------------------------------

int bhwp_stft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, bool inverse, uint32_t flags, const void *d_x,
                     const void *d_y, bool pointers, bool welch)
{
    int rc = bhwp_f32_checks(p, length, flags);
    if (rc) return rc;
    if (!inverse && flags) return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x: the frames call takes none", flags);
    if (!s) return bhwp_fail(BHW_ERR_BADARG, "stft descriptor is NULL");
    if (s->struct_size != sizeof(bhw_stft)) return bhwp_fail(BHW_ERR_BADARG, "bhw_stft.struct_size %u != %zu", s->struct_size, sizeof(bhw_stft));
    if (s->channels != 1 && s->channels != 2) return bhwp_fail(BHW_ERR_BADARG, "channels %u (1 or 2)", s->channels);
    if (s->batch == 0) return bhwp_fail(BHW_ERR_BADARG, "batch is 0");
    if (s->hop == 0) return bhwp_fail(BHW_ERR_BADARG, "hop is 0");
    if (s->n_fft == 0 || s->n_fft > (1ull << 31)) return bhwp_fail(BHW_ERR_BADARG, "n_fft %llu outside 1..2^31", (unsigned long long)s->n_fft);
    if (s->shift > 62) return bhwp_fail(BHW_ERR_BADARG, "shift %u > 62", s->shift);
    if (s->col0 > s->n_fft || length > s->n_fft - s->col0)
        return bhwp_fail(BHW_ERR_BADARG, "col0 + L = %llu + %llu > n_fft = %llu", (unsigned long long)s->col0, (unsigned long long)length,
                         (unsigned long long)s->n_fft);
    if (s->pad > (1ull << 40)) return bhwp_fail(BHW_ERR_BADARG, "pad %llu above 2^40", (unsigned long long)s->pad);
    if (inverse ? s->pad_mode != 0 : (s->pad_mode != BHW_PAD_CONSTANT && s->pad_mode != BHW_PAD_REFLECT))
        return bhwp_fail(BHW_ERR_BADARG, inverse ? "pad_mode %u: the overlap-add takes 0" : "pad_mode %u (BHW_PAD_CONSTANT or BHW_PAD_REFLECT)",
                         s->pad_mode);
    const uint64_t T = s->samples, C = s->channels, F = s->frames, NC = s->n_fft * C;
    if (inverse) {
        if (!T) return BHW_OK;
        if (!F) return bhwp_fail(BHW_ERR_BADARG, "frames is 0 with samples %llu > 0", (unsigned long long)T);
        if (s->pad < s->col0)
            return bhwp_fail(BHW_ERR_BADARG, "pad %llu < col0 %llu: the first outputs have no window under them", (unsigned long long)s->pad,
                             (unsigned long long)s->col0);
        if (T > (1ull << 34)) return bhwp_fail(BHW_ERR_BADARG, "samples %llu above 2^34 per signal", (unsigned long long)T);
    } else {
        if (!F) return BHW_OK;
        if (!T) return bhwp_fail(BHW_ERR_BADARG, "samples is 0 with frames %llu > 0", (unsigned long long)F);
        // every frame inside the padded signal; hop is a free 64-bit value, so the products are taken in 128 bits
        // (a Welch segment reads its L window columns only: the columns up to n_fft are the zero padding at its end)
        if (welch && (unsigned __int128)(F - 1) * s->hop + length > (unsigned __int128)T + 2 * s->pad)
            return bhwp_fail(BHW_ERR_BADARG, "(frames - 1) * hop + L > samples: segment %llu leaves the signal", (unsigned long long)(F - 1));
        if (!welch && (unsigned __int128)(F - 1) * s->hop + s->n_fft > (unsigned __int128)T + 2 * s->pad)
            return bhwp_fail(BHW_ERR_BADARG, "(frames - 1) * hop + n_fft > samples + 2 * pad: frame %llu leaves the padded signal",
                             (unsigned long long)(F - 1));
        if (s->pad_mode == BHW_PAD_REFLECT && s->pad > T - 1)
            return bhwp_fail(BHW_ERR_BADARG, "reflect padding needs pad %llu <= samples - 1 = %llu", (unsigned long long)s->pad,
                             (unsigned long long)(T - 1));
    }
    if ((unsigned __int128)s->batch * F * s->n_fft > (1ull << 34))
        return bhwp_fail(BHW_ERR_BADARG, "batch * frames * n_fft above 2^34 per call");
    if ((unsigned __int128)T * C > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "samples * channels beyond 2^60 elements");
    if (s->x_stride && s->x_stride < T * C)
        return bhwp_fail(BHW_ERR_BADARG, "x_stride %llu < samples * channels = %llu: signals overlap", (unsigned long long)s->x_stride,
                         (unsigned long long)(T * C));
    if (s->y_stride && s->y_stride < NC)
        return bhwp_fail(BHW_ERR_BADARG, "y_stride %llu < n_fft * channels = %llu: rows overlap", (unsigned long long)s->y_stride,
                         (unsigned long long)NC);
    const uint64_t ys = s->y_stride ? s->y_stride : NC;
    const unsigned __int128 ysig = (unsigned __int128)(F - 1) * ys + NC;           // the rows of one signal
    if (ysig > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "y extent beyond 2^60 elements");
    if (s->y_batch_stride && s->y_batch_stride < (uint64_t)ysig)
        return bhwp_fail(BHW_ERR_BADARG, "y_batch_stride %llu < (frames - 1) * y_stride + n_fft * channels = %llu: signals overlap",
                         (unsigned long long)s->y_batch_stride, (unsigned long long)ysig);
    if (!pointers) return BHW_OK;
    if (!d_x || !d_y) return bhwp_fail(BHW_ERR_BADARG, "d_x / d_y is NULL");
    const uint64_t xs = s->x_stride ? s->x_stride : T * C, ybs = s->y_batch_stride ? s->y_batch_stride : F * ys;
    const unsigned __int128 xe = (unsigned __int128)(s->batch - 1) * xs + T * C, ye = (unsigned __int128)(s->batch - 1) * ybs + ysig;
    if (xe > (1ull << 60) || ye > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "x or y extent beyond 2^60 elements");
    const uint64_t xa = (uint64_t)(uintptr_t)d_x, ya = (uint64_t)(uintptr_t)d_y, xb = (uint64_t)xe * 4u, yb = (uint64_t)ye * 4u;
    if (xa > UINT64_MAX - xb || ya > UINT64_MAX - yb) return bhwp_fail(BHW_ERR_BADARG, "x or y range wraps the address space");
    if (xa < ya + yb && ya < xa + xb) return bhwp_fail(BHW_ERR_BADARG, "d_x and d_y overlap");
    return BHW_OK;
}

BhwStftPlan bhwp_stft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, bool from_table)
{
    (void)p;
    BhwStftPlan pl{};
    const uint64_t C = s->channels;
    pl.route = from_table ? BHWP_FRAMES_TABLE : BHWP_FRAMES_DIRECT;
    pl.len = length;
    pl.x_stride = s->x_stride ? s->x_stride : s->samples * C;
    pl.y_stride = s->y_stride ? s->y_stride : s->n_fft * C;
    pl.y_bstride = s->y_batch_stride ? s->y_batch_stride : s->frames * pl.y_stride;
    pl.kx = 1;
    while (pl.kx < kFramesBlock && pl.kx < s->n_fft) pl.kx *= 2;
    pl.fy = kFramesBlock / pl.kx;
    pl.grid_x = (s->n_fft + pl.kx - 1) / pl.kx;
    pl.rows = s->batch * s->frames;
    if (!pl.rows) return pl;
    pl.step_b = pl.fy / s->frames;
    pl.step_f = pl.fy % s->frames;
    // as bhwp_frames_plan, over the row pool of the whole batch: a lane applies its coefficient to G rows of any signals
    const uint64_t groups = (pl.rows + pl.fy - 1) / pl.fy;
    const uint64_t gy_target = pl.grid_x >= kFramesOnePassGx ? 1 : (kFramesTargetWg + pl.grid_x - 1) / pl.grid_x;
    const uint64_t G = (groups + gy_target - 1) / gy_target;
    pl.group = G < 1 ? 1 : G;
    pl.row_blocks = (groups + pl.group - 1) / pl.group;
    pl.grid_y = pl.row_blocks < kFramesMaxGridY ? pl.row_blocks : kFramesMaxGridY;
    return pl;
}

void bhwp_stft_ola(const bhw_stft *s, bhw_ola &o, BhwOlaBatch &bt)
{
    memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.channels = s->channels;
    o.frames = s->frames;
    o.hop = s->hop;
    o.y_stride = s->y_stride ? s->y_stride : s->n_fft * s->channels;
    o.t0 = s->pad - s->col0;                                       // output t of the signal is window-start time t + pad - col0
    o.count = s->samples;
    o.shift = s->shift;
    bt.batch = s->batch;
    bt.y_bstride = s->y_batch_stride ? s->y_batch_stride : s->frames * o.y_stride;
    bt.x_bstride = s->x_stride ? s->x_stride : s->samples * s->channels;
}

int bhwp_describe_stft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, bool inverse, uint32_t flags,
                       char *buf, uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const char *route = ct ? "table" : "direct";
    char kern[64];
    const char *pad = s->pad_mode == BHW_PAD_REFLECT ? "reflect" : "constant";
    if (!inverse) {
        if (!s->frames) {
            snprintf(buf, len, "stft frames %s (L = %llu): nothing (frames 0)", route, (unsigned long long)length);
            return BHW_OK;
        }
        const BhwStftPlan pl = bhwp_stft_plan(p, length, s, ct != nullptr);
        kernel_name(p, ct, "k_stft_frames_direct", "k_stft_frames_table", false, kern, sizeof kern);
        snprintf(buf, len, "stft frames %s (L = %llu, n_fft %llu, col0 %llu, pad %llu %s): %s, %u channel%s, %llu signals x %llu frames = "
                 "%llu rows, G = %llu rows per lane, grid %llu x %llu x %u lanes (%u along the row)", route, (unsigned long long)length,
                 (unsigned long long)s->n_fft, (unsigned long long)s->col0, (unsigned long long)s->pad, pad, kern, s->channels,
                 s->channels == 2 ? "s" : "", (unsigned long long)s->batch, (unsigned long long)s->frames, (unsigned long long)pl.rows,
                 (unsigned long long)pl.group, (unsigned long long)pl.grid_x, (unsigned long long)pl.grid_y, kFramesBlock, pl.kx);
        return BHW_OK;
    }
    const char *norm = (flags & BHW_OLA_NORMALIZE) ? "normalised by the window envelope" : "not normalised";
    if (!s->samples) {
        snprintf(buf, len, "istft overlap-add %s (L = %llu), %s: nothing (samples 0)", route, (unsigned long long)length, norm);
        return BHW_OK;
    }
    bhw_ola o;
    BhwOlaBatch bt;
    bhwp_stft_ola(s, o, bt);
    const bool nm = (flags & BHW_OLA_NORMALIZE) != 0;
    const bool any = bhwp_len_kernels(p, length, false);           // the overlap-add takes the power-of-two kernels at L = 2^phi_width
    const BhwOlaPlan pl = bhwp_ola_plan(p, &o, ct != nullptr, 0, 0, any ? length : 0, nm ? kOlaQMaxNorm : kOlaQMax, bt.batch);
    char inner[384];
    ola_line("", p, ct, &o, pl, any, inner, sizeof inner, "k_ola_f32_direct", "k_ola_f32_table");
    const uint64_t gz = bt.batch < kOlaMaxGridZ ? bt.batch : kOlaMaxGridZ;
    snprintf(buf, len, "istft overlap-add %s (L = %llu, n_fft %llu, col0 %llu, pad %llu: t0 = %llu), %s, %llu signals (grid z %llu): %s", route,
             (unsigned long long)length, (unsigned long long)s->n_fft, (unsigned long long)s->col0, (unsigned long long)s->pad,
             (unsigned long long)o.t0, norm, (unsigned long long)bt.batch, (unsigned long long)gz, inner);
    return BHW_OK;
}

// ---- Welch's method: window sums, detrended segments, averaged periodogram ----------------------------------------------------------

int bhwp_sums_checks(const bhw_params *p, uint64_t length, uint32_t flags, const void *d_sums, bool pointers)
{
    const int rc = bhwp_len_checks(p, length);
    if (rc) return rc;
    if (flags & ~BHW_SUMS_F32) return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x (0 or BHW_SUMS_F32)", flags);
    if (!pointers) return BHW_OK;
    if (!d_sums) return bhwp_fail(BHW_ERR_BADARG, "d_sums is NULL");
    if ((uintptr_t)d_sums % 8) return bhwp_fail(BHW_ERR_BADARG, "d_sums is not 8-byte aligned");
    return BHW_OK;
}

BhwSumsPlan bhwp_sums_plan(uint64_t length)
{
    BhwSumsPlan pl{};
    pl.len = length;
    const uint64_t per_wg = (uint64_t)kSumsBlock * kSumsPerLane;
    const uint64_t g = (length + per_wg - 1) / per_wg;
    pl.grid = (uint32_t)(g < 1 ? 1 : g > kSumsMaxGrid ? kSumsMaxGrid : g);
    const uint64_t lanes = (uint64_t)pl.grid * kSumsBlock;
    pl.trips = (uint32_t)((length + lanes - 1) / lanes);
    return pl;
}

uint64_t bhwp_welch_workspace_bytes(const bhw_stft *s, uint32_t flags)
{
    if (!s || !(flags & BHW_WELCH_DETREND_CONSTANT)) return 0;
    const unsigned __int128 n = (unsigned __int128)s->batch * s->frames * s->channels * 4u;
    return n > (1ull << 62) ? 0 : (uint64_t)n;
}

int bhwp_welch_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_x, const void *d_y,
                      const void *workspace, uint64_t workspace_bytes, bool pointers)
{
    int rc = bhwp_f32_checks(p, length, 0);
    if (rc) return rc;
    if (flags & ~BHW_WELCH_DETREND_CONSTANT) return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x (0 or BHW_WELCH_DETREND_CONSTANT)", flags);
    rc = bhwp_stft_checks(p, length, s, false, 0, d_x, d_y, pointers, true);
    if (rc) return rc;
    if (s->pad) return bhwp_fail(BHW_ERR_BADARG, "pad %llu: Welch segments take no padding", (unsigned long long)s->pad);
    if (s->col0) return bhwp_fail(BHW_ERR_BADARG, "col0 %llu: Welch segments are zero-padded at the end (col0 0)", (unsigned long long)s->col0);
    if (s->pad_mode) return bhwp_fail(BHW_ERR_BADARG, "pad_mode %u: Welch segments take 0", s->pad_mode);
    if (!pointers || !s->frames || !(flags & BHW_WELCH_DETREND_CONSTANT)) return BHW_OK;
    const uint64_t need = bhwp_welch_workspace_bytes(s, flags);
    if (!workspace) return bhwp_fail(BHW_ERR_BADARG, "workspace is NULL: detrending needs %llu bytes", (unsigned long long)need);
    if ((uintptr_t)workspace % 4) return bhwp_fail(BHW_ERR_BADARG, "workspace is not 4-byte aligned");
    if (workspace_bytes < need)
        return bhwp_fail(BHW_ERR_WORKSPACE, "workspace of %llu bytes, detrending needs %llu", (unsigned long long)workspace_bytes,
                         (unsigned long long)need);
    // the extents bhwp_stft_checks has bounded (2^60 elements each, no wrap)
    const uint64_t T = s->samples, C = s->channels, F = s->frames, NC = s->n_fft * C;
    const uint64_t xs = s->x_stride ? s->x_stride : T * C, ys = s->y_stride ? s->y_stride : NC;
    const uint64_t ybs = s->y_batch_stride ? s->y_batch_stride : F * ys;
    const uint64_t xb = ((s->batch - 1) * xs + T * C) * 4u, yb = ((s->batch - 1) * ybs + (F - 1) * ys + NC) * 4u;
    const uint64_t xa = (uint64_t)(uintptr_t)d_x, ya = (uint64_t)(uintptr_t)d_y, wa = (uint64_t)(uintptr_t)workspace;
    if (wa > UINT64_MAX - need) return bhwp_fail(BHW_ERR_BADARG, "workspace range wraps the address space");
    if ((wa < xa + xb && xa < wa + need) || (wa < ya + yb && ya < wa + need))
        return bhwp_fail(BHW_ERR_BADARG, "workspace overlaps d_x or d_y");
    return BHW_OK;
}

BhwWelchPlan bhwp_welch_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table)
{
    BhwWelchPlan pl{};
    pl.frames = bhwp_stft_plan(p, length, s, from_table);
    pl.detrend = (flags & BHW_WELCH_DETREND_CONSTANT) != 0;
    if (pl.detrend && pl.frames.rows) {
        const uint64_t per_wg = kWelchMeanBlock / 64u;
        const uint64_t wg = (pl.frames.rows + per_wg - 1) / per_wg;
        pl.mean_grid = wg < kWelchMeanMaxGrid ? wg : kWelchMeanMaxGrid;
        pl.ws_bytes = bhwp_welch_workspace_bytes(s, flags);
    }
    return pl;
}

BhwPsdPlan bhwp_psd_plan(const bhw_psd *d)
{
    BhwPsdPlan pl{};
    pl.blocks = (d->frames + BHW_WELCH_BLOCK - 1) / BHW_WELCH_BLOCK;
    pl.tiles = (d->bins + kPsdLanes - 1) / kPsdLanes;
    pl.grid = d->batch * pl.blocks * pl.tiles;
    pl.unroll = pl.grid <= kPsdSmallGrid ? kPsdUnrollMax : kPsdUnrollMin;
    pl.y_stride = d->y_stride ? d->y_stride : d->bins;
    pl.y_bstride = d->y_batch_stride ? d->y_batch_stride : d->frames * pl.y_stride;
    pl.p_stride = d->p_stride ? d->p_stride : d->bins;
    if (pl.blocks > 1) {
        pl.join_grid = (d->batch * d->bins + 255u) / 256u;
        pl.ws_bytes = d->batch * pl.blocks * d->bins * 8u;
    }
    return pl;
}

int bhwp_psd_checks(const bhw_psd *d, const void *d_Y, const void *d_P, const void *workspace, uint64_t workspace_bytes, bool pointers)
{
    if (!d) return bhwp_fail(BHW_ERR_BADARG, "psd descriptor is NULL");
    if (d->struct_size != sizeof(bhw_psd)) return bhwp_fail(BHW_ERR_BADARG, "bhw_psd.struct_size %u != %zu", d->struct_size, sizeof(bhw_psd));
    if (d->flags & ~BHW_PSD_ONESIDED) return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x (0 or BHW_PSD_ONESIDED)", d->flags);
    if (!d->batch || !d->frames || !d->bins) return bhwp_fail(BHW_ERR_BADARG, "batch, frames or bins is 0");
    if (!d->n_fft || d->n_fft > (1ull << 31)) return bhwp_fail(BHW_ERR_BADARG, "n_fft %llu outside 1..2^31", (unsigned long long)d->n_fft);
    if (d->bins > d->n_fft) return bhwp_fail(BHW_ERR_BADARG, "bins %llu above n_fft %llu", (unsigned long long)d->bins, (unsigned long long)d->n_fft);
    if ((d->flags & BHW_PSD_ONESIDED) && d->bins != d->n_fft / 2 + 1)
        return bhwp_fail(BHW_ERR_BADARG, "BHW_PSD_ONESIDED needs bins = n_fft / 2 + 1 = %llu, got %llu", (unsigned long long)(d->n_fft / 2 + 1),
                         (unsigned long long)d->bins);
    if (!(d->scale - d->scale == 0.0)) return bhwp_fail(BHW_ERR_BADARG, "scale is not finite");
    const uint64_t K = d->bins, F = d->frames;
    if ((unsigned __int128)d->batch * F * K > (1ull << 34)) return bhwp_fail(BHW_ERR_BADARG, "batch * frames * bins above 2^34 per call");
    if (d->y_stride && d->y_stride < K)
        return bhwp_fail(BHW_ERR_BADARG, "y_stride %llu < bins %llu: rows overlap", (unsigned long long)d->y_stride, (unsigned long long)K);
    const uint64_t ys = d->y_stride ? d->y_stride : K;
    const unsigned __int128 ysig = (unsigned __int128)(F - 1) * ys + K;
    if (ysig > (1ull << 58)) return bhwp_fail(BHW_ERR_BADARG, "Y extent beyond 2^58 elements");
    if (d->y_batch_stride && d->y_batch_stride < (uint64_t)ysig)
        return bhwp_fail(BHW_ERR_BADARG, "y_batch_stride %llu < (frames - 1) * y_stride + bins = %llu: signals overlap",
                         (unsigned long long)d->y_batch_stride, (unsigned long long)ysig);
    if (d->p_stride && d->p_stride < K)
        return bhwp_fail(BHW_ERR_BADARG, "p_stride %llu < bins %llu: rows overlap", (unsigned long long)d->p_stride, (unsigned long long)K);
    const uint64_t ybs = d->y_batch_stride ? d->y_batch_stride : F * ys, ps = d->p_stride ? d->p_stride : K;
    const unsigned __int128 ye = (unsigned __int128)(d->batch - 1) * ybs + ysig, pe = (unsigned __int128)(d->batch - 1) * ps + K;
    if (ye > (1ull << 58) || pe > (1ull << 58)) return bhwp_fail(BHW_ERR_BADARG, "Y or P extent beyond 2^58 elements");
    const uint64_t blocks = (F + BHW_WELCH_BLOCK - 1) / BHW_WELCH_BLOCK, tiles = (K + kPsdLanes - 1) / kPsdLanes;
    if ((unsigned __int128)d->batch * blocks * tiles > 0x7FFFFFFFull)
        return bhwp_fail(BHW_ERR_BADARG, "batch * ceil(frames / %u) * ceil(bins / %u) above 2^31 - 1 workgroups", BHW_WELCH_BLOCK, kPsdLanes);
    if (!pointers) return BHW_OK;
    if (!d_Y || !d_P) return bhwp_fail(BHW_ERR_BADARG, "d_Y / d_P is NULL");
    if ((uintptr_t)d_Y % 8) return bhwp_fail(BHW_ERR_BADARG, "d_Y is not 8-byte aligned");
    if ((uintptr_t)d_P % 4) return bhwp_fail(BHW_ERR_BADARG, "d_P is not 4-byte aligned");
    const uint64_t Ya = (uint64_t)(uintptr_t)d_Y, Pa = (uint64_t)(uintptr_t)d_P, Yb = (uint64_t)ye * 8u, Pb = (uint64_t)pe * 4u;
    if (Ya > UINT64_MAX - Yb || Pa > UINT64_MAX - Pb) return bhwp_fail(BHW_ERR_BADARG, "Y or P range wraps the address space");
    if (Ya < Pa + Pb && Pa < Ya + Yb) return bhwp_fail(BHW_ERR_BADARG, "d_Y and d_P overlap");
    if (blocks > 1) {
        const uint64_t need = d->batch * blocks * K * 8u;                       // below 2^34 / 256 * 8 + ... : no overflow
        if (!workspace) return bhwp_fail(BHW_ERR_BADARG, "workspace is NULL: %llu frame blocks need %llu bytes", (unsigned long long)blocks,
                                         (unsigned long long)need);
        if ((uintptr_t)workspace % 8) return bhwp_fail(BHW_ERR_BADARG, "workspace is not 8-byte aligned");
        if (workspace_bytes < need)
            return bhwp_fail(BHW_ERR_WORKSPACE, "workspace of %llu bytes, the block sums need %llu", (unsigned long long)workspace_bytes,
                             (unsigned long long)need);
        const uint64_t Wa = (uint64_t)(uintptr_t)workspace;
        if (Wa > UINT64_MAX - need) return bhwp_fail(BHW_ERR_BADARG, "workspace range wraps the address space");
        if ((Wa < Ya + Yb && Ya < Wa + need) || (Wa < Pa + Pb && Pa < Wa + need))
            return bhwp_fail(BHW_ERR_BADARG, "workspace overlaps d_Y or d_P");
    }
    return BHW_OK;
}

int bhwp_describe_welch(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_psd *d,
                        char *buf, uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    if (d) {
        const BhwPsdPlan pl = bhwp_psd_plan(d);
        snprintf(buf, len, "welch psd (%s, n_fft %llu): k_welch_psd<%d,%u>, %llu signals x %llu frames x %llu bins, %llu block%s of %u frames, "
                 "grid %llu x %u lanes (%u along the bins x %u waves of %u frames a pass)%s, workspace %llu bytes", (d->flags & BHW_PSD_ONESIDED) ? "one-sided" : "two-sided",
                 (unsigned long long)d->n_fft, pl.blocks > 1 ? 1 : 0, pl.unroll, (unsigned long long)d->batch, (unsigned long long)d->frames,
                 (unsigned long long)d->bins, (unsigned long long)pl.blocks, pl.blocks == 1 ? "" : "s", BHW_WELCH_BLOCK,
                 (unsigned long long)pl.grid, kPsdLanes * kPsdWaves, kPsdLanes, kPsdWaves, pl.unroll, pl.blocks > 1 ? ", then k_welch_psd_join in block order" : "",
                 (unsigned long long)pl.ws_bytes);
        return BHW_OK;
    }
    const char *route = ct ? "table" : "direct";
    char kern[64];
    if (!s) {
        const BhwSumsPlan pl = bhwp_sums_plan(length);
        kernel_name(p, ct, "k_window_sums_direct", "k_window_sums_table", false, kern, sizeof kern);
        snprintf(buf, len, "window sums %s (L = %llu, %s): memset of 4 words, then %s, grid %u x %u lanes, %u coefficient%s per lane, "
                 "3 integer atomics per workgroup", route, (unsigned long long)length, (flags & BHW_SUMS_F32) ? "u = fl32(w)" : "u = w", kern,
                 pl.grid, kSumsBlock, pl.trips, pl.trips == 1 ? "" : "s");
        return BHW_OK;
    }
    if (!(flags & BHW_WELCH_DETREND_CONSTANT)) {
        char inner[512];
        const int rc = bhwp_describe_stft(p, ct, length, s, false, 0, inner, sizeof inner);
        if (rc) return rc;
        snprintf(buf, len, "welch segments %s, no detrending: %s", route, inner);
        return BHW_OK;
    }
    if (!s->frames) {
        snprintf(buf, len, "welch segments %s (L = %llu): nothing (frames 0)", route, (unsigned long long)length);
        return BHW_OK;
    }
    const BhwWelchPlan pl = bhwp_welch_plan(p, length, s, flags, ct != nullptr);
    kernel_name(p, ct, "k_welch_frames_direct", "k_welch_frames_table", false, kern, sizeof kern);
    snprintf(buf, len, "welch segments %s (L = %llu, n_fft %llu), constant detrend: mean pass %s (one wave per row, grid %llu x %u "
             "lanes, workspace %llu bytes), then %s, %u channel%s, %llu signals x %llu frames = %llu rows, G = %llu rows per lane, "
             "grid %llu x %llu x %u lanes (%u along the row)", route, (unsigned long long)length, (unsigned long long)s->n_fft,
             s->channels == 1 ? "k_welch_mean<0>" : "k_welch_mean<2> (<1> where the pairs are not 8-byte aligned)",
             (unsigned long long)pl.mean_grid, kWelchMeanBlock, (unsigned long long)pl.ws_bytes, kern, s->channels, s->channels == 2 ? "s" : "",
             (unsigned long long)s->batch, (unsigned long long)s->frames, (unsigned long long)pl.frames.rows,
             (unsigned long long)pl.frames.group, (unsigned long long)pl.frames.grid_x, (unsigned long long)pl.frames.grid_y, kFramesBlock,
             pl.frames.kx);
    return BHW_OK;
}

// ---- cross spectra -----------------------------------------------------------------------------------------------------------------------
BhwCsdPlan bhwp_csd_plan(const bhw_csd *d)
{
    BhwCsdPlan pl{};
    pl.blocks = (d->frames + BHW_WELCH_BLOCK - 1) / BHW_WELCH_BLOCK;
    pl.tiles = (d->bins + kPsdLanes - 1) / kPsdLanes;
    pl.grid = d->batch * pl.blocks * pl.tiles;
    pl.chains = (d->flags & kCsdOutputMask) == BHW_CSD_PXY ? 2u : 4u;
    pl.unroll = kCsdPassBytes / (kPsdWaves * kPsdLanes * pl.chains * 8u);
    pl.lds_bytes = kPsdWaves * pl.unroll * kPsdLanes * pl.chains * 8u;
    pl.x_stride = d->x_stride ? d->x_stride : d->bins;
    pl.x_bstride = (d->flags & BHW_CSD_BROADCAST_X) ? 0 : d->x_batch_stride ? d->x_batch_stride : d->frames * pl.x_stride;
    pl.y_stride = d->y_stride ? d->y_stride : d->bins;
    pl.y_bstride = d->y_batch_stride ? d->y_batch_stride : d->frames * pl.y_stride;
    pl.o_stride = d->o_stride ? d->o_stride : d->bins;
    if (pl.blocks > 1) {
        pl.join_grid = (d->batch * d->bins + 255u) / 256u;
        pl.ws_bytes = d->batch * pl.blocks * d->bins * pl.chains * 8u;
    }
    return pl;
}

// one operand's strides: rows and signals apart; *ext = its extent in complex elements
static int csd_operand(const char *name, uint64_t B, uint64_t F, uint64_t K, uint64_t stride, uint64_t bstride, uint64_t *ext)
{
    if (stride && stride < K)
        return bhwp_fail(BHW_ERR_BADARG, "%s_stride %llu < bins %llu: rows overlap", name, (unsigned long long)stride, (unsigned long long)K);
    const uint64_t s = stride ? stride : K;
    const unsigned __int128 sig = (unsigned __int128)(F - 1) * s + K;
    if (sig > (1ull << 58)) return bhwp_fail(BHW_ERR_BADARG, "%s extent beyond 2^58 elements", name);
    if (bstride && bstride < (uint64_t)sig)
        return bhwp_fail(BHW_ERR_BADARG, "%s_batch_stride %llu < (frames - 1) * %s_stride + bins = %llu: signals overlap", name,
                         (unsigned long long)bstride, name, (unsigned long long)sig);
    const uint64_t bs = bstride ? bstride : F * s;
    const unsigned __int128 e = (unsigned __int128)(B - 1) * bs + sig;
    if (e > (1ull << 58)) return bhwp_fail(BHW_ERR_BADARG, "%s extent beyond 2^58 elements", name);
    *ext = (uint64_t)e;
    return BHW_OK;
}

// The byte ranges a cross-spectra call touches (bhwp_csd_checks, bhwp_csd_fft_checks): the two operands first, then the requested
// outputs, then the workspace.
struct CsdRanges {
    uint64_t lo[kCsdOutputs + 3], nb[kCsdOutputs + 3];
    const char *what[kCsdOutputs + 3];
    uint32_t n = 0;
    void add(uint64_t a, uint64_t bytes, const char *name) { lo[n] = a, nb[n] = bytes, what[n++] = name; }
};

// the requested outputs of the mask: each present and aligned to its element; oe = the extent of an output in elements
static int csd_output_ranges(uint32_t flags, const void *const *outs, uint64_t oe, CsdRanges &r)
{
    static const char *const names[kCsdOutputs] = {"d_Pxy", "d_Pxx", "d_Pyy", "d_Cxy", "d_H1"};
    static const uint32_t bits[kCsdOutputs] = {BHW_CSD_PXY, BHW_CSD_PXX, BHW_CSD_PYY, BHW_CSD_COHERENCE, BHW_CSD_H1};
    static const uint32_t width[kCsdOutputs] = {8, 4, 4, 4, 8};
    for (uint32_t i = 0; i < kCsdOutputs; ++i) {
        if (!(flags & bits[i])) continue;
        const void *o = outs ? outs[i] : nullptr;
        if (!o) return bhwp_fail(BHW_ERR_BADARG, "%s is NULL and its output is requested", names[i]);
        if ((uintptr_t)o % width[i]) return bhwp_fail(BHW_ERR_BADARG, "%s is not %u-byte aligned", names[i], width[i]);
        r.add((uint64_t)(uintptr_t)o, oe * width[i], names[i]);
    }
    return BHW_OK;
}

// no range wraps; nothing written overlaps anything (the two operands are only read: they may coincide)
static int csd_overlaps(const CsdRanges &r, bool has_ws)
{
    for (uint32_t i = 0; i < r.n; ++i)
        if (r.lo[i] > UINT64_MAX - r.nb[i]) return bhwp_fail(BHW_ERR_BADARG, "%s range wraps the address space", r.what[i]);
    for (uint32_t i = 2; i < r.n; ++i)
        for (uint32_t j = 0; j < i; ++j)
            if (r.lo[i] < r.lo[j] + r.nb[j] && r.lo[j] < r.lo[i] + r.nb[i]) {
                if (i == r.n - 1 && has_ws) return bhwp_fail(BHW_ERR_BADARG, "workspace overlaps %s", r.what[j]);
                return bhwp_fail(BHW_ERR_BADARG, "%s and %s overlap", r.what[j], r.what[i]);
            }
    return BHW_OK;
}

int bhwp_csd_checks(const bhw_csd *d, const void *d_X, const void *d_Y, const void *const *outs, const void *workspace,
                    uint64_t workspace_bytes, bool pointers)
{
    if (!d) return bhwp_fail(BHW_ERR_BADARG, "csd descriptor is NULL");
    if (d->struct_size != sizeof(bhw_csd)) return bhwp_fail(BHW_ERR_BADARG, "bhw_csd.struct_size %u != %zu", d->struct_size, sizeof(bhw_csd));
    if (d->reserved) return bhwp_fail(BHW_ERR_BADARG, "bhw_csd.reserved is not 0");
    if (d->flags & ~(BHW_CSD_ONESIDED | BHW_CSD_BROADCAST_X | kCsdOutputMask))
        return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x (BHW_CSD_ONESIDED, BHW_CSD_BROADCAST_X and the output mask 0x%x)", d->flags, kCsdOutputMask);
    if (!(d->flags & kCsdOutputMask)) return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x: the output mask is empty", d->flags);
    if (!d->batch || !d->frames || !d->bins) return bhwp_fail(BHW_ERR_BADARG, "batch, frames or bins is 0");
    if (!d->n_fft || d->n_fft > (1ull << 31)) return bhwp_fail(BHW_ERR_BADARG, "n_fft %llu outside 1..2^31", (unsigned long long)d->n_fft);
    if (d->bins > d->n_fft) return bhwp_fail(BHW_ERR_BADARG, "bins %llu above n_fft %llu", (unsigned long long)d->bins, (unsigned long long)d->n_fft);
    if ((d->flags & BHW_CSD_ONESIDED) && d->bins != d->n_fft / 2 + 1)
        return bhwp_fail(BHW_ERR_BADARG, "BHW_CSD_ONESIDED needs bins = n_fft / 2 + 1 = %llu, got %llu", (unsigned long long)(d->n_fft / 2 + 1),
                         (unsigned long long)d->bins);
    if (!(d->scale - d->scale == 0.0)) return bhwp_fail(BHW_ERR_BADARG, "scale is not finite");
    const uint64_t K = d->bins, F = d->frames, B = d->batch;
    const bool bcast = (d->flags & BHW_CSD_BROADCAST_X) != 0;
    if ((unsigned __int128)B * F * K > (1ull << 34)) return bhwp_fail(BHW_ERR_BADARG, "batch * frames * bins above 2^34 per call");
    if (bcast && d->x_batch_stride)
        return bhwp_fail(BHW_ERR_BADARG, "x_batch_stride %llu under BHW_CSD_BROADCAST_X: X is one signal", (unsigned long long)d->x_batch_stride);
    uint64_t xe, ye;
    if (int rc = csd_operand("x", bcast ? 1 : B, F, K, d->x_stride, d->x_batch_stride, &xe)) return rc;
    if (int rc = csd_operand("y", B, F, K, d->y_stride, d->y_batch_stride, &ye)) return rc;
    if (d->o_stride && d->o_stride < K)
        return bhwp_fail(BHW_ERR_BADARG, "o_stride %llu < bins %llu: rows overlap", (unsigned long long)d->o_stride, (unsigned long long)K);
    const unsigned __int128 oe = (unsigned __int128)(B - 1) * (d->o_stride ? d->o_stride : K) + K;
    if (oe > (1ull << 58)) return bhwp_fail(BHW_ERR_BADARG, "output extent beyond 2^58 elements");
    const uint64_t blocks = (F + BHW_WELCH_BLOCK - 1) / BHW_WELCH_BLOCK, tiles = (K + kPsdLanes - 1) / kPsdLanes;
    if ((unsigned __int128)B * blocks * tiles > 0x7FFFFFFFull)
        return bhwp_fail(BHW_ERR_BADARG, "batch * ceil(frames / %u) * ceil(bins / %u) above 2^31 - 1 workgroups", BHW_WELCH_BLOCK, kPsdLanes);
    if (!pointers) return BHW_OK;
    if (!d_X || !d_Y) return bhwp_fail(BHW_ERR_BADARG, "d_X / d_Y is NULL");
    if ((uintptr_t)d_X % 8 || (uintptr_t)d_Y % 8) return bhwp_fail(BHW_ERR_BADARG, "d_X / d_Y is not 8-byte aligned");
    // the byte ranges the call touches: X, Y, the requested outputs, the workspace
    CsdRanges r;
    r.add((uint64_t)(uintptr_t)d_X, xe * 8u, "d_X");
    r.add((uint64_t)(uintptr_t)d_Y, ye * 8u, "d_Y");
    if (int rc = csd_output_ranges(d->flags, outs, (uint64_t)oe, r)) return rc;
    const uint32_t chains = (d->flags & kCsdOutputMask) == BHW_CSD_PXY ? 2u : 4u;
    const uint64_t need = blocks > 1 ? B * blocks * K * chains * 8u : 0;             // below 2^34 / 256 * 32 + ...: no overflow
    if (need) {
        if (!workspace) return bhwp_fail(BHW_ERR_BADARG, "workspace is NULL: %llu frame blocks need %llu bytes", (unsigned long long)blocks,
                                         (unsigned long long)need);
        if ((uintptr_t)workspace % 8) return bhwp_fail(BHW_ERR_BADARG, "workspace is not 8-byte aligned");
        if (workspace_bytes < need)
            return bhwp_fail(BHW_ERR_WORKSPACE, "workspace of %llu bytes, the block sums need %llu", (unsigned long long)workspace_bytes,
                             (unsigned long long)need);
        r.add((uint64_t)(uintptr_t)workspace, need, "workspace");
    }
    return csd_overlaps(r, need != 0);
}

int bhwp_describe_csd(const bhw_csd *d, char *buf, uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const BhwCsdPlan pl = bhwp_csd_plan(d);
    char outs[64] = "";
    static const char *const names[kCsdOutputs] = {"pxy", "pxx", "pyy", "coherence", "h1"};
    static const uint32_t bits[kCsdOutputs] = {BHW_CSD_PXY, BHW_CSD_PXX, BHW_CSD_PYY, BHW_CSD_COHERENCE, BHW_CSD_H1};
    for (uint32_t i = 0; i < kCsdOutputs; ++i)
        if (d->flags & bits[i]) {
            if (outs[0]) strncat(outs, "+", sizeof outs - strlen(outs) - 1);
            strncat(outs, names[i], sizeof outs - strlen(outs) - 1);
        }
    snprintf(buf, len, "welch csd (%s, n_fft %llu, %s%s): k_welch_csd<%u,%d>, %u chains (%s), %llu signals x %llu frames x %llu bins, "
             "%llu block%s of %u frames, grid %llu x %u lanes (%u along the bins x %u waves of %u frames a pass, %u bytes of LDS)%s, "
             "workspace %llu bytes", (d->flags & BHW_CSD_ONESIDED) ? "one-sided" : "two-sided", (unsigned long long)d->n_fft, outs,
             (d->flags & BHW_CSD_BROADCAST_X) ? ", X broadcast" : "", pl.chains, pl.blocks > 1 ? 1 : 0, pl.chains,
             pl.chains == 2 ? "C_re, C_im" : "S_xx, S_yy, C_re, C_im", (unsigned long long)d->batch, (unsigned long long)d->frames,
             (unsigned long long)d->bins, (unsigned long long)pl.blocks, pl.blocks == 1 ? "" : "s", BHW_WELCH_BLOCK, (unsigned long long)pl.grid,
             kPsdLanes * kPsdWaves, kPsdLanes, kPsdWaves, pl.unroll, pl.lds_bytes,
             pl.blocks > 1 ? (pl.chains == 2 ? ", then k_welch_csd_join<2> in block order" : ", then k_welch_csd_join<4> in block order") : "",
             (unsigned long long)pl.ws_bytes);
    return BHW_OK;
}

// ---- fused window and real FFT -------------------------------------------------------------------------------------------------------------

// The descriptor with packed output strides, for a call whose y strides count other rows than the call it borrows its checks or its
// plan from, or that writes no rows at all: t = *s with both y strides 0, and &t is returned.  A NULL or wrongly sized descriptor is
// passed through for the borrowed checks to refuse (t is then not set).
static const bhw_stft *packed_strides(const bhw_stft *s, bhw_stft &t)
{
    if (!s || s->struct_size != sizeof(bhw_stft)) return s;
    t = *s;
    t.y_stride = t.y_batch_stride = 0;
    return &t;
}

int bhwp_stft_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_x, const void *d_Y,
                         bool pointers)
{
    int rc = bhwp_f32_checks(p, length, 0);
    if (rc) return rc;
    if (flags & ~BHW_WELCH_DETREND_CONSTANT) return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x (0 or BHW_WELCH_DETREND_CONSTANT)", flags);
    if (!s) return bhwp_fail(BHW_ERR_BADARG, "stft descriptor is NULL");
    if (s->struct_size != sizeof(bhw_stft)) return bhwp_fail(BHW_ERR_BADARG, "bhw_stft.struct_size %u != %zu", s->struct_size, sizeof(bhw_stft));
    // what the frames or the segments call checks, for the same descriptor with packed rows (the output strides mean something else
    // here and are checked below)
    bhw_stft t;
    packed_strides(s, t);
    const bool segments = (flags & BHW_WELCH_DETREND_CONSTANT) || (!s->pad && !s->col0 && !s->pad_mode);
    if (segments) rc = bhwp_welch_checks(p, length, &t, flags, nullptr, nullptr, nullptr, 0, false);
    else          rc = bhwp_stft_checks(p, length, &t, false, 0, nullptr, nullptr, false);
    if (rc) return rc;
    if (s->channels != 1) return bhwp_fail(BHW_ERR_UNSUPPORTED, "channels %u: the fused FFT takes real input (1)", s->channels);
    if ((s->n_fft & (s->n_fft - 1)) || s->n_fft < (1ull << kFftMinLog) || s->n_fft > (1ull << kFftMaxLog))
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu: the fused FFT takes a power of two in %u..%u", (unsigned long long)s->n_fft,
                         1u << kFftMinLog, 1u << kFftMaxLog);
    const uint64_t T = s->samples, F = s->frames, K2 = s->n_fft + 2;          // 2K floats of a spectrum row
    if (!F) return BHW_OK;
    if ((unsigned __int128)s->batch * F * (K2 / 2) > (1ull << 34)) return bhwp_fail(BHW_ERR_BADARG, "batch * frames * K above 2^34 per call");
    if (s->y_stride && (s->y_stride < K2 || s->y_stride % 2))
        return bhwp_fail(BHW_ERR_BADARG, "y_stride %llu: at least 2 * K = %llu floats, and even", (unsigned long long)s->y_stride,
                         (unsigned long long)K2);
    const uint64_t ys = s->y_stride ? s->y_stride : K2;
    const unsigned __int128 ysig = (unsigned __int128)(F - 1) * ys + K2;
    if (ysig > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "Y extent beyond 2^60 elements");
    if (s->y_batch_stride && (s->y_batch_stride < (uint64_t)ysig || s->y_batch_stride % 2))
        return bhwp_fail(BHW_ERR_BADARG, "y_batch_stride %llu: at least (frames - 1) * y_stride + 2 * K = %llu floats, and even",
                         (unsigned long long)s->y_batch_stride, (unsigned long long)ysig);
    if (!pointers) return BHW_OK;
    if (!d_x || !d_Y) return bhwp_fail(BHW_ERR_BADARG, "d_x / d_Y is NULL");
    if ((uintptr_t)d_Y % 8) return bhwp_fail(BHW_ERR_BADARG, "d_Y is not 8-byte aligned");
    if ((uintptr_t)d_x % 4) return bhwp_fail(BHW_ERR_BADARG, "d_x is not 4-byte aligned");
    const uint64_t xs = s->x_stride ? s->x_stride : T, ybs = s->y_batch_stride ? s->y_batch_stride : F * ys;
    const unsigned __int128 xe = (unsigned __int128)(s->batch - 1) * xs + T, ye = (unsigned __int128)(s->batch - 1) * ybs + ysig;
    if (xe > (1ull << 60) || ye > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "x or Y extent beyond 2^60 elements");
    const uint64_t xa = (uint64_t)(uintptr_t)d_x, ya = (uint64_t)(uintptr_t)d_Y, xb = (uint64_t)xe * 4u, yb = (uint64_t)ye * 4u;
    if (xa > UINT64_MAX - xb || ya > UINT64_MAX - yb) return bhwp_fail(BHW_ERR_BADARG, "x or Y range wraps the address space");
    if (xa < ya + yb && ya < xa + xb) return bhwp_fail(BHW_ERR_BADARG, "d_x and d_Y overlap");
    return BHW_OK;
}

BhwStftFftPlan bhwp_stft_fft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table)
{
    (void)p;
    BhwStftFftPlan pl{};
    pl.route = from_table ? BHWP_FRAMES_TABLE : BHWP_FRAMES_DIRECT;
    pl.detrend = (flags & BHW_WELCH_DETREND_CONSTANT) != 0;
    pl.len = length;
    while ((1ull << pl.log2n) < s->n_fft) ++pl.log2n;
    pl.m = (uint32_t)(s->n_fft / 2);
    const uint32_t quarter = pl.m / 4 < 4 ? 4 : pl.m / 4;
    pl.lpf = quarter < kFftBlock ? quarter : kFftBlock;
    pl.fy = kFftBlock / pl.lpf;
    pl.cpl = (uint32_t)(s->n_fft / pl.lpf);
    pl.radix4 = (pl.log2n - 1) / 2;
    pl.radix2 = (pl.log2n - 1) % 2;
    pl.lds_bytes = 2u * pl.fy * pl.m * 8u + pl.m * 8u + pl.fy * 4u;
    pl.x_stride = s->x_stride ? s->x_stride : s->samples;
    pl.y_stride = s->y_stride ? s->y_stride : s->n_fft + 2;
    pl.y_bstride = s->y_batch_stride ? s->y_batch_stride : s->frames * pl.y_stride;
    pl.rows = s->batch * s->frames;
    pl.groups = (pl.rows + pl.fy - 1) / pl.fy;
    pl.grid = pl.groups < kFftMaxGrid ? pl.groups : kFftMaxGrid;
    return pl;
}

void bhwp_stft_fft_schedule(const BhwStftFftPlan &pl, char *buf, uint64_t len)
{
    if (!buf || !len) return;
    buf[0] = 0;
    for (uint32_t i = 0; i < pl.radix4 + pl.radix2; ++i) {
        const size_t at = strlen(buf);
        snprintf(buf + at, len - at, "%s%d", i ? "x" : "", i < pl.radix4 ? 4 : 2);
    }
}

int bhwp_describe_stft_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                           uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const char *route = ct ? "table" : "direct";
    const BhwStftFftPlan pl = bhwp_stft_fft_plan(p, length, s, flags, ct != nullptr);
    const char *pad = s->pad_mode == BHW_PAD_REFLECT ? "reflect" : "constant";
    const char *det = pl.detrend ? "constant detrend" : "no detrending";
    if (!s->frames) {
        snprintf(buf, len, "stft fft %s (L = %llu, n_fft %llu, %s): nothing (frames 0)", route, (unsigned long long)length,
                 (unsigned long long)s->n_fft, det);
        return BHW_OK;
    }
    char kern[64], sched[48];
    kernel_name(p, ct, "k_stft_fft_direct", "k_stft_fft_table", false, kern, sizeof kern);
    bhwp_stft_fft_schedule(pl, sched, sizeof sched);
    snprintf(buf, len, "stft fft %s (L = %llu, n_fft %llu, col0 %llu, pad %llu %s, %s): %s, %llu signals x %llu frames = %llu rows, "
             "complex FFT of %u points in passes %s + split, %u lanes per row x %u rows per workgroup, %u columns per lane, %llu groups, "
             "grid %llu x %u lanes, %u bytes of LDS", route, (unsigned long long)length, (unsigned long long)s->n_fft,
             (unsigned long long)s->col0, (unsigned long long)s->pad, pad, det, kern, (unsigned long long)s->batch,
             (unsigned long long)s->frames, (unsigned long long)pl.rows, pl.m, sched, pl.lpf, pl.fy, pl.cpl, (unsigned long long)pl.groups,
             (unsigned long long)pl.grid, kFftBlock, pl.lds_bytes);
    return BHW_OK;
}

// ---- fused power and filter-bank spectrogram ---------------------------------------------------------------------------------------------

int bhwp_spectrogram_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb, const void *d_x,
                            const void *d_P, bool pointers)
{
    // the input side: the forward call's checks for the descriptor with packed output strides (they count other rows here)
    bhw_stft t;
    int rc = bhwp_stft_fft_checks(p, length, packed_strides(s, t), flags, nullptr, nullptr, false);
    if (rc) return rc;
    const uint64_t T = s->samples, F = s->frames, K = s->n_fft / 2 + 1;
    if (fb) {
        if (fb->struct_size != sizeof(bhw_fbank))
            return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.struct_size %u != %zu", fb->struct_size, sizeof(bhw_fbank));
        if (fb->reserved) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.reserved is not 0");
        if (fb->filters < 1 || fb->filters > kSpecMaxFilters)
            return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.filters %u outside 1..%u", fb->filters, kSpecMaxFilters);
        if (fb->bins != K)
            return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.bins %u: the call has n_fft / 2 + 1 = %llu bins", fb->bins, (unsigned long long)K);
        if (fb->weights > kSpecMaxWeights) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.weights %u above 2^24", fb->weights);
    }
    if (!F) return BHW_OK;
    const uint64_t W = fb ? fb->filters : K;
    if ((unsigned __int128)s->batch * F * W > (1ull << 34)) return bhwp_fail(BHW_ERR_BADARG, "batch * frames * W above 2^34 per call");
    if (s->y_stride && s->y_stride < W)
        return bhwp_fail(BHW_ERR_BADARG, "y_stride %llu: at least W = %llu floats", (unsigned long long)s->y_stride, (unsigned long long)W);
    const uint64_t ys = s->y_stride ? s->y_stride : W;
    const unsigned __int128 ysig = (unsigned __int128)(F - 1) * ys + W;
    if (ysig > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "P extent beyond 2^60 elements");
    if (s->y_batch_stride && s->y_batch_stride < (uint64_t)ysig)
        return bhwp_fail(BHW_ERR_BADARG, "y_batch_stride %llu: at least (frames - 1) * y_stride + W = %llu floats",
                         (unsigned long long)s->y_batch_stride, (unsigned long long)ysig);
    if (!pointers) return BHW_OK;
    if (!d_x || !d_P) return bhwp_fail(BHW_ERR_BADARG, "d_x / d_P is NULL");
    if ((uintptr_t)d_P % 4) return bhwp_fail(BHW_ERR_BADARG, "d_P is not 4-byte aligned");
    if ((uintptr_t)d_x % 4) return bhwp_fail(BHW_ERR_BADARG, "d_x is not 4-byte aligned");
    const uint64_t xs = s->x_stride ? s->x_stride : T, ybs = s->y_batch_stride ? s->y_batch_stride : F * ys;
    const unsigned __int128 xe = (unsigned __int128)(s->batch - 1) * xs + T, ye = (unsigned __int128)(s->batch - 1) * ybs + ysig;
    if (xe > (1ull << 60) || ye > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "x or P extent beyond 2^60 elements");
    const uint64_t xa = (uint64_t)(uintptr_t)d_x, ya = (uint64_t)(uintptr_t)d_P, xb = (uint64_t)xe * 4u, yb = (uint64_t)ye * 4u;
    if (xa > UINT64_MAX - xb || ya > UINT64_MAX - yb) return bhwp_fail(BHW_ERR_BADARG, "x or P range wraps the address space");
    if (xa < ya + yb && ya < xa + xb) return bhwp_fail(BHW_ERR_BADARG, "d_x and d_P overlap");
    if (fb) {
        if (!fb->d_first || !fb->d_offset) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.d_first / d_offset is NULL");
        if (!fb->d_weight && fb->weights) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.d_weight is NULL with %u weights", fb->weights);
        const void *ptr[3] = {fb->d_first, fb->d_offset, fb->d_weight};
        const uint64_t nb[3] = {(uint64_t)fb->filters * 4u, ((uint64_t)fb->filters + 1u) * 4u, (uint64_t)fb->weights * 4u};
        static const char *const what[3] = {"d_first", "d_offset", "d_weight"};
        for (int i = 0; i < 3; ++i) {
            const uint64_t a = (uint64_t)(uintptr_t)ptr[i];
            if (a % 4) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.%s is not 4-byte aligned", what[i]);
            if (a > UINT64_MAX - nb[i]) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.%s range wraps the address space", what[i]);
            if (nb[i] && a < ya + yb && ya < a + nb[i]) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.%s and d_P overlap", what[i]);
        }
    }
    return BHW_OK;
}

BhwStftFftPlan bhwp_spectrogram_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                                     bool from_table)
{
    BhwStftFftPlan pl = bhwp_stft_fft_plan(p, length, s, flags, from_table);
    const uint64_t W = fb ? fb->filters : s->n_fft / 2 + 1;
    pl.y_stride = s->y_stride ? s->y_stride : W;
    pl.y_bstride = s->y_batch_stride ? s->y_batch_stride : s->frames * pl.y_stride;
    return pl;
}

int bhwp_describe_spectrogram(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                              const bhw_fbank *fb, char *buf, uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const char *route = ct ? "table" : "direct";
    const BhwStftFftPlan pl = bhwp_spectrogram_plan(p, length, s, flags, fb, ct != nullptr);
    const char *pad = s->pad_mode == BHW_PAD_REFLECT ? "reflect" : "constant";
    const char *det = pl.detrend ? "constant detrend" : "no detrending";
    const uint64_t W = fb ? fb->filters : s->n_fft / 2 + 1;
    char mode[96];
    if (fb) snprintf(mode, sizeof mode, "bank mode, W = %llu (%u filters, %u weights, %u filters per lane)", (unsigned long long)W, fb->filters,
                     fb->weights, (fb->filters + pl.lpf - 1) / pl.lpf);
    else    snprintf(mode, sizeof mode, "power mode, W = %llu", (unsigned long long)W);
    if (!s->frames) {
        snprintf(buf, len, "spectrogram %s (L = %llu, n_fft %llu, %s), %s: nothing (frames 0)", route, (unsigned long long)length,
                 (unsigned long long)s->n_fft, det, mode);
        return BHW_OK;
    }
    char kern[64], sched[48];
    kernel_name(p, ct, "k_spectrogram_direct", "k_spectrogram_table", false, kern, sizeof kern);
    bhwp_stft_fft_schedule(pl, sched, sizeof sched);
    snprintf(buf, len, "spectrogram %s (L = %llu, n_fft %llu, col0 %llu, pad %llu %s, %s), %s: %s, %llu signals x %llu frames = %llu rows, "
             "complex FFT of %u points in passes %s + split, %u lanes per row x %u rows per workgroup, %u columns per lane, %llu groups, "
             "grid %llu x %u lanes, %u bytes of LDS", route, (unsigned long long)length, (unsigned long long)s->n_fft,
             (unsigned long long)s->col0, (unsigned long long)s->pad, pad, det, mode, kern, (unsigned long long)s->batch,
             (unsigned long long)s->frames, (unsigned long long)pl.rows, pl.m, sched, pl.lpf, pl.fy, pl.cpl, (unsigned long long)pl.groups,
             (unsigned long long)pl.grid, kFftBlock, pl.lds_bytes);
    return BHW_OK;
}

// ---- fused Welch PSD ------------------------------------------------------------------------------------------------------------------------

BhwWelchRuns bhwp_welch_runs(uint64_t batch, uint64_t F, uint32_t fy, uint64_t bins, uint64_t p_stride)
{
    BhwWelchRuns r{};
    r.bins = bins;
    r.p_stride = p_stride ? p_stride : bins;
    r.run = fy > BHW_WELCH_FFT_CHUNK ? fy : BHW_WELCH_FFT_CHUNK;
    r.gpr = (uint32_t)(r.run / fy);
    r.acc = fy >= BHW_WELCH_FFT_CHUNK ? 0u : (uint32_t)((bins + kFftBlock - 1) / kFftBlock);
    if (!F || !batch) return r;
    r.fpad = ((F - 1) / r.run + 1) * r.run;
    r.chunks = (F - 1) / BHW_WELCH_FFT_CHUNK + 1;
    r.blocks = (F - 1) / BHW_WELCH_BLOCK + 1;
    r.runs = batch * (r.fpad / r.run);
    r.groups = r.runs * r.gpr;
    r.grid = r.runs < kFftMaxGrid ? r.runs : kFftMaxGrid;
    r.blocks_grid = (batch * r.blocks * bins + 255u) / 256u;
    r.join_grid = r.blocks > 1 ? (batch * bins + 255u) / 256u : 0;
    const unsigned __int128 n = (unsigned __int128)batch * (r.chunks + (r.blocks > 1 ? r.blocks : 0)) * bins;
    r.ws_bytes = n > (1ull << 57) ? 0 : (uint64_t)n * 8u;
    return r;
}

// The output side of every fused Welch call, after the forward call's checks and the refusal of that call's power flag: the y strides,
// psd_flags (the real-input calls; NULL for I/Q input), scale, p_stride, the 2^34 bound, the pointers, the workspace and the overlaps,
// in the order of include/bhw.h.  bins: the columns of a row of P; xf: the floats of a sample of x (1 real, 2 I/Q); row, cap: the
// words for `bins` in the p_stride and the 2^34 messages ("bins" and "K", or "n_fft" twice).  The hold calls pass `pointers` false and
// check theirs in hold_pointer_checks.
static int welch_output_checks(const bhw_stft *s, uint64_t bins, uint64_t xf, const char *row, const char *cap, double scale,
                               const uint32_t *psd_flags, uint64_t p_stride, const void *d_x, const void *d_P, const void *workspace,
                               uint64_t workspace_bytes, bool pointers)
{
    if (s->y_stride || s->y_batch_stride)
        return bhwp_fail(BHW_ERR_BADARG, "y_stride %llu, y_batch_stride %llu: no spectrum is written, both must be 0",
                         (unsigned long long)s->y_stride, (unsigned long long)s->y_batch_stride);
    if (psd_flags && (*psd_flags & ~BHW_PSD_ONESIDED)) return bhwp_fail(BHW_ERR_BADARG, "psd_flags 0x%x (0 or BHW_PSD_ONESIDED)", *psd_flags);
    if (!(scale - scale == 0.0)) return bhwp_fail(BHW_ERR_BADARG, "scale is not finite");
    const uint64_t T = xf * s->samples, F = s->frames;                  // T: the floats of a signal
    if (!F) return BHW_OK;
    if (p_stride && p_stride < bins)
        return bhwp_fail(BHW_ERR_BADARG, "p_stride %llu < %s %llu: rows overlap", (unsigned long long)p_stride, row, (unsigned long long)bins);
    const uint64_t chunks = (F - 1) / BHW_WELCH_FFT_CHUNK + 1;
    if ((unsigned __int128)s->batch * chunks * bins > (1ull << 34))
        return bhwp_fail(BHW_ERR_BADARG, "batch * ceil(frames / %u) * %s above 2^34 per call", BHW_WELCH_FFT_CHUNK, cap);
    if (!pointers) return BHW_OK;
    if (!d_x || !d_P) return bhwp_fail(BHW_ERR_BADARG, "d_x / d_P is NULL");
    if ((uintptr_t)d_P % 4) return bhwp_fail(BHW_ERR_BADARG, "d_P is not 4-byte aligned");
    if ((uintptr_t)d_x % 4) return bhwp_fail(BHW_ERR_BADARG, "d_x is not 4-byte aligned");
    const uint64_t need = bhwp_welch_runs(s->batch, F, 1, bins).ws_bytes;                 // the bytes do not depend on fy
    if (!workspace) return bhwp_fail(BHW_ERR_BADARG, "workspace is NULL: the chunk sums need %llu bytes", (unsigned long long)need);
    if ((uintptr_t)workspace % 8) return bhwp_fail(BHW_ERR_BADARG, "workspace is not 8-byte aligned");
    if (workspace_bytes < need)
        return bhwp_fail(BHW_ERR_WORKSPACE, "workspace of %llu bytes, the chunk and block sums need %llu", (unsigned long long)workspace_bytes,
                         (unsigned long long)need);
    const uint64_t xs = s->x_stride ? s->x_stride : T, ps = p_stride ? p_stride : bins;
    const unsigned __int128 xe = (unsigned __int128)(s->batch - 1) * xs + T, pe = (unsigned __int128)(s->batch - 1) * ps + bins;
    if (xe > (1ull << 60) || pe > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "x or P extent beyond 2^60 elements");
    const uint64_t xa = (uint64_t)(uintptr_t)d_x, pa = (uint64_t)(uintptr_t)d_P, wa = (uint64_t)(uintptr_t)workspace;
    const uint64_t xb = (uint64_t)xe * 4u, pb = (uint64_t)pe * 4u;
    if (xa > UINT64_MAX - xb || pa > UINT64_MAX - pb || wa > UINT64_MAX - need)
        return bhwp_fail(BHW_ERR_BADARG, "x, P or workspace range wraps the address space");
    if (xa < pa + pb && pa < xa + xb) return bhwp_fail(BHW_ERR_BADARG, "d_x and d_P overlap");
    if ((wa < xa + xb && xa < wa + need) || (wa < pa + pb && pa < wa + need))
        return bhwp_fail(BHW_ERR_BADARG, "workspace overlaps d_x or d_P");
    return BHW_OK;
}

// The run plan of a Welch plan whose forward plan is set -- the plan's BhwWelchRuns base --, with the groups and the grid of pl.fft
// recounted from the runs and its y strides 0 (no spectrum is written).
template <class Plan>
static void welch_plan_runs(Plan &pl, const bhw_stft *s, uint64_t bins, uint64_t p_stride)
{
    pl.fft.y_stride = pl.fft.y_bstride = 0;
    static_cast<BhwWelchRuns &>(pl) = bhwp_welch_runs(s->batch, s->frames, pl.fft.fy, bins, p_stride);
    pl.fft.groups = pl.groups;
    pl.fft.grid = pl.grid;
}

// The common end of the four describe_*_runs lines, appended to the head in buf: from "; chunk" to the tail.
static void describe_runs_tail(char *buf, uint64_t len, const BhwWelchRuns &r, const char *join, const char *tail)
{
    const size_t at = strlen(buf);
    snprintf(buf + at, len - at, "; chunk %u frames, %llu runs of %llu frames (%u group%s per run), %u accumulator%s per lane, %llu chunks "
             "and %llu block%s per signal, then %s %s, workspace %llu bytes%s",
             BHW_WELCH_FFT_CHUNK, (unsigned long long)r.runs, (unsigned long long)r.run, r.gpr, r.gpr == 1 ? "" : "s", r.acc,
             r.acc == 1 ? "" : "s", (unsigned long long)r.chunks, (unsigned long long)r.blocks, r.blocks == 1 ? "" : "s", join,
             r.blocks == 1 ? "once (chunks)" : "twice (chunks, blocks)", (unsigned long long)r.ws_bytes, tail);
}

uint64_t bhwp_welch_fft_workspace_bytes(const bhw_stft *s)
{
    if (!s || !s->frames || !s->batch) return 0;
    return bhwp_welch_runs(s->batch, s->frames, 1, s->n_fft / 2 + 1).ws_bytes;        // the bytes do not depend on fy
}

int bhwp_welch_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint32_t psd_flags,
                          uint64_t p_stride, const void *d_x, const void *d_P, const void *workspace, uint64_t workspace_bytes,
                          bool pointers)
{
    // the input side: the forward call's checks for the descriptor with packed output strides (no spectrum is written here)
    bhw_stft t;
    const bhw_stft *packed = packed_strides(s, t);
    int rc = bhwp_stft_fft_checks(p, length, packed, flags, nullptr, nullptr, false);
    if (rc) return rc;
    return welch_output_checks(s, s->n_fft / 2 + 1, 1, "bins", "K", scale, &psd_flags, p_stride, d_x, d_P, workspace, workspace_bytes, pointers);
}

BhwWelchFftPlan bhwp_welch_fft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                    bool from_table)
{
    BhwWelchFftPlan pl{};
    bhw_stft t;
    packed_strides(s, t);
    pl.fft = bhwp_stft_fft_plan(p, length, &t, flags, from_table);
    welch_plan_runs(pl, s, s->n_fft / 2 + 1, p_stride);
    return pl;
}

// The describe line of the calls that put stft_fft_rows under an epilogue that owns runs: bhw_describe_welch_fft (what "welch", the
// join k_welch_fft_join, no tail) and bhw_describe_hold_fft (what "hold", its kernels, its join and the traces as the tail).
static int describe_fft_runs(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                             const char *what, const char *k_direct, const char *k_table, const char *join, const char *tail, char *buf,
                             uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const char *route = ct ? "table" : "direct";
    const BhwWelchFftPlan wp = bhwp_welch_fft_plan(p, length, s, flags, 0, ct != nullptr);
    const BhwStftFftPlan &pl = wp.fft;
    const char *pad = s->pad_mode == BHW_PAD_REFLECT ? "reflect" : "constant";
    const char *det = pl.detrend ? "constant detrend" : "no detrending";
    if (!s->frames) {
        snprintf(buf, len, "%s fft %s (L = %llu, n_fft %llu, %s): nothing (frames 0)%s", what, route, (unsigned long long)length,
                 (unsigned long long)s->n_fft, det, tail);
        return BHW_OK;
    }
    char kern[64], sched[48];
    kernel_name(p, ct, k_direct, k_table, false, kern, sizeof kern);
    bhwp_stft_fft_schedule(pl, sched, sizeof sched);
    snprintf(buf, len, "%s fft %s (L = %llu, n_fft %llu, col0 %llu, pad %llu %s, %s): %s, %llu signals x %llu frames = %llu rows, "
             "complex FFT of %u points in passes %s + split, %u lanes per row x %u rows per workgroup, %u columns per lane, %llu groups, "
             "grid %llu x %u lanes, %u bytes of LDS",
             what, route, (unsigned long long)length, (unsigned long long)s->n_fft, (unsigned long long)s->col0, (unsigned long long)s->pad, pad,
             det, kern, (unsigned long long)s->batch, (unsigned long long)s->frames, (unsigned long long)pl.rows, pl.m, sched, pl.lpf, pl.fy,
             pl.cpl, (unsigned long long)pl.groups, (unsigned long long)pl.grid, kFftBlock, pl.lds_bytes);
    describe_runs_tail(buf, len, wp, join, tail);
    return BHW_OK;
}

int bhwp_describe_welch_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                            uint64_t len)
{
    return describe_fft_runs(p, ct, length, s, flags, "welch", "k_welch_fft_direct", "k_welch_fft_table", "k_welch_fft_join", "", buf, len);
}

// ---- fused Welch cross spectra ----------------------------------------------------------------------------------------------------------------

uint64_t bhwp_csd_fft_workspace_bytes(const bhw_stft *s)
{
    if (!s || !s->frames || !s->batch) return 0;
    return bhwp_welch_runs(s->batch, s->frames, 1, kCsdFftChains * (s->n_fft / 2 + 1)).ws_bytes;   // four chains on the bin axis
}

int bhwp_csd_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint32_t csd_flags,
                        uint64_t o_stride, const void *d_x, const void *d_y, const void *const *outs, const void *workspace,
                        uint64_t workspace_bytes, bool pointers)
{
    // the descriptor: bhwp_welch_fft_checks' in its order, with the routes that take what this call refuses named
    bhw_stft t;
    const bhw_stft *packed = packed_strides(s, t);
    // the params first, as every fused call has them first: their refusals (the source, the model, phi_width) keep their words
    int rc = bhwp_f32_checks(p, length, 0);
    if (rc) return rc;
    rc = bhwp_stft_fft_checks(p, length, packed, flags, nullptr, nullptr, false);
    const bool sized = packed == &t;
    const bool pow2 = sized && s->n_fft && !(s->n_fft & (s->n_fft - 1)) && s->n_fft >= (1ull << kFftMinLog) && s->n_fft <= (1ull << kFftMaxLog);
    if (rc == BHW_ERR_UNSUPPORTED && sized && (s->channels != 1 || !pow2)) {           // the two refusals this call renames
        if (s->channels != 1)
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "channels %u: the fused cross spectra take real input (1); for I/Q input use "
                             "bhw_stft_cfft_f32_* + bhw_welch_csd_f32", s->channels);
        if (bhwp_mfft_supported(s->n_fft))
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu: the fused cross spectra take a power of two in %u..%u; for a mixed-radix "
                             "n_fft use bhw_stft_mfft_f32_* + bhw_welch_csd_f32", (unsigned long long)s->n_fft, 1u << kFftMinLog,
                             1u << kCsdFftMaxLog);
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu: the fused cross spectra take a power of two in %u..%u",
                         (unsigned long long)s->n_fft, 1u << kFftMinLog, 1u << kCsdFftMaxLog);
    }
    if (rc) return rc;
    if (s->n_fft > (1ull << kCsdFftMaxLog))
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu: the fused cross spectra take a power of two in %u..%u (two operands side by "
                         "side); use bhw_stft_fft_f32_* + bhw_welch_csd_f32", (unsigned long long)s->n_fft, 1u << kFftMinLog,
                         1u << kCsdFftMaxLog);
    if (s->y_stride || s->y_batch_stride)
        return bhwp_fail(BHW_ERR_BADARG, "y_stride %llu, y_batch_stride %llu: no spectrum is written, both must be 0",
                         (unsigned long long)s->y_stride, (unsigned long long)s->y_batch_stride);
    if (csd_flags & ~(BHW_CSD_ONESIDED | BHW_CSD_BROADCAST_X | kCsdOutputMask))
        return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x (BHW_CSD_ONESIDED, BHW_CSD_BROADCAST_X and the output mask 0x%x)", csd_flags, kCsdOutputMask);
    if (!(csd_flags & kCsdOutputMask)) return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x: the output mask is empty", csd_flags);
    if (!(scale - scale == 0.0)) return bhwp_fail(BHW_ERR_BADARG, "scale is not finite");
    const uint64_t T = s->samples, F = s->frames, K = s->n_fft / 2 + 1, B = s->batch;
    if (!F) return BHW_OK;
    if (o_stride && o_stride < K)
        return bhwp_fail(BHW_ERR_BADARG, "o_stride %llu < bins %llu: rows overlap", (unsigned long long)o_stride, (unsigned long long)K);
    const uint64_t chunks = (F - 1) / BHW_WELCH_FFT_CHUNK + 1;
    if ((unsigned __int128)B * chunks * K * kCsdFftChains > (1ull << 34))
        return bhwp_fail(BHW_ERR_BADARG, "batch * ceil(frames / %u) * 4 K above 2^34 per call", BHW_WELCH_FFT_CHUNK);
    if (!pointers) return BHW_OK;
    if (!d_x || !d_y) return bhwp_fail(BHW_ERR_BADARG, "d_x / d_y is NULL");
    if ((uintptr_t)d_x % 4 || (uintptr_t)d_y % 4) return bhwp_fail(BHW_ERR_BADARG, "d_x / d_y is not 4-byte aligned");
    const bool bcast = (csd_flags & BHW_CSD_BROADCAST_X) != 0;
    const uint64_t xs = s->x_stride ? s->x_stride : T;
    const unsigned __int128 ye = (unsigned __int128)(B - 1) * xs + T, xe = bcast ? (unsigned __int128)T : ye;
    const unsigned __int128 oe = (unsigned __int128)(B - 1) * (o_stride ? o_stride : K) + K;
    if (ye > (1ull << 58) || oe > (1ull << 58)) return bhwp_fail(BHW_ERR_BADARG, "x, y or output extent beyond 2^58 elements");
    CsdRanges r;
    r.add((uint64_t)(uintptr_t)d_x, (uint64_t)xe * 4u, "d_x");
    r.add((uint64_t)(uintptr_t)d_y, (uint64_t)ye * 4u, "d_y");
    if ((rc = csd_output_ranges(csd_flags, outs, (uint64_t)oe, r))) return rc;
    const uint64_t need = bhwp_csd_fft_workspace_bytes(s);
    if (!workspace) return bhwp_fail(BHW_ERR_BADARG, "workspace is NULL: the chunk sums need %llu bytes", (unsigned long long)need);
    if ((uintptr_t)workspace % 8) return bhwp_fail(BHW_ERR_BADARG, "workspace is not 8-byte aligned");
    if (workspace_bytes < need)
        return bhwp_fail(BHW_ERR_WORKSPACE, "workspace of %llu bytes, the chunk and block sums need %llu", (unsigned long long)workspace_bytes,
                         (unsigned long long)need);
    r.add((uint64_t)(uintptr_t)workspace, need, "workspace");
    return csd_overlaps(r, true);
}

BhwCsdFftPlan bhwp_csd_fft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint32_t csd_flags,
                                uint64_t o_stride, bool from_table)
{
    BhwCsdFftPlan pl{};
    bhw_stft t;
    packed_strides(s, t);
    BhwStftFftPlan &f = pl.fft;
    f = bhwp_stft_fft_plan(p, length, &t, flags, from_table);
    f.y_stride = f.y_bstride = 0;
    if (f.lpf > kCsdFftMaxLpf) {                                        // n_fft 2048: two slots of 128 lanes
        f.lpf = kCsdFftMaxLpf;
        f.fy = kFftBlock / f.lpf;
        f.cpl = (uint32_t)(s->n_fft / f.lpf);
        f.lds_bytes = 2u * f.fy * f.m * 8u + f.m * 8u + f.fy * 4u;
    }
    pl.bins = s->n_fft / 2 + 1;
    pl.pairs = f.fy / 2u;
    pl.flags = csd_flags;
    const BhwWelchRuns r = bhwp_welch_runs(s->batch, s->frames, pl.pairs, kCsdFftChains * pl.bins);
    pl.run = r.run;
    pl.gpr = r.gpr;
    pl.acc = pl.pairs >= BHW_WELCH_FFT_CHUNK ? 0u : (uint32_t)((pl.bins + kFftBlock - 1) / kFftBlock);
    pl.fpad = r.fpad;
    pl.chunks = r.chunks;
    pl.blocks = r.blocks;
    pl.runs = r.runs;
    f.groups = r.groups;
    f.grid = r.grid;
    pl.blocks_grid = r.blocks > 1 ? r.blocks_grid : 0;
    pl.out_grid = s->frames ? (s->batch * pl.bins + 255u) / 256u : 0;
    pl.o_stride = o_stride ? o_stride : pl.bins;
    pl.ws_bytes = r.ws_bytes;
    return pl;
}

int bhwp_describe_csd_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                          uint32_t csd_flags, char *buf, uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const char *route = ct ? "table" : "direct";
    const BhwCsdFftPlan cp = bhwp_csd_fft_plan(p, length, s, flags, csd_flags, 0, ct != nullptr);
    const BhwStftFftPlan &pl = cp.fft;
    const char *pad = s->pad_mode == BHW_PAD_REFLECT ? "reflect" : "constant";
    const char *det = pl.detrend ? "constant detrend" : "no detrending";
    if (!s->frames) {
        snprintf(buf, len, "csd fft %s (L = %llu, n_fft %llu, %s): nothing (frames 0)", route, (unsigned long long)length,
                 (unsigned long long)s->n_fft, det);
        return BHW_OK;
    }
    char outs[64] = "";
    static const char *const names[kCsdOutputs] = {"pxy", "pxx", "pyy", "coherence", "h1"};
    static const uint32_t bits[kCsdOutputs] = {BHW_CSD_PXY, BHW_CSD_PXX, BHW_CSD_PYY, BHW_CSD_COHERENCE, BHW_CSD_H1};
    for (uint32_t i = 0; i < kCsdOutputs; ++i)
        if (csd_flags & bits[i]) {
            if (outs[0]) strncat(outs, "+", sizeof outs - strlen(outs) - 1);
            strncat(outs, names[i], sizeof outs - strlen(outs) - 1);
        }
    char kern[64], sched[48];
    kernel_name(p, ct, "k_csd_fft_direct", "k_csd_fft_table", false, kern, sizeof kern);
    bhwp_stft_fft_schedule(pl, sched, sizeof sched);
    snprintf(buf, len, "csd fft %s (L = %llu, n_fft %llu, col0 %llu, pad %llu %s, %s): %s, %llu signals x %llu frames = %llu rows, "
             "complex FFT of %u points in passes %s + split, %u lanes per row x %u rows per workgroup, %u columns per lane, %llu groups, "
             "grid %llu x %u lanes, %u bytes of LDS; %u frame pair%s per group (x and y side by side%s), %s, %s; chunk %u frames, %llu runs "
             "of %llu frames (%u group%s per run), %u accumulator%s per lane and chain, %u chains, %llu chunks and %llu block%s per "
             "signal, then %s, workspace %llu bytes",
             route, (unsigned long long)length, (unsigned long long)s->n_fft, (unsigned long long)s->col0, (unsigned long long)s->pad, pad,
             det, kern, (unsigned long long)s->batch, (unsigned long long)s->frames, (unsigned long long)pl.rows, pl.m, sched, pl.lpf, pl.fy,
             pl.cpl, (unsigned long long)pl.groups, (unsigned long long)pl.grid, kFftBlock, pl.lds_bytes, cp.pairs, cp.pairs == 1 ? "" : "s",
             (csd_flags & BHW_CSD_BROADCAST_X) ? ", x broadcast" : "", (csd_flags & BHW_CSD_ONESIDED) ? "one-sided" : "two-sided", outs,
             BHW_WELCH_FFT_CHUNK, (unsigned long long)cp.runs, (unsigned long long)cp.run, cp.gpr, cp.gpr == 1 ? "" : "s", cp.acc,
             cp.acc == 1 ? "" : "s", kCsdFftChains, (unsigned long long)cp.chunks, (unsigned long long)cp.blocks, cp.blocks == 1 ? "" : "s",
             cp.blocks == 1 ? "k_csd_fft_out once (chunks)" : "k_welch_fft_join (chunks) and k_csd_fft_out (blocks), twice",
             (unsigned long long)cp.ws_bytes);
    return BHW_OK;
}

// ---- mixed-radix fused window and real FFT -------------------------------------------------------------------------------------------------

bool bhwp_mfft_supported(uint64_t n)
{
    if (n < kMfftMinN || n > kMfftMaxN || (n & 1u) || !(n & (n - 1))) return false;
    for (const uint64_t r : {2ull, 3ull, 5ull})
        while (n % r == 0) n /= r;
    return n == 1;
}

int bhwp_stft_mfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb, const void *d_x,
                          const void *d_out, bool pointers)
{
    int rc = bhwp_f32_checks(p, length, 0);
    if (rc) return rc;
    if (flags & ~(BHW_WELCH_DETREND_CONSTANT | BHW_MFFT_POWER))
        return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x (any of BHW_WELCH_DETREND_CONSTANT, BHW_MFFT_POWER)", flags);
    if (!s) return bhwp_fail(BHW_ERR_BADARG, "stft descriptor is NULL");
    if (s->struct_size != sizeof(bhw_stft)) return bhwp_fail(BHW_ERR_BADARG, "bhw_stft.struct_size %u != %zu", s->struct_size, sizeof(bhw_stft));
    if (fb && !(flags & BHW_MFFT_POWER)) return bhwp_fail(BHW_ERR_BADARG, "a filter bank folds powers: fb needs BHW_MFFT_POWER in flags");
    // what the frames or the segments call checks, for the same descriptor with packed rows (the output strides mean something else
    // here and are checked below)
    bhw_stft t;
    packed_strides(s, t);
    const uint32_t det = flags & BHW_WELCH_DETREND_CONSTANT;
    const bool segments = det || (!s->pad && !s->col0 && !s->pad_mode);
    if (segments) rc = bhwp_welch_checks(p, length, &t, det, nullptr, nullptr, nullptr, 0, false);
    else          rc = bhwp_stft_checks(p, length, &t, false, 0, nullptr, nullptr, false);
    if (rc) return rc;
    if (s->channels != 1)
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "channels %u: the mixed-radix fused FFT takes real input (1)", s->channels);
    if (!(s->n_fft & (s->n_fft - 1)))
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu is a power of two: bhw_stft_fft_f32_* and bhw_spectrogram_f32_* transform it "
                         "(one transform per n_fft)", (unsigned long long)s->n_fft);
    if (!bhwp_mfft_supported(s->n_fft))
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu: the mixed-radix fused FFT takes an even 2^a 3^b 5^c in %u..%u", (unsigned long long)s->n_fft,
                         kMfftMinN, kMfftMaxN);
    const uint64_t T = s->samples, F = s->frames, K = s->n_fft / 2 + 1;
    if (fb) {
        if (fb->struct_size != sizeof(bhw_fbank))
            return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.struct_size %u != %zu", fb->struct_size, sizeof(bhw_fbank));
        if (fb->reserved) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.reserved is not 0");
        if (fb->filters < 1 || fb->filters > kSpecMaxFilters)
            return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.filters %u outside 1..%u", fb->filters, kSpecMaxFilters);
        if (fb->bins != K)
            return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.bins %u: the call has n_fft / 2 + 1 = %llu bins", fb->bins, (unsigned long long)K);
        if (fb->weights > kSpecMaxWeights) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.weights %u above 2^24", fb->weights);
    }
    if (!F) return BHW_OK;
    // the output rows: W floats each; spectrum rows are complex64 pairs (even strides, 8-byte alignment)
    const bool spectrum = !(flags & BHW_MFFT_POWER);
    const uint64_t W = spectrum ? 2 * K : fb ? fb->filters : K;
    const char *wname = spectrum ? "2 * K" : "W";
    if ((unsigned __int128)s->batch * F * (spectrum ? K : W) > (1ull << 34))
        return bhwp_fail(BHW_ERR_BADARG, "batch * frames * %s above 2^34 per call", spectrum ? "K" : "W");
    if (s->y_stride && (s->y_stride < W || (spectrum && s->y_stride % 2)))
        return bhwp_fail(BHW_ERR_BADARG, "y_stride %llu: at least %s = %llu floats%s", (unsigned long long)s->y_stride, wname,
                         (unsigned long long)W, spectrum ? ", and even" : "");
    const uint64_t ys = s->y_stride ? s->y_stride : W;
    const unsigned __int128 ysig = (unsigned __int128)(F - 1) * ys + W;
    if (ysig > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "output extent beyond 2^60 elements");
    if (s->y_batch_stride && (s->y_batch_stride < (uint64_t)ysig || (spectrum && s->y_batch_stride % 2)))
        return bhwp_fail(BHW_ERR_BADARG, "y_batch_stride %llu: at least (frames - 1) * y_stride + %s = %llu floats%s",
                         (unsigned long long)s->y_batch_stride, wname, (unsigned long long)ysig, spectrum ? ", and even" : "");
    if (!pointers) return BHW_OK;
    if (!d_x || !d_out) return bhwp_fail(BHW_ERR_BADARG, "d_x / d_out is NULL");
    if ((uintptr_t)d_out % (spectrum ? 8 : 4)) return bhwp_fail(BHW_ERR_BADARG, "d_out is not %d-byte aligned", spectrum ? 8 : 4);
    if ((uintptr_t)d_x % 4) return bhwp_fail(BHW_ERR_BADARG, "d_x is not 4-byte aligned");
    const uint64_t xs = s->x_stride ? s->x_stride : T, ybs = s->y_batch_stride ? s->y_batch_stride : F * ys;
    const unsigned __int128 xe = (unsigned __int128)(s->batch - 1) * xs + T, ye = (unsigned __int128)(s->batch - 1) * ybs + ysig;
    if (xe > (1ull << 60) || ye > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "x or output extent beyond 2^60 elements");
    const uint64_t xa = (uint64_t)(uintptr_t)d_x, ya = (uint64_t)(uintptr_t)d_out, xb = (uint64_t)xe * 4u, yb = (uint64_t)ye * 4u;
    if (xa > UINT64_MAX - xb || ya > UINT64_MAX - yb) return bhwp_fail(BHW_ERR_BADARG, "x or output range wraps the address space");
    if (xa < ya + yb && ya < xa + xb) return bhwp_fail(BHW_ERR_BADARG, "d_x and d_out overlap");
    if (fb) {
        if (!fb->d_first || !fb->d_offset) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.d_first / d_offset is NULL");
        if (!fb->d_weight && fb->weights) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.d_weight is NULL with %u weights", fb->weights);
        const void *ptr[3] = {fb->d_first, fb->d_offset, fb->d_weight};
        const uint64_t nb[3] = {(uint64_t)fb->filters * 4u, ((uint64_t)fb->filters + 1u) * 4u, (uint64_t)fb->weights * 4u};
        static const char *const what[3] = {"d_first", "d_offset", "d_weight"};
        for (int i = 0; i < 3; ++i) {
            const uint64_t a = (uint64_t)(uintptr_t)ptr[i];
            if (a % 4) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.%s is not 4-byte aligned", what[i]);
            if (a > UINT64_MAX - nb[i]) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.%s range wraps the address space", what[i]);
            if (nb[i] && a < ya + yb && ya < a + nb[i]) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.%s and d_out overlap", what[i]);
        }
    }
    return BHW_OK;
}

BhwStftMfftPlan bhwp_stft_mfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                                    bool from_table)
{
    (void)p;
    BhwStftMfftPlan pl{};
    pl.route = from_table ? BHWP_FRAMES_TABLE : BHWP_FRAMES_DIRECT;
    pl.detrend = (flags & BHW_WELCH_DETREND_CONSTANT) != 0;
    pl.form = !(flags & BHW_MFFT_POWER) ? BHWP_MFFT_SPECTRUM : fb ? BHWP_MFFT_BANK : BHWP_MFFT_POWER;
    pl.len = length;
    const uint32_t n = (uint32_t)s->n_fft;
    pl.m = n / 2;
    pl.lpf = 4;
    while (pl.lpf < kFftBlock && 4u * pl.lpf < pl.m) pl.lpf *= 2;       // the smallest power of two >= M / 4
    pl.fy = kFftBlock / pl.lpf;
    pl.cpl = (n + pl.lpf - 1) / pl.lpf;
    // the schedule: 5s, 3s, 4s, a last 2
    uint32_t rest = pl.m;
    for (const uint32_t r : {5u, 3u, 4u, 2u})
        while (rest % r == 0 && pl.passes < kMfftMaxPasses) {
            pl.radix[pl.passes++] = (uint8_t)r;
            rest /= r;
        }
    pl.lds_bytes = 2u * pl.fy * pl.m * 8u + pl.m * 8u + pl.fy * 4u;
    const uint64_t K = s->n_fft / 2 + 1;
    const uint64_t W = pl.form == BHWP_MFFT_SPECTRUM ? 2 * K : pl.form == BHWP_MFFT_BANK ? fb->filters : K;
    pl.x_stride = s->x_stride ? s->x_stride : s->samples;
    pl.y_stride = s->y_stride ? s->y_stride : W;
    pl.y_bstride = s->y_batch_stride ? s->y_batch_stride : s->frames * pl.y_stride;
    pl.rows = s->batch * s->frames;
    pl.groups = (pl.rows + pl.fy - 1) / pl.fy;
    pl.grid = pl.groups < kFftMaxGrid ? pl.groups : kFftMaxGrid;
    return pl;
}

void bhwp_stft_mfft_schedule(const BhwStftMfftPlan &pl, char *buf, uint64_t len)
{
    if (!buf || !len) return;
    buf[0] = 0;
    for (uint32_t i = 0; i < pl.passes; ++i) {
        const size_t at = strlen(buf);
        if (at + 1 >= len) break;
        snprintf(buf + at, len - at, "%s%u", i ? "x" : "", (unsigned)pl.radix[i]);
    }
}

int bhwp_describe_stft_mfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                            const bhw_fbank *fb, char *buf, uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const char *route = ct ? "table" : "direct";
    const BhwStftMfftPlan pl = bhwp_stft_mfft_plan(p, length, s, flags, fb, ct != nullptr);
    const char *pad = s->pad_mode == BHW_PAD_REFLECT ? "reflect" : "constant";
    const char *det = pl.detrend ? "constant detrend" : "no detrending";
    const uint64_t K = s->n_fft / 2 + 1;
    char form[112];
    if (pl.form == BHWP_MFFT_BANK)
        snprintf(form, sizeof form, "bank rows, W = %u (%u filters, %u weights, %u filters per lane)", fb->filters, fb->filters, fb->weights,
                 (fb->filters + pl.lpf - 1) / pl.lpf);
    else if (pl.form == BHWP_MFFT_POWER) snprintf(form, sizeof form, "power rows, W = %llu", (unsigned long long)K);
    else                                 snprintf(form, sizeof form, "spectrum rows, K = %llu", (unsigned long long)K);
    if (!s->frames) {
        snprintf(buf, len, "stft mfft %s (L = %llu, n_fft %llu, %s), %s: nothing (frames 0)", route, (unsigned long long)length,
                 (unsigned long long)s->n_fft, det, form);
        return BHW_OK;
    }
    char kern[64], sched[48];
    kernel_name(p, ct, "k_stft_mfft_direct", "k_stft_mfft_table", false, kern, sizeof kern);
    bhwp_stft_mfft_schedule(pl, sched, sizeof sched);
    snprintf(buf, len, "stft mfft %s (L = %llu, n_fft %llu, col0 %llu, pad %llu %s, %s), %s: %s, %llu signals x %llu frames = %llu rows, "
             "complex FFT of %u points in passes %s + split, %u lanes per row x %u rows per workgroup, %u columns per lane, %llu groups, "
             "grid %llu x %u lanes, %u bytes of LDS", route, (unsigned long long)length, (unsigned long long)s->n_fft,
             (unsigned long long)s->col0, (unsigned long long)s->pad, pad, det, form, kern, (unsigned long long)s->batch,
             (unsigned long long)s->frames, (unsigned long long)pl.rows, pl.m, sched, pl.lpf, pl.fy, pl.cpl, (unsigned long long)pl.groups,
             (unsigned long long)pl.grid, kFftBlock, pl.lds_bytes);
    return BHW_OK;
}

// ---- fused log spectrogram, log-mel and MFCC ---------------------------------------------------------------------------------------------

uint64_t bhwp_logspec_width(const bhw_stft *s, const bhw_fbank *fb, const bhw_logspec *ls)
{
    return ls->coeffs ? ls->coeffs : fb ? fb->filters : s->n_fft / 2 + 1;
}

int bhwp_logspec_checks(bool mixed, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                        const bhw_logspec *ls, const void *d_x, const void *d_out, bool pointers)
{
    if (flags & ~BHW_WELCH_DETREND_CONSTANT)
        return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x (0 or BHW_WELCH_DETREND_CONSTANT: the power is implied)", flags);
    // the input side and the fields of fb: the parent's checks for the descriptor with packed output strides (they count other rows
    // here and are checked below)
    bhw_stft t;
    const bhw_stft *ps = packed_strides(s, t);
    int rc = mixed ? bhwp_stft_mfft_checks(p, length, ps, flags | BHW_MFFT_POWER, fb, nullptr, nullptr, false)
                   : bhwp_spectrogram_checks(p, length, ps, flags, fb, nullptr, nullptr, false);
    if (rc == BHW_ERR_UNSUPPORTED && ps == &t && s->channels == 1) {
        // the other family's n_fft: name its call
        const uint64_t n = s->n_fft;
        if (mixed && n && !(n & (n - 1)))
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu is a power of two: bhw_logspec_f32_* transforms it (one transform per n_fft)",
                             (unsigned long long)n);
        if (!mixed && bhwp_mfft_supported(n))
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu is no power of two: bhw_logspec_mfft_f32_* transforms it (one transform per n_fft)",
                             (unsigned long long)n);
    }
    if (rc) return rc;
    if (!ls) return bhwp_fail(BHW_ERR_BADARG, "log descriptor is NULL");
    if (ls->struct_size != sizeof(bhw_logspec))
        return bhwp_fail(BHW_ERR_BADARG, "bhw_logspec.struct_size %u != %zu", ls->struct_size, sizeof(bhw_logspec));
    if (ls->reserved) return bhwp_fail(BHW_ERR_BADARG, "bhw_logspec.reserved is not 0");
    if (ls->mode != BHW_LOG_CLAMP && ls->mode != BHW_LOG_ADD)
        return bhwp_fail(BHW_ERR_BADARG, "bhw_logspec.mode %u (BHW_LOG_CLAMP or BHW_LOG_ADD)", ls->mode);
    if (!std::isfinite(ls->floor) || !(ls->floor > 0.0)) return bhwp_fail(BHW_ERR_BADARG, "bhw_logspec.floor %g: finite and > 0", ls->floor);
    if (!std::isfinite(ls->mult) || ls->mult == 0.0) return bhwp_fail(BHW_ERR_BADARG, "bhw_logspec.mult %g: finite and not 0", ls->mult);
    if (ls->coeffs > kLogMaxCoeffs) return bhwp_fail(BHW_ERR_BADARG, "bhw_logspec.coeffs %u above %u", ls->coeffs, kLogMaxCoeffs);
    if (ls->coeffs) {
        if (!fb) return bhwp_fail(BHW_ERR_BADARG, "bhw_logspec.coeffs %u without a filter bank: the DCT takes bank rows", ls->coeffs);
        if (ls->dct_rows != fb->filters)
            return bhwp_fail(BHW_ERR_BADARG, "bhw_logspec.dct_rows %u: the bank has %u filters", ls->dct_rows, fb->filters);
        if (fb->filters > s->n_fft)
            return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.filters %u above n_fft %llu: the log row of a DCT waits in n_fft floats of LDS",
                             fb->filters, (unsigned long long)s->n_fft);
        if ((uint64_t)ls->dct_rows * ls->coeffs > kLogMaxDct)
            return bhwp_fail(BHW_ERR_BADARG, "bhw_logspec.dct_rows * coeffs = %llu above 2^24", (unsigned long long)ls->dct_rows * ls->coeffs);
    }
    const uint64_t T = s->samples, F = s->frames;
    if (!F) return BHW_OK;
    // the output rows: the parent's rules with W
    const uint64_t W = bhwp_logspec_width(s, fb, ls);
    if ((unsigned __int128)s->batch * F * W > (1ull << 34)) return bhwp_fail(BHW_ERR_BADARG, "batch * frames * W above 2^34 per call");
    if (s->y_stride && s->y_stride < W)
        return bhwp_fail(BHW_ERR_BADARG, "y_stride %llu: at least W = %llu floats", (unsigned long long)s->y_stride, (unsigned long long)W);
    const uint64_t ys = s->y_stride ? s->y_stride : W;
    const unsigned __int128 ysig = (unsigned __int128)(F - 1) * ys + W;
    if (ysig > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "output extent beyond 2^60 elements");
    if (s->y_batch_stride && s->y_batch_stride < (uint64_t)ysig)
        return bhwp_fail(BHW_ERR_BADARG, "y_batch_stride %llu: at least (frames - 1) * y_stride + W = %llu floats",
                         (unsigned long long)s->y_batch_stride, (unsigned long long)ysig);
    if (!pointers) return BHW_OK;
    if (!d_x || !d_out) return bhwp_fail(BHW_ERR_BADARG, "d_x / d_out is NULL");
    if ((uintptr_t)d_out % 4) return bhwp_fail(BHW_ERR_BADARG, "d_out is not 4-byte aligned");
    if ((uintptr_t)d_x % 4) return bhwp_fail(BHW_ERR_BADARG, "d_x is not 4-byte aligned");
    const uint64_t xs = s->x_stride ? s->x_stride : T, ybs = s->y_batch_stride ? s->y_batch_stride : F * ys;
    const unsigned __int128 xe = (unsigned __int128)(s->batch - 1) * xs + T, ye = (unsigned __int128)(s->batch - 1) * ybs + ysig;
    if (xe > (1ull << 60) || ye > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "x or output extent beyond 2^60 elements");
    const uint64_t xa = (uint64_t)(uintptr_t)d_x, ya = (uint64_t)(uintptr_t)d_out, xb = (uint64_t)xe * 4u, yb = (uint64_t)ye * 4u;
    if (xa > UINT64_MAX - xb || ya > UINT64_MAX - yb) return bhwp_fail(BHW_ERR_BADARG, "x or output range wraps the address space");
    if (xa < ya + yb && ya < xa + xb) return bhwp_fail(BHW_ERR_BADARG, "d_x and d_out overlap");
    uint64_t ba[3] = {0, 0, 0}, bn[3] = {0, 0, 0};
    static const char *const what[3] = {"d_first", "d_offset", "d_weight"};
    if (fb) {
        if (!fb->d_first || !fb->d_offset) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.d_first / d_offset is NULL");
        if (!fb->d_weight && fb->weights) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.d_weight is NULL with %u weights", fb->weights);
        const void *ptr[3] = {fb->d_first, fb->d_offset, fb->d_weight};
        const uint64_t nb[3] = {(uint64_t)fb->filters * 4u, ((uint64_t)fb->filters + 1u) * 4u, (uint64_t)fb->weights * 4u};
        for (int i = 0; i < 3; ++i) {
            const uint64_t a = (uint64_t)(uintptr_t)ptr[i];
            if (a % 4) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.%s is not 4-byte aligned", what[i]);
            if (a > UINT64_MAX - nb[i]) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.%s range wraps the address space", what[i]);
            if (nb[i] && a < ya + yb && ya < a + nb[i]) return bhwp_fail(BHW_ERR_BADARG, "bhw_fbank.%s and d_out overlap", what[i]);
            ba[i] = a;
            bn[i] = nb[i];
        }
    }
    if (ls->coeffs) {
        if (!ls->d_dct) return bhwp_fail(BHW_ERR_BADARG, "bhw_logspec.d_dct is NULL with %u coeffs", ls->coeffs);
        const uint64_t a = (uint64_t)(uintptr_t)ls->d_dct, n = (uint64_t)ls->dct_rows * ls->coeffs * 4u;
        if (a % 4) return bhwp_fail(BHW_ERR_BADARG, "bhw_logspec.d_dct is not 4-byte aligned");
        if (a > UINT64_MAX - n) return bhwp_fail(BHW_ERR_BADARG, "bhw_logspec.d_dct range wraps the address space");
        if (a < ya + yb && ya < a + n) return bhwp_fail(BHW_ERR_BADARG, "bhw_logspec.d_dct and d_out overlap");
        for (int i = 0; i < 3; ++i)
            if (bn[i] && a < ba[i] + bn[i] && ba[i] < a + n)
                return bhwp_fail(BHW_ERR_BADARG, "bhw_logspec.d_dct and bhw_fbank.%s overlap", what[i]);
    }
    return BHW_OK;
}

// the parent's plan with the output strides resolved for W
template <class Plan>
static Plan logspec_strides(Plan pl, const bhw_stft *s, const bhw_fbank *fb, const bhw_logspec *ls)
{
    const uint64_t W = bhwp_logspec_width(s, fb, ls);
    pl.y_stride = s->y_stride ? s->y_stride : W;
    pl.y_bstride = s->y_batch_stride ? s->y_batch_stride : s->frames * pl.y_stride;
    return pl;
}

BhwStftFftPlan bhwp_logspec_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                                 const bhw_logspec *ls, bool from_table)
{
    return logspec_strides(bhwp_spectrogram_plan(p, length, s, flags, fb, from_table), s, fb, ls);
}

BhwStftMfftPlan bhwp_logspec_mfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                                       const bhw_logspec *ls, bool from_table)
{
    return logspec_strides(bhwp_stft_mfft_plan(p, length, s, flags | BHW_MFFT_POWER, fb, from_table), s, fb, ls);
}

int bhwp_describe_logspec(bool mixed, const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                          const bhw_fbank *fb, const bhw_logspec *ls, char *buf, uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    // the parent's line: its plan fields stand in it from the kernel's name on, and stay in the parent's words
    char parent[1024];
    const int rc = mixed ? bhwp_describe_stft_mfft(p, ct, length, s, flags | BHW_MFFT_POWER, fb, parent, sizeof parent)
                         : bhwp_describe_spectrogram(p, ct, length, s, flags, fb, parent, sizeof parent);
    if (rc) return rc;
    const char *name = mixed ? "logspec mfft" : "logspec";
    const char *route = ct ? "table" : "direct";
    const char *det = (flags & BHW_WELCH_DETREND_CONSTANT) ? "constant detrend" : "no detrending";
    char stage[224], form[96];
    if (fb) snprintf(form, sizeof form, "bank rows (%u filters, %u weights)", fb->filters, fb->weights);
    else    snprintf(form, sizeof form, "power rows");
    const int at = snprintf(stage, sizeof stage, "%s, %s floor %g, mult %.17g", form, ls->mode == BHW_LOG_ADD ? "log add" : "log clamp",
                            ls->floor, ls->mult);
    if (ls->coeffs && at > 0 && (size_t)at < sizeof stage)
        snprintf(stage + at, sizeof stage - at, ", DCT %u x %u", ls->dct_rows, ls->coeffs);
    const uint64_t W = bhwp_logspec_width(s, fb, ls);
    if (!s->frames) {
        snprintf(buf, len, "%s %s (L = %llu, n_fft %llu, %s), %s, W = %llu: nothing (frames 0)", name, route, (unsigned long long)length,
                 (unsigned long long)s->n_fft, det, stage, (unsigned long long)W);
        return BHW_OK;
    }
    char kern[64];
    kernel_name(p, ct, mixed ? "k_logspec_mfft_direct" : "k_logspec_direct", mixed ? "k_logspec_mfft_table" : "k_logspec_table", false, kern,
                sizeof kern);
    // the parent's plan fields: everything after its kernel name
    const char *fields = strstr(parent, " signals x ");
    while (fields && fields > parent && fields[-1] != ' ') --fields;
    const char *pad = s->pad_mode == BHW_PAD_REFLECT ? "reflect" : "constant";
    snprintf(buf, len, "%s %s (L = %llu, n_fft %llu, col0 %llu, pad %llu %s, %s), %s, W = %llu: %s, %s", name, route, (unsigned long long)length,
             (unsigned long long)s->n_fft, (unsigned long long)s->col0, (unsigned long long)s->pad, pad, det, stage, (unsigned long long)W, kern,
             fields ? fields : "");
    return BHW_OK;
}

// ---- fused window and complex FFT for I/Q input ----------------------------------------------------------------------------------------------

// Steps 4 and 5 of the I/Q forward calls (bhw_stft_cfft_f32_*, bhw_stft_cmfft_f32_*): frames 0, the stride rules of the output form,
// the pointers.
static int iq_output_checks(const bhw_stft *s, uint32_t flags, const void *d_x, const void *d_Y, bool pointers)
{
    const uint64_t T = s->samples, F = s->frames;
    if (!F) return BHW_OK;
    const bool power = (flags & BHW_CFFT_POWER) != 0;
    const uint64_t W = power ? s->n_fft : 2 * s->n_fft;                       // floats of an output row
    const char *wname = power ? "n_fft" : "2 * n_fft";
    if (s->y_stride && (s->y_stride < W || (!power && s->y_stride % 2)))
        return bhwp_fail(BHW_ERR_BADARG, power ? "y_stride %llu: at least %s = %llu floats" : "y_stride %llu: at least %s = %llu floats, and even",
                         (unsigned long long)s->y_stride, wname, (unsigned long long)W);
    const uint64_t ys = s->y_stride ? s->y_stride : W;
    const unsigned __int128 ysig = (unsigned __int128)(F - 1) * ys + W;
    if (ysig > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "Y extent beyond 2^60 elements");
    if (s->y_batch_stride && (s->y_batch_stride < (uint64_t)ysig || (!power && s->y_batch_stride % 2)))
        return bhwp_fail(BHW_ERR_BADARG, power ? "y_batch_stride %llu: at least (frames - 1) * y_stride + %s = %llu floats"
                                               : "y_batch_stride %llu: at least (frames - 1) * y_stride + %s = %llu floats, and even",
                         (unsigned long long)s->y_batch_stride, wname, (unsigned long long)ysig);
    if (!pointers) return BHW_OK;
    if (!d_x || !d_Y) return bhwp_fail(BHW_ERR_BADARG, "d_x / d_Y is NULL");
    if ((uintptr_t)d_Y % (power ? 4 : 8)) return bhwp_fail(BHW_ERR_BADARG, "d_Y is not %d-byte aligned", power ? 4 : 8);
    if ((uintptr_t)d_x % 4) return bhwp_fail(BHW_ERR_BADARG, "d_x is not 4-byte aligned");
    const uint64_t xs = s->x_stride ? s->x_stride : 2 * T, ybs = s->y_batch_stride ? s->y_batch_stride : F * ys;
    const unsigned __int128 xe = (unsigned __int128)(s->batch - 1) * xs + 2 * T, ye = (unsigned __int128)(s->batch - 1) * ybs + ysig;
    if (xe > (1ull << 60) || ye > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "x or Y extent beyond 2^60 elements");
    const uint64_t xa = (uint64_t)(uintptr_t)d_x, ya = (uint64_t)(uintptr_t)d_Y, xb = (uint64_t)xe * 4u, yb = (uint64_t)ye * 4u;
    if (xa > UINT64_MAX - xb || ya > UINT64_MAX - yb) return bhwp_fail(BHW_ERR_BADARG, "x or Y range wraps the address space");
    if (xa < ya + yb && ya < xa + xb) return bhwp_fail(BHW_ERR_BADARG, "d_x and d_Y overlap");
    return BHW_OK;
}

// Steps 1 and 2 of the same calls: the descriptor as the frames or the segments call checks it, then the flag bits.
static int iq_descriptor_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags)
{
    int rc = bhwp_f32_checks(p, length, 0);
    if (rc) return rc;
    if (!s) return bhwp_fail(BHW_ERR_BADARG, "stft descriptor is NULL");
    if (s->struct_size != sizeof(bhw_stft)) return bhwp_fail(BHW_ERR_BADARG, "bhw_stft.struct_size %u != %zu", s->struct_size, sizeof(bhw_stft));
    // 1. what the frames or the segments call checks, for the same descriptor with packed rows (the output strides mean something
    //    else here and are checked below); this holds batch * frames * n_fft to 2^34 and the extents of x to 2^60 floats
    bhw_stft t;
    packed_strides(s, t);
    const uint32_t detrend = flags & BHW_WELCH_DETREND_CONSTANT;
    const bool segments = detrend || (!s->pad && !s->col0 && !s->pad_mode);
    if (segments) rc = bhwp_welch_checks(p, length, &t, detrend, nullptr, nullptr, nullptr, 0, false);
    else          rc = bhwp_stft_checks(p, length, &t, false, 0, nullptr, nullptr, false);
    if (rc) return rc;
    // 2.
    if (flags & ~kCfftFlags)
        return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x (BHW_WELCH_DETREND_CONSTANT, BHW_CFFT_POWER, BHW_CFFT_SHIFT)", flags);
    return BHW_OK;
}

int bhwp_stft_cfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_x, const void *d_Y,
                          bool pointers)
{
    const int rc = iq_descriptor_checks(p, length, s, flags);
    if (rc) return rc;
    // 3.
    if (s->channels != 2)
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "channels %u: the fused complex FFT takes interleaved I/Q input (2); real input: bhw_stft_fft_f32_*",
                         s->channels);
    if ((s->n_fft & (s->n_fft - 1)) || s->n_fft < (1ull << kCfftMinLog) || s->n_fft > (1ull << kCfftMaxLog))
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu: the fused complex FFT takes a power of two in %u..%u", (unsigned long long)s->n_fft,
                         1u << kCfftMinLog, 1u << kCfftMaxLog);
    // 4., 5.
    return iq_output_checks(s, flags, d_x, d_Y, pointers);
}

BhwStftCfftPlan bhwp_stft_cfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table)
{
    (void)p;
    BhwStftCfftPlan pl{};
    pl.route = from_table ? BHWP_FRAMES_TABLE : BHWP_FRAMES_DIRECT;
    pl.detrend = (flags & BHW_WELCH_DETREND_CONSTANT) != 0;
    pl.power = (flags & BHW_CFFT_POWER) != 0;
    pl.shifted = (flags & BHW_CFFT_SHIFT) != 0;
    pl.len = length;
    while ((1ull << pl.log2n) < s->n_fft) ++pl.log2n;
    pl.n = (uint32_t)s->n_fft;
    const uint32_t quarter = pl.n / 4 < 4 ? 4 : pl.n / 4;
    pl.lpf = quarter < kFftBlock ? quarter : kFftBlock;
    pl.fy = kFftBlock / pl.lpf;
    pl.cpl = pl.n / pl.lpf;
    pl.radix4 = pl.log2n / 2;
    pl.radix2 = pl.log2n % 2;
    pl.lds_bytes = 2u * pl.fy * pl.n * 8u + pl.n / 2u * 8u + pl.fy * 8u;
    pl.x_stride = s->x_stride ? s->x_stride : 2 * s->samples;
    pl.y_stride = s->y_stride ? s->y_stride : (pl.power ? s->n_fft : 2 * s->n_fft);
    pl.y_bstride = s->y_batch_stride ? s->y_batch_stride : s->frames * pl.y_stride;
    pl.rows = s->batch * s->frames;
    pl.groups = (pl.rows + pl.fy - 1) / pl.fy;
    pl.grid = pl.groups < kFftMaxGrid ? pl.groups : kFftMaxGrid;
    return pl;
}

int bhwp_describe_stft_cfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                            uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const char *route = ct ? "table" : "direct";
    const BhwStftCfftPlan pl = bhwp_stft_cfft_plan(p, length, s, flags, ct != nullptr);
    const char *pad = s->pad_mode == BHW_PAD_REFLECT ? "reflect" : "constant";
    const char *det = pl.detrend ? "constant detrend" : "no detrending";
    const char *form = pl.power ? "power rows" : "spectrum rows";
    const char *bins = pl.shifted ? "bins shifted" : "bins in order";
    if (!s->frames) {
        snprintf(buf, len, "stft cfft %s (L = %llu, n_fft %llu, %s), %s, %s: nothing (frames 0)", route, (unsigned long long)length,
                 (unsigned long long)s->n_fft, det, form, bins);
        return BHW_OK;
    }
    char kern[64], sched[48];
    kernel_name(p, ct, "k_stft_cfft_direct", "k_stft_cfft_table", false, kern, sizeof kern);
    BhwStftFftPlan f{};
    f.radix4 = pl.radix4;
    f.radix2 = pl.radix2;
    bhwp_stft_fft_schedule(f, sched, sizeof sched);
    snprintf(buf, len, "stft cfft %s (L = %llu, n_fft %llu, col0 %llu, pad %llu %s, %s), %s, %s: %s, %llu signals x %llu frames = %llu rows, "
             "complex FFT of %u points in passes %s (no split), %u lanes per row x %u rows per workgroup, %u columns per lane, %llu groups, "
             "grid %llu x %u lanes, %u bytes of LDS", route, (unsigned long long)length, (unsigned long long)s->n_fft,
             (unsigned long long)s->col0, (unsigned long long)s->pad, pad, det, form, bins, kern, (unsigned long long)s->batch,
             (unsigned long long)s->frames, (unsigned long long)pl.rows, pl.n, sched, pl.lpf, pl.fy, pl.cpl, (unsigned long long)pl.groups,
             (unsigned long long)pl.grid, kFftBlock, pl.lds_bytes);
    return BHW_OK;
}

// ---- mixed-radix fused window and complex FFT for I/Q input -------------------------------------------------------------------------------

bool bhwp_cmfft_supported(uint64_t n)
{
    if (n < kCmfftMinN || n > kCmfftMaxN || !(n & (n - 1))) return false;
    for (const uint64_t r : {2ull, 3ull, 5ull})
        while (n % r == 0) n /= r;
    return n == 1;
}

int bhwp_stft_cmfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_x, const void *d_Y,
                           bool pointers)
{
    const int rc = iq_descriptor_checks(p, length, s, flags);
    if (rc) return rc;
    // 3.: each refusal names the route that takes the call
    if (s->channels != 2)
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "channels %u: the mixed-radix fused complex FFT takes interleaved I/Q input (2); real input: "
                         "bhw_stft_mfft_f32_*", s->channels);
    if (!(s->n_fft & (s->n_fft - 1)))
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu is a power of two: bhw_stft_cfft_f32_* transforms it (one transform per n_fft)",
                         (unsigned long long)s->n_fft);
    if (!bhwp_cmfft_supported(s->n_fft))
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu: the mixed-radix fused complex FFT takes 2^a 3^b 5^c in %u..%u", (unsigned long long)s->n_fft,
                         kCmfftMinN, kCmfftMaxN);
    // 4., 5.
    return iq_output_checks(s, flags, d_x, d_Y, pointers);
}

BhwStftCmfftPlan bhwp_stft_cmfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table)
{
    (void)p;
    BhwStftCmfftPlan pl{};
    pl.route = from_table ? BHWP_FRAMES_TABLE : BHWP_FRAMES_DIRECT;
    pl.detrend = (flags & BHW_WELCH_DETREND_CONSTANT) != 0;
    pl.power = (flags & BHW_CFFT_POWER) != 0;
    pl.shifted = (flags & BHW_CFFT_SHIFT) != 0;
    pl.len = length;
    const uint32_t n = (uint32_t)s->n_fft;
    pl.n = n;
    pl.fold = (n & 1u) ? n : n / 2;
    pl.lpf = 4;
    while (pl.lpf < kFftBlock && 4u * pl.lpf < n) pl.lpf *= 2;         // the smallest power of two >= n / 4
    pl.fy = kFftBlock / pl.lpf;
    pl.cpl = (n + pl.lpf - 1) / pl.lpf;
    // the schedule: 5s, 3s, 4s, a last 2
    uint32_t rest = n;
    for (const uint32_t r : {5u, 3u, 4u, 2u})
        while (rest % r == 0 && pl.passes < kMfftMaxPasses) {
            pl.radix[pl.passes++] = (uint8_t)r;
            rest /= r;
        }
    pl.lds_bytes = 2u * pl.fy * n * 8u + pl.fold * 8u + pl.fy * 8u;
    pl.x_stride = s->x_stride ? s->x_stride : 2 * s->samples;
    pl.y_stride = s->y_stride ? s->y_stride : (pl.power ? s->n_fft : 2 * s->n_fft);
    pl.y_bstride = s->y_batch_stride ? s->y_batch_stride : s->frames * pl.y_stride;
    pl.rows = s->batch * s->frames;
    pl.groups = (pl.rows + pl.fy - 1) / pl.fy;
    pl.grid = pl.groups < kFftMaxGrid ? pl.groups : kFftMaxGrid;
    return pl;
}

int bhwp_describe_stft_cmfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                             uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const char *route = ct ? "table" : "direct";
    const BhwStftCmfftPlan pl = bhwp_stft_cmfft_plan(p, length, s, flags, ct != nullptr);
    const char *pad = s->pad_mode == BHW_PAD_REFLECT ? "reflect" : "constant";
    const char *det = pl.detrend ? "constant detrend" : "no detrending";
    const char *form = pl.power ? "power rows" : "spectrum rows";
    const char *bins = pl.shifted ? "bins shifted" : "bins in order";
    if (!s->frames) {
        snprintf(buf, len, "stft cmfft %s (L = %llu, n_fft %llu, %s), %s, %s: nothing (frames 0)", route, (unsigned long long)length,
                 (unsigned long long)s->n_fft, det, form, bins);
        return BHW_OK;
    }
    char kern[64], sched[48];
    kernel_name(p, ct, "k_stft_cmfft_direct", "k_stft_cmfft_table", false, kern, sizeof kern);
    BhwStftMfftPlan f{};
    f.passes = pl.passes;
    memcpy(f.radix, pl.radix, sizeof f.radix);
    bhwp_stft_mfft_schedule(f, sched, sizeof sched);
    snprintf(buf, len, "stft cmfft %s (L = %llu, n_fft %llu, col0 %llu, pad %llu %s, %s), %s, %s: %s, %llu signals x %llu frames = %llu rows, "
             "complex FFT of %u points in passes %s (no split), %u lanes per row x %u rows per workgroup, %u columns per lane, %llu groups, "
             "grid %llu x %u lanes, %u bytes of LDS, %u twiddles", route, (unsigned long long)length, (unsigned long long)s->n_fft,
             (unsigned long long)s->col0, (unsigned long long)s->pad, pad, det, form, bins, kern, (unsigned long long)s->batch,
             (unsigned long long)s->frames, (unsigned long long)pl.rows, pl.n, sched, pl.lpf, pl.fy, pl.cpl, (unsigned long long)pl.groups,
             (unsigned long long)pl.grid, kFftBlock, pl.lds_bytes, pl.fold);
    return BHW_OK;
}

// ---- fused Welch PSD for I/Q input --------------------------------------------------------------------------------------------------------------

uint64_t bhwp_welch_cfft_workspace_bytes(const bhw_stft *s)
{
    if (!s || !s->frames || !s->batch) return 0;
    return bhwp_welch_runs(s->batch, s->frames, 1, s->n_fft).ws_bytes;                // the bytes do not depend on fy
}

// The output side of both fused I/Q Welch calls (bhw_welch_cfft_f32_*, bhw_welch_cmfft_f32_*), after the forward call's checks passed:
// steps 2 to 7 of include/bhw.h -- the refusal of BHW_CFFT_POWER, then welch_output_checks with bins = n_fft and two floats a sample.
static int welch_iq_output_checks(const bhw_stft *s, uint32_t flags, double scale, uint64_t p_stride, const void *d_x, const void *d_P,
                                  const void *workspace, uint64_t workspace_bytes, bool pointers)
{
    // 2.
    if (flags & BHW_CFFT_POWER)
        return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x: BHW_CFFT_POWER has no meaning here (BHW_WELCH_DETREND_CONSTANT, BHW_CFFT_SHIFT)", flags);
    return welch_output_checks(s, s->n_fft, 2, "n_fft", "n_fft", scale, nullptr, p_stride, d_x, d_P, workspace, workspace_bytes, pointers);
}

int bhwp_welch_cfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint64_t p_stride,
                           const void *d_x, const void *d_P, const void *workspace, uint64_t workspace_bytes, bool pointers)
{
    // 1. the input side: the forward call's checks for the descriptor with packed output strides (no spectrum is written here)
    bhw_stft t;
    const bhw_stft *packed = packed_strides(s, t);
    const int rc = bhwp_stft_cfft_checks(p, length, packed, flags, nullptr, nullptr, false);
    if (rc) return rc;
    return welch_iq_output_checks(s, flags, scale, p_stride, d_x, d_P, workspace, workspace_bytes, pointers);
}

BhwWelchCfftPlan bhwp_welch_cfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                      bool from_table)
{
    BhwWelchCfftPlan pl{};
    bhw_stft t;
    packed_strides(s, t);
    pl.fft = bhwp_stft_cfft_plan(p, length, &t, flags & kWelchCfftFlags, from_table);
    welch_plan_runs(pl, s, s->n_fft, p_stride);
    return pl;
}

// The describe line of the calls that put stft_cfft_rows under an epilogue that owns runs: bhw_describe_welch_cfft (what "welch", the
// join k_welch_fft_join, no tail) and bhw_describe_hold_cfft (what "hold", its kernels, its join and the traces as the tail).
static int describe_cfft_runs(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                              const char *what, const char *k_direct, const char *k_table, const char *join, const char *tail, char *buf,
                              uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const char *route = ct ? "table" : "direct";
    const BhwWelchCfftPlan wp = bhwp_welch_cfft_plan(p, length, s, flags, 0, ct != nullptr);
    const BhwStftCfftPlan &pl = wp.fft;
    const char *pad = s->pad_mode == BHW_PAD_REFLECT ? "reflect" : "constant";
    const char *det = pl.detrend ? "constant detrend" : "no detrending";
    const char *bins = pl.shifted ? "bins shifted" : "bins in order";
    if (!s->frames) {
        snprintf(buf, len, "%s cfft %s (L = %llu, n_fft %llu, %s), %s: nothing (frames 0)%s", what, route, (unsigned long long)length,
                 (unsigned long long)s->n_fft, det, bins, tail);
        return BHW_OK;
    }
    char kern[64], sched[48];
    kernel_name(p, ct, k_direct, k_table, false, kern, sizeof kern);
    BhwStftFftPlan f{};
    f.radix4 = pl.radix4;
    f.radix2 = pl.radix2;
    bhwp_stft_fft_schedule(f, sched, sizeof sched);
    snprintf(buf, len, "%s cfft %s (L = %llu, n_fft %llu, col0 %llu, pad %llu %s, %s), %s: %s, %llu signals x %llu frames = %llu rows, "
             "complex FFT of %u points in passes %s (no split), %u lanes per row x %u rows per workgroup, %u columns per lane, %llu groups, "
             "grid %llu x %u lanes, %u bytes of LDS",
             what, route, (unsigned long long)length, (unsigned long long)s->n_fft, (unsigned long long)s->col0, (unsigned long long)s->pad, pad,
             det, bins, kern, (unsigned long long)s->batch, (unsigned long long)s->frames, (unsigned long long)pl.rows, pl.n, sched, pl.lpf,
             pl.fy, pl.cpl, (unsigned long long)pl.groups, (unsigned long long)pl.grid, kFftBlock, pl.lds_bytes);
    describe_runs_tail(buf, len, wp, join, tail);
    return BHW_OK;
}

int bhwp_describe_welch_cfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                             uint64_t len)
{
    return describe_cfft_runs(p, ct, length, s, flags, "welch", "k_welch_cfft_direct", "k_welch_cfft_table", "k_welch_fft_join", "", buf, len);
}

// ---- fused Welch PSD for I/Q input at mixed-radix n_fft -----------------------------------------------------------------------------------------

uint64_t bhwp_welch_cmfft_workspace_bytes(const bhw_stft *s)
{
    if (!s || !s->frames || !s->batch) return 0;
    return bhwp_welch_runs(s->batch, s->frames, 1, s->n_fft).ws_bytes;                // the bytes do not depend on fy
}

int bhwp_welch_cmfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint64_t p_stride,
                            const void *d_x, const void *d_P, const void *workspace, uint64_t workspace_bytes, bool pointers)
{
    // 1. the input side: the mixed-radix forward call's checks for the descriptor with packed output strides
    bhw_stft t;
    const bhw_stft *packed = packed_strides(s, t);
    const int rc = bhwp_stft_cmfft_checks(p, length, packed, flags, nullptr, nullptr, false);
    if (rc) return rc;
    return welch_iq_output_checks(s, flags, scale, p_stride, d_x, d_P, workspace, workspace_bytes, pointers);
}

BhwWelchCmfftPlan bhwp_welch_cmfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                        bool from_table)
{
    BhwWelchCmfftPlan pl{};
    bhw_stft t;
    packed_strides(s, t);
    pl.fft = bhwp_stft_cmfft_plan(p, length, &t, flags & kWelchCfftFlags, from_table);
    welch_plan_runs(pl, s, s->n_fft, p_stride);
    return pl;
}

// describe_cfft_runs for stft_cmfft_rows: bhw_describe_welch_cmfft and bhw_describe_hold_cmfft.
static int describe_cmfft_runs(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                               const char *what, const char *k_direct, const char *k_table, const char *join, const char *tail, char *buf,
                               uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const char *route = ct ? "table" : "direct";
    const BhwWelchCmfftPlan wp = bhwp_welch_cmfft_plan(p, length, s, flags, 0, ct != nullptr);
    const BhwStftCmfftPlan &pl = wp.fft;
    const char *pad = s->pad_mode == BHW_PAD_REFLECT ? "reflect" : "constant";
    const char *det = pl.detrend ? "constant detrend" : "no detrending";
    const char *bins = pl.shifted ? "bins shifted" : "bins in order";
    if (!s->frames) {
        snprintf(buf, len, "%s cmfft %s (L = %llu, n_fft %llu, %s), %s: nothing (frames 0)%s", what, route, (unsigned long long)length,
                 (unsigned long long)s->n_fft, det, bins, tail);
        return BHW_OK;
    }
    char kern[64], sched[48];
    kernel_name(p, ct, k_direct, k_table, false, kern, sizeof kern);
    BhwStftMfftPlan f{};
    f.passes = pl.passes;
    memcpy(f.radix, pl.radix, sizeof f.radix);
    bhwp_stft_mfft_schedule(f, sched, sizeof sched);
    snprintf(buf, len, "%s cmfft %s (L = %llu, n_fft %llu, col0 %llu, pad %llu %s, %s), %s: %s, %llu signals x %llu frames = %llu rows, "
             "complex FFT of %u points in passes %s (no split), %u lanes per row x %u rows per workgroup, %u columns per lane, %llu groups, "
             "grid %llu x %u lanes, %u bytes of LDS, %u twiddles",
             what, route, (unsigned long long)length, (unsigned long long)s->n_fft, (unsigned long long)s->col0, (unsigned long long)s->pad, pad,
             det, bins, kern, (unsigned long long)s->batch, (unsigned long long)s->frames, (unsigned long long)pl.rows, pl.n, sched, pl.lpf,
             pl.fy, pl.cpl, (unsigned long long)pl.groups, (unsigned long long)pl.grid, kFftBlock, pl.lds_bytes, pl.fold);
    describe_runs_tail(buf, len, wp, join, tail);
    return BHW_OK;
}

int bhwp_describe_welch_cmfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                              uint64_t len)
{
    return describe_cmfft_runs(p, ct, length, s, flags, "welch", "k_welch_cmfft_direct", "k_welch_cmfft_table", "k_welch_fft_join", "", buf,
                               len);
}

// ---- fused max-hold / min-hold traces for I/Q input -------------------------------------------------------------------------------------------

uint64_t bhwp_hold_cfft_workspace_bytes(const bhw_stft *s) { return bhwp_welch_cfft_workspace_bytes(s); }
uint64_t bhwp_hold_cmfft_workspace_bytes(const bhw_stft *s) { return bhwp_welch_cmfft_workspace_bytes(s); }

int bhwp_hold_traces_check(uint32_t traces)
{
    if (!traces || (traces & ~(BHW_HOLD_MAX | BHW_HOLD_MIN)))
        return bhwp_fail(BHW_ERR_BADARG, "traces 0x%x: a non-empty subset of BHW_HOLD_MAX | BHW_HOLD_MIN", traces);
    return BHW_OK;
}

// The pointers of both hold calls, after the Welch sibling's check function passed everything else (the descriptor, the flags, the
// y strides, scale, p_stride and the 2^34 bound: steps 1 to 4 of include/bhw.h): steps 5 to 7.  d_P's rules hold for each output
// and between the two.  bins: the columns of a trace row (n_fft for I/Q input, K for real input); xt: the floats of one signal (2 T
// or T); need: the sibling's workspace bytes.
static int hold_pointer_checks(const bhw_stft *s, uint64_t p_stride, uint64_t bins, uint64_t xt, uint64_t need, const void *d_x,
                               const void *d_max, const void *d_min, const void *workspace, uint64_t workspace_bytes)
{
    const uint64_t N = bins;
    if (!s->frames) return BHW_OK;
    // 5.
    if (!d_x) return bhwp_fail(BHW_ERR_BADARG, "d_x is NULL");
    if (!d_max && !d_min) return bhwp_fail(BHW_ERR_BADARG, "d_max and d_min are both NULL: no trace is asked for");
    if ((uintptr_t)d_max % 4) return bhwp_fail(BHW_ERR_BADARG, "d_max is not 4-byte aligned");
    if ((uintptr_t)d_min % 4) return bhwp_fail(BHW_ERR_BADARG, "d_min is not 4-byte aligned");
    if ((uintptr_t)d_x % 4) return bhwp_fail(BHW_ERR_BADARG, "d_x is not 4-byte aligned");
    // 6.
    if (!workspace) return bhwp_fail(BHW_ERR_BADARG, "workspace is NULL: the chunk pairs need %llu bytes", (unsigned long long)need);
    if ((uintptr_t)workspace % 8) return bhwp_fail(BHW_ERR_BADARG, "workspace is not 8-byte aligned");
    if (workspace_bytes < need)
        return bhwp_fail(BHW_ERR_WORKSPACE, "workspace of %llu bytes, the chunk and block pairs need %llu", (unsigned long long)workspace_bytes,
                         (unsigned long long)need);
    // 7. (x counts floats: xt of a signal)
    const uint64_t xs = s->x_stride ? s->x_stride : xt, ps = p_stride ? p_stride : N;
    const unsigned __int128 xe = (unsigned __int128)(s->batch - 1) * xs + xt, pe = (unsigned __int128)(s->batch - 1) * ps + N;
    if (xe > (1ull << 60) || pe > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "x or trace extent beyond 2^60 elements");
    const uint64_t xa = (uint64_t)(uintptr_t)d_x, wa = (uint64_t)(uintptr_t)workspace;
    const uint64_t xb = (uint64_t)xe * 4u, pb = (uint64_t)pe * 4u;
    const uint64_t oa[2] = {(uint64_t)(uintptr_t)d_max, (uint64_t)(uintptr_t)d_min};
    const char *const name[2] = {"d_max", "d_min"};
    if (xa > UINT64_MAX - xb || wa > UINT64_MAX - need || (d_max && oa[0] > UINT64_MAX - pb) || (d_min && oa[1] > UINT64_MAX - pb))
        return bhwp_fail(BHW_ERR_BADARG, "x, trace or workspace range wraps the address space");
    for (int i = 0; i < 2; ++i)
        if (oa[i] && xa < oa[i] + pb && oa[i] < xa + xb) return bhwp_fail(BHW_ERR_BADARG, "d_x and %s overlap", name[i]);
    if (d_max && d_min && oa[0] < oa[1] + pb && oa[1] < oa[0] + pb) return bhwp_fail(BHW_ERR_BADARG, "d_max and d_min overlap");
    if (wa < xa + xb && xa < wa + need) return bhwp_fail(BHW_ERR_BADARG, "workspace overlaps d_x");
    for (int i = 0; i < 2; ++i)
        if (oa[i] && wa < oa[i] + pb && oa[i] < wa + need) return bhwp_fail(BHW_ERR_BADARG, "workspace overlaps %s", name[i]);
    return BHW_OK;
}

int bhwp_hold_cfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint64_t p_stride,
                          const void *d_x, const void *d_max, const void *d_min, const void *workspace, uint64_t workspace_bytes,
                          bool pointers)
{
    const int rc = bhwp_welch_cfft_checks(p, length, s, flags, scale, p_stride, nullptr, nullptr, nullptr, 0, false);
    if (rc || !pointers) return rc;
    return hold_pointer_checks(s, p_stride, s->n_fft, 2 * s->samples, bhwp_welch_cfft_workspace_bytes(s), d_x, d_max, d_min, workspace,
                               workspace_bytes);
}

int bhwp_hold_cmfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint64_t p_stride,
                           const void *d_x, const void *d_max, const void *d_min, const void *workspace, uint64_t workspace_bytes,
                           bool pointers)
{
    const int rc = bhwp_welch_cmfft_checks(p, length, s, flags, scale, p_stride, nullptr, nullptr, nullptr, 0, false);
    if (rc || !pointers) return rc;
    return hold_pointer_checks(s, p_stride, s->n_fft, 2 * s->samples, bhwp_welch_cmfft_workspace_bytes(s), d_x, d_max, d_min, workspace,
                               workspace_bytes);
}

BhwHoldCfftPlan bhwp_hold_cfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                    uint32_t traces, bool from_table)
{
    return BhwHoldCfftPlan{bhwp_welch_cfft_plan(p, length, s, flags, p_stride, from_table), traces};
}

BhwHoldCmfftPlan bhwp_hold_cmfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                      uint32_t traces, bool from_table)
{
    return BhwHoldCmfftPlan{bhwp_welch_cmfft_plan(p, length, s, flags, p_stride, from_table), traces};
}

static const char *hold_traces_tail(uint32_t traces)
{
    return traces == BHW_HOLD_MAX ? "; traces: max" : traces == BHW_HOLD_MIN ? "; traces: min" : "; traces: max, min";
}

int bhwp_describe_hold_cfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                            uint32_t traces, char *buf, uint64_t len)
{
    return describe_cfft_runs(p, ct, length, s, flags, "hold", "k_hold_cfft_direct", "k_hold_cfft_table", "k_hold_join",
                              hold_traces_tail(traces), buf, len);
}

int bhwp_describe_hold_cmfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                             uint32_t traces, char *buf, uint64_t len)
{
    return describe_cmfft_runs(p, ct, length, s, flags, "hold", "k_hold_cmfft_direct", "k_hold_cmfft_table", "k_hold_join",
                               hold_traces_tail(traces), buf, len);
}

// ---- fused Welch PSD at mixed-radix n_fft -------------------------------------------------------------------------------------------------------

uint64_t bhwp_welch_mfft_workspace_bytes(const bhw_stft *s)
{
    if (!s || !s->frames || !s->batch) return 0;
    return bhwp_welch_runs(s->batch, s->frames, 1, s->n_fft / 2 + 1).ws_bytes;        // the bytes do not depend on fy
}

int bhwp_welch_mfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint32_t psd_flags,
                           uint64_t p_stride, const void *d_x, const void *d_P, const void *workspace, uint64_t workspace_bytes,
                           bool pointers)
{
    // 1. the input side: the forward call's checks for the descriptor with packed output strides (no spectrum is written here) and no
    //    bank.  BHW_MFFT_POWER is a flag that call knows: it passes here and is refused below.
    bhw_stft t;
    const bhw_stft *packed = packed_strides(s, t);
    int rc = bhwp_stft_mfft_checks(p, length, packed, flags, nullptr, nullptr, nullptr, false);
    if (rc) return rc;
    // 2.
    if (flags & BHW_MFFT_POWER)
        return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x: BHW_MFFT_POWER has no meaning here (BHW_WELCH_DETREND_CONSTANT)", flags);
    return welch_output_checks(s, s->n_fft / 2 + 1, 1, "bins", "K", scale, &psd_flags, p_stride, d_x, d_P, workspace, workspace_bytes, pointers);
}

BhwWelchMfftPlan bhwp_welch_mfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                      bool from_table)
{
    BhwWelchMfftPlan pl{};
    bhw_stft t;
    packed_strides(s, t);
    pl.fft = bhwp_stft_mfft_plan(p, length, &t, flags & BHW_WELCH_DETREND_CONSTANT, nullptr, from_table);
    welch_plan_runs(pl, s, s->n_fft / 2 + 1, p_stride);
    return pl;
}

// describe_fft_runs for stft_mfft_rows: bhw_describe_welch_mfft and bhw_describe_hold_mfft.
static int describe_mfft_runs(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                              const char *what, const char *k_direct, const char *k_table, const char *join, const char *tail, char *buf,
                              uint64_t len)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const char *route = ct ? "table" : "direct";
    const BhwWelchMfftPlan wp = bhwp_welch_mfft_plan(p, length, s, flags, 0, ct != nullptr);
    const BhwStftMfftPlan &pl = wp.fft;
    const char *pad = s->pad_mode == BHW_PAD_REFLECT ? "reflect" : "constant";
    const char *det = pl.detrend ? "constant detrend" : "no detrending";
    if (!s->frames) {
        snprintf(buf, len, "%s mfft %s (L = %llu, n_fft %llu, %s): nothing (frames 0)%s", what, route, (unsigned long long)length,
                 (unsigned long long)s->n_fft, det, tail);
        return BHW_OK;
    }
    char kern[64], sched[48];
    kernel_name(p, ct, k_direct, k_table, false, kern, sizeof kern);
    bhwp_stft_mfft_schedule(pl, sched, sizeof sched);
    snprintf(buf, len, "%s mfft %s (L = %llu, n_fft %llu, col0 %llu, pad %llu %s, %s): %s, %llu signals x %llu frames = %llu rows, "
             "complex FFT of %u points in passes %s + split, %u lanes per row x %u rows per workgroup, %u columns per lane, %llu groups, "
             "grid %llu x %u lanes, %u bytes of LDS",
             what, route, (unsigned long long)length, (unsigned long long)s->n_fft, (unsigned long long)s->col0, (unsigned long long)s->pad, pad,
             det, kern, (unsigned long long)s->batch, (unsigned long long)s->frames, (unsigned long long)pl.rows, pl.m, sched, pl.lpf, pl.fy,
             pl.cpl, (unsigned long long)pl.groups, (unsigned long long)pl.grid, kFftBlock, pl.lds_bytes);
    describe_runs_tail(buf, len, wp, join, tail);
    return BHW_OK;
}

int bhwp_describe_welch_mfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                             uint64_t len)
{
    return describe_mfft_runs(p, ct, length, s, flags, "welch", "k_welch_mfft_direct", "k_welch_mfft_table", "k_welch_fft_join", "", buf,
                              len);
}

// ---- fused max-hold / min-hold traces for real input -------------------------------------------------------------------------------------------

uint64_t bhwp_hold_fft_workspace_bytes(const bhw_stft *s) { return bhwp_welch_fft_workspace_bytes(s); }
uint64_t bhwp_hold_mfft_workspace_bytes(const bhw_stft *s) { return bhwp_welch_mfft_workspace_bytes(s); }

int bhwp_hold_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint32_t psd_flags,
                         uint64_t p_stride, const void *d_x, const void *d_max, const void *d_min, const void *workspace,
                         uint64_t workspace_bytes, bool pointers)
{
    const int rc = bhwp_welch_fft_checks(p, length, s, flags, scale, psd_flags, p_stride, nullptr, nullptr, nullptr, 0, false);
    if (rc || !pointers) return rc;
    return hold_pointer_checks(s, p_stride, s->n_fft / 2 + 1, s->samples, bhwp_welch_fft_workspace_bytes(s), d_x, d_max, d_min, workspace,
                               workspace_bytes);
}

int bhwp_hold_mfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint32_t psd_flags,
                          uint64_t p_stride, const void *d_x, const void *d_max, const void *d_min, const void *workspace,
                          uint64_t workspace_bytes, bool pointers)
{
    const int rc = bhwp_welch_mfft_checks(p, length, s, flags, scale, psd_flags, p_stride, nullptr, nullptr, nullptr, 0, false);
    if (rc || !pointers) return rc;
    return hold_pointer_checks(s, p_stride, s->n_fft / 2 + 1, s->samples, bhwp_welch_mfft_workspace_bytes(s), d_x, d_max, d_min, workspace,
                               workspace_bytes);
}

BhwHoldFftPlan bhwp_hold_fft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                  uint32_t traces, bool from_table)
{
    return BhwHoldFftPlan{bhwp_welch_fft_plan(p, length, s, flags, p_stride, from_table), traces};
}

BhwHoldMfftPlan bhwp_hold_mfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                    uint32_t traces, bool from_table)
{
    return BhwHoldMfftPlan{bhwp_welch_mfft_plan(p, length, s, flags, p_stride, from_table), traces};
}

int bhwp_describe_hold_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                           uint32_t traces, char *buf, uint64_t len)
{
    return describe_fft_runs(p, ct, length, s, flags, "hold", "k_hold_fft_direct", "k_hold_fft_table", "k_hold_join",
                             hold_traces_tail(traces), buf, len);
}

int bhwp_describe_hold_mfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                            uint32_t traces, char *buf, uint64_t len)
{
    return describe_mfft_runs(p, ct, length, s, flags, "hold", "k_hold_mfft_direct", "k_hold_mfft_table", "k_hold_join",
                              hold_traces_tail(traces), buf, len);
}

// ---- the fused inverse fronts: inverse FFT, window and overlap-add (real and I/Q output, both radix families) ----------------------------

// The first and the last step of the four checks functions; each puts its channel and n_fft refusals between them.
// The descriptor as the overlap-add checks it, for the same descriptor with packed rows (the input strides mean something else here
// and are checked by istft_io_checks).  The real pair passes the caller's whole flags, so the overlap-add refuses a foreign bit; the
// I/Q pair (iq) has the shift bit of its own: it passes the normalise bit alone and refuses foreign bits afterwards.
static int istft_descriptor_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool iq)
{
    const uint32_t ola_flags = iq ? flags & BHW_OLA_NORMALIZE : flags;
    int rc = bhwp_f32_checks(p, length, ola_flags);
    if (rc) return rc;
    if (!s) return bhwp_fail(BHW_ERR_BADARG, "stft descriptor is NULL");
    if (s->struct_size != sizeof(bhw_stft)) return bhwp_fail(BHW_ERR_BADARG, "bhw_stft.struct_size %u != %zu", s->struct_size, sizeof(bhw_stft));
    bhw_stft t;
    packed_strides(s, t);
    rc = bhwp_stft_checks(p, length, &t, true, ola_flags, nullptr, nullptr, false);
    if (rc) return rc;
    if (iq && (flags & ~kIcfftFlags)) return bhwp_fail(BHW_ERR_BADARG, "flags 0x%x (BHW_OLA_NORMALIZE, BHW_CFFT_SHIFT)", flags);
    return BHW_OK;
}

// samples 0, the stride rules of the spectrum rows, the pointers.  W: the floats of a spectrum row (2K = n_fft + 2, or 2 * n_fft),
// `row` its name in two messages; xf: the floats of an output sample (1, or 2 for I/Q).  batch * frames * W is below the overlap-add's
// cap on n_fft.
static int istft_io_checks(const bhw_stft *s, uint64_t W, const char *row, uint64_t xf, const void *d_Y, const void *d_x, bool pointers)
{
    const uint64_t T = s->samples, F = s->frames;
    if (!T) return BHW_OK;
    if (s->y_stride && (s->y_stride < W || s->y_stride % 2))
        return bhwp_fail(BHW_ERR_BADARG, "y_stride %llu: at least %s = %llu floats, and even", (unsigned long long)s->y_stride, row,
                         (unsigned long long)W);
    const uint64_t ys = s->y_stride ? s->y_stride : W;
    const unsigned __int128 ysig = (unsigned __int128)(F - 1) * ys + W;
    if (ysig > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "Y extent beyond 2^60 elements");
    if (s->y_batch_stride && (s->y_batch_stride < (uint64_t)ysig || s->y_batch_stride % 2))
        return bhwp_fail(BHW_ERR_BADARG, "y_batch_stride %llu: at least (frames - 1) * y_stride + %s = %llu floats, and even",
                         (unsigned long long)s->y_batch_stride, row, (unsigned long long)ysig);
    if (!pointers) return BHW_OK;
    if (!d_x || !d_Y) return bhwp_fail(BHW_ERR_BADARG, "d_Y / d_x is NULL");
    if ((uintptr_t)d_Y % 8) return bhwp_fail(BHW_ERR_BADARG, "d_Y is not 8-byte aligned");
    if ((uintptr_t)d_x % 4) return bhwp_fail(BHW_ERR_BADARG, "d_x is not 4-byte aligned");
    const uint64_t xs = s->x_stride ? s->x_stride : xf * T, ybs = s->y_batch_stride ? s->y_batch_stride : F * ys;
    const unsigned __int128 xe = (unsigned __int128)(s->batch - 1) * xs + xf * T, ye = (unsigned __int128)(s->batch - 1) * ybs + ysig;
    if (xe > (1ull << 60) || ye > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "x or Y extent beyond 2^60 elements");
    const uint64_t xa = (uint64_t)(uintptr_t)d_x, ya = (uint64_t)(uintptr_t)d_Y, xb = (uint64_t)xe * 4u, yb = (uint64_t)ye * 4u;
    if (xa > UINT64_MAX - xb || ya > UINT64_MAX - yb) return bhwp_fail(BHW_ERR_BADARG, "x or Y range wraps the address space");
    if (xa < ya + yb && ya < xa + xb) return bhwp_fail(BHW_ERR_BADARG, "d_Y and d_x overlap");
    return BHW_OK;
}

// The span plan of a fused inverse call (BhwIstftRuns in bhw_plan.h) with fy slots per workgroup, W floats in a spectrum row and xf
// floats in an output sample: one function for the four fronts.
static BhwIstftRuns istft_runs(uint64_t length, const bhw_stft *s, uint32_t flags, uint32_t fy, int route, uint64_t W, uint64_t xf)
{
    BhwIstftRuns pl{};
    pl.route = route;
    pl.normalize = (flags & BHW_OLA_NORMALIZE) != 0;
    pl.len = length;
    pl.x_stride = s->x_stride ? s->x_stride : xf * s->samples;
    pl.y_stride = s->y_stride ? s->y_stride : W;
    pl.y_bstride = s->y_batch_stride ? s->y_batch_stride : s->frames * pl.y_stride;
    pl.t0 = s->pad - s->col0;
    const uint64_t end = pl.t0 + s->samples;                         // <= 2^40 + 2^34
    pl.hop = s->hop < end ? s->hop : end;
    pl.halo = (length + pl.hop - 1) / pl.hop - 1;
    uint64_t fw_count = (end + pl.hop - 1) / pl.hop;                  // frames that start below the last output
    if (fw_count > s->frames) fw_count = s->frames;
    const uint64_t s_grid = (uint64_t)((unsigned __int128)s->batch * fw_count / ((uint64_t)kIfftTargetGroups * fy));
    const uint64_t s_halo = kIfftHaloFactor * pl.halo;
    uint64_t S = s_grid > s_halo ? s_grid : s_halo;
    if (S < 1) S = 1;
    if (S > fw_count) S = fw_count;
    pl.halo_bound = S > s_grid && s_grid >= 1;                       // enough rows for the grid target, were it not for the halo
    pl.span = S;
    pl.spans = (end + S * pl.hop - 1) / (S * pl.hop);
    pl.groups = (s->batch * pl.spans + fy - 1) / fy;
    pl.grid = pl.groups < kFftMaxGrid ? pl.groups : kFftMaxGrid;
    pl.trips = S + pl.halo < s->frames ? S + pl.halo : s->frames;
    return pl;
}

// What a describe line says of a family's lanes, beside the span plan.
struct IstftLanes {
    uint32_t points, lpf, fy, cpl, lds_bytes;
    uint32_t twiddles;    // the entries of the twiddle table, for the family whose line says them (cmfft's fold); 0: not said
    char sched[48];
};

// The describe line of the four fused inverse calls, next to describe_runs_tail for the forward ones.  The families differ in their
// name, their kernels, the twiddle count and, between real and I/Q output (iq), in three places: the bins phrase, whether the
// transform has a pre-split, and the library call the heavy-overlap tail names.  lanes_of(IstftLanes &) fills the lanes and returns
// the family's plan; it is not called at samples 0, where no plan exists (the hop clamp would be 0).
template <typename LanesOf>
static int describe_istft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, const char *family,
                          const char *k_direct, const char *k_table, bool iq, char *buf, uint64_t len, LanesOf lanes_of)
{
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const char *route = ct ? "table" : "direct";
    const char *norm = (flags & BHW_OLA_NORMALIZE) ? "normalised by the window envelope" : "not normalised";
    const char *bins = !iq ? "" : (flags & BHW_CFFT_SHIFT) ? ", bins shifted" : ", bins in order";
    if (!s->samples) {
        snprintf(buf, len, "istft %s %s (L = %llu, n_fft %llu), %s%s: nothing (samples 0)", family, route, (unsigned long long)length,
                 (unsigned long long)s->n_fft, norm, bins);
        return BHW_OK;
    }
    IstftLanes ln{};
    const BhwIstftRuns pl = lanes_of(ln);
    char kern[64], twiddles[32] = "", heavy[128] = "";
    kernel_name(p, ct, k_direct, k_table, false, kern, sizeof kern);
    if (ln.twiddles) snprintf(twiddles, sizeof twiddles, ", %u twiddles", ln.twiddles);
    // the repeats: every span but a signal's first transforms up to `halo` frames that the span before it transforms too (span >= 1:
    // the quotient needs no guard)
    const uint64_t repeat = pl.spans > 1 ? 100 * pl.halo / (pl.span + pl.halo) : 0;
    if (pl.halo_bound && pl.groups < kIfftTargetGroups / 4)
        snprintf(heavy, sizeof heavy, "; heavy overlap: the halo sets S and few workgroups run (%s + istft overlap-add may be faster)",
                 iq ? "ifft" : "irfft");
    snprintf(buf, len, "istft %s %s (L = %llu, n_fft %llu, col0 %llu, pad %llu: t0 = %llu), %s%s: %s, %llu signals x %llu frames = %llu rows, "
             "inverse complex FFT of %u points in %spasses %s%s, %u lanes per row x %u spans per workgroup, %u columns per lane, "
             "spans of S = %llu frames + halo %llu (%llu spans per signal, up to %llu frames a span, %llu%% of the transforms repeated), "
             "%llu groups, grid %llu x %u lanes, %u bytes of LDS%s%s", family, route, (unsigned long long)length,
             (unsigned long long)s->n_fft, (unsigned long long)s->col0, (unsigned long long)s->pad, (unsigned long long)pl.t0, norm, bins, kern,
             (unsigned long long)s->batch, (unsigned long long)s->frames, (unsigned long long)(s->batch * s->frames), ln.points,
             iq ? "" : "pre-split + ", ln.sched, iq ? " (no split)" : "", ln.lpf, ln.fy, ln.cpl, (unsigned long long)pl.span,
             (unsigned long long)pl.halo, (unsigned long long)pl.spans, (unsigned long long)pl.trips, (unsigned long long)repeat,
             (unsigned long long)pl.groups, (unsigned long long)pl.grid, kFftBlock, ln.lds_bytes, twiddles, heavy);
    return BHW_OK;
}

// the schedule text of a plan's radix fields (the forward plans' formatters)
template <typename Plan>
static void istft_fft_schedule(const Plan &pl, IstftLanes &ln)
{
    BhwStftFftPlan f{};
    f.radix4 = pl.radix4;
    f.radix2 = pl.radix2;
    bhwp_stft_fft_schedule(f, ln.sched, sizeof ln.sched);
}

template <typename Plan>
static void istft_mfft_schedule(const Plan &pl, IstftLanes &ln)
{
    BhwStftMfftPlan f{};
    f.passes = pl.passes;
    for (uint32_t i = 0; i < pl.passes; ++i) f.radix[i] = pl.radix[i];
    bhwp_stft_mfft_schedule(f, ln.sched, sizeof ln.sched);
}

// ---- fused inverse real FFT, window and overlap-add -----------------------------------------------------------------------------------------

int bhwp_istft_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_Y, const void *d_x,
                          bool pointers)
{
    const int rc = istft_descriptor_checks(p, length, s, flags, false);
    if (rc) return rc;
    if (s->channels != 1) return bhwp_fail(BHW_ERR_UNSUPPORTED, "channels %u: the fused inverse FFT gives real output (1)", s->channels);
    if ((s->n_fft & (s->n_fft - 1)) || s->n_fft < (1ull << kFftMinLog) || s->n_fft > (1ull << kFftMaxLog))
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu: the fused inverse FFT takes a power of two in %u..%u", (unsigned long long)s->n_fft,
                         1u << kFftMinLog, 1u << kFftMaxLog);
    return istft_io_checks(s, s->n_fft + 2, "2 * K", 1, d_Y, d_x, pointers);
}

BhwIstftFftPlan bhwp_istft_fft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table)
{
    // the lane layout and the radix schedule are the forward's
    bhw_stft fw = *s;
    fw.frames = 0;
    const BhwStftFftPlan f = bhwp_stft_fft_plan(p, length, &fw, 0, from_table);
    BhwIstftFftPlan pl{};
    static_cast<BhwIstftRuns &>(pl) = istft_runs(length, s, flags, f.fy, f.route, s->n_fft + 2, 1);
    pl.log2n = f.log2n;
    pl.m = f.m;
    pl.lpf = f.lpf;
    pl.fy = f.fy;
    pl.cpl = f.cpl;
    pl.radix4 = f.radix4;
    pl.radix2 = f.radix2;
    pl.lds_bytes = 2u * pl.fy * pl.m * 8u + pl.m * 8u + (uint32_t)s->n_fft * 4u;
    return pl;
}

int bhwp_describe_istft_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                            uint64_t len)
{
    return describe_istft(p, ct, length, s, flags, "fft", "k_istft_fft_direct", "k_istft_fft_table", false, buf, len, [&](IstftLanes &ln) {
        const BhwIstftFftPlan pl = bhwp_istft_fft_plan(p, length, s, flags, ct != nullptr);
        ln.points = pl.m, ln.lpf = pl.lpf, ln.fy = pl.fy, ln.cpl = pl.cpl, ln.lds_bytes = pl.lds_bytes;
        istft_fft_schedule(pl, ln);
        return static_cast<const BhwIstftRuns &>(pl);
    });
}

// ---- fused STFT, spectral mask and inverse STFT ---------------------------------------------------------------------------------------------

// a field the two descriptors must share
static int mask_fft_agree(const char *field, uint64_t a, uint64_t s)
{
    if (a == s) return BHW_OK;
    return bhwp_fail(BHW_ERR_BADARG, "%s: the analysis descriptor has %llu, the synthesis descriptor %llu (they must agree)", field,
                     (unsigned long long)a, (unsigned long long)s);
}

// What both fused masks check once each descriptor has passed its parent's checks: nonzero y strides, the seven fields that must agree,
// the gain strides, the pointers, their alignment, the extents, the wrap and the overlaps.  g_elem: the bytes of a gain, 4 (a float) or
// 8 (an interleaved float32 pair (gr, gi)); the gain strides and the gain extent count such elements.  xf: the floats of a sample of d_x
// and d_out, 1 or 2 (interleaved I/Q: K = n_fft gains a row, and the extents and overlaps of d_x and d_out count two floats a sample).
// ch: the channel axis of the filter-and-sum calls (bhw_beam_*), nullptr elsewhere: n_ch channels of d_x and of d_g stand inside one
// signal's stride, the extents of both count them, and d_out holds one signal per group of channels.
static int mask_tail_checks(const bhw_stft *sa, const bhw_stft *ss, const void *d_x, const void *d_g, uint64_t g_stride, uint64_t g_batch_stride,
                            const void *d_out, bool pointers, uint32_t g_elem, uint64_t xf = 1, const BhwBeamAxis *ch = nullptr)
{
    const char *unit = g_elem == 8u ? "pairs" : "floats";
    int rc;
    if (sa->y_stride || sa->y_batch_stride || ss->y_stride || ss->y_batch_stride)
        return bhwp_fail(BHW_ERR_BADARG, "y_stride / y_batch_stride of the %s descriptor is not 0: the fused mask has no spectrum rows",
                         (sa->y_stride || sa->y_batch_stride) ? "analysis" : "synthesis");
    if ((rc = mask_fft_agree("batch", sa->batch, ss->batch))) return rc;
    if ((rc = mask_fft_agree("frames", sa->frames, ss->frames))) return rc;
    if ((rc = mask_fft_agree("hop", sa->hop, ss->hop))) return rc;
    if ((rc = mask_fft_agree("n_fft", sa->n_fft, ss->n_fft))) return rc;
    if ((rc = mask_fft_agree("col0", sa->col0, ss->col0))) return rc;
    if ((rc = mask_fft_agree("shift", sa->shift, ss->shift))) return rc;
    if ((rc = mask_fft_agree("channels", sa->channels, ss->channels))) return rc;
    if (ch && (ch->n_ch < 1u || ch->n_ch > BHW_BEAM_MAX_CH))
        return bhwp_fail(BHW_ERR_BADARG, "n_ch %u: 1..%u channels a signal", ch->n_ch, (unsigned)BHW_BEAM_MAX_CH);
    if (!ss->samples) return BHW_OK;
    // (samples > 0: the inverse checks have refused frames 0, and with frames > 0 the forward ones samples 0 of the analysis side)
    const uint64_t K = xf == 2 ? ss->n_fft : ss->n_fft / 2 + 1, F = ss->frames, Bn = ss->batch;
    if (g_stride && g_stride < K)
        return bhwp_fail(BHW_ERR_BADARG, "g_stride %llu: 0 (one gain row for every frame) or at least K = %llu %s", (unsigned long long)g_stride,
                         (unsigned long long)K, unit);
    const unsigned __int128 gsig = (unsigned __int128)(F - 1) * g_stride + K;                // the gain rows of one signal
    if (gsig > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "g extent beyond 2^60 elements");
    const uint64_t C1 = ch ? ch->n_ch - 1u : 0, xcs = ch ? (ch->x_ch_stride ? ch->x_ch_stride : sa->samples) : 0, gcs = ch ? ch->g_ch_stride : 0;
    unsigned __int128 gall = gsig;                                                          // the gain rows of one signal, every channel
    if (ch) {
        if (ch->x_ch_stride && ch->x_ch_stride < sa->samples)
            return bhwp_fail(BHW_ERR_BADARG, "x_ch_stride %llu: 0 (packed channels) or at least the analysis samples %llu",
                             (unsigned long long)ch->x_ch_stride, (unsigned long long)sa->samples);
        const unsigned __int128 xall = (unsigned __int128)C1 * xcs + sa->samples;           // the channels of one signal
        if (xall > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "x extent beyond 2^60 elements");
        if (sa->x_stride && sa->x_stride < (uint64_t)xall)
            return bhwp_fail(BHW_ERR_BADARG, "x_stride %llu of the analysis descriptor: 0 (n_ch channel strides) or at least (n_ch - 1) * "
                             "x_ch_stride + samples = %llu", (unsigned long long)sa->x_stride, (unsigned long long)(uint64_t)xall);
        if (C1 && !gcs)
            return bhwp_fail(BHW_ERR_BADARG, "g_ch_stride 0 with n_ch %u: the same weights on every channel are a sum of the channels of x "
                             "before bhw_cmask_*; the fused beamformer takes a gain row per channel", ch->n_ch);
        if (gcs && gcs < (uint64_t)gsig)
            return bhwp_fail(BHW_ERR_BADARG, "g_ch_stride %llu: at least (frames - 1) * g_stride + K = %llu %s", (unsigned long long)gcs,
                             (unsigned long long)(uint64_t)gsig, unit);
        gall = (unsigned __int128)C1 * gcs + gsig;
        if (gall > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "g extent beyond 2^60 elements");
    }
    if (g_batch_stride && g_batch_stride < (uint64_t)gall)
        return bhwp_fail(BHW_ERR_BADARG, "g_batch_stride %llu: 0 (the same gains for every signal) or at least %s(frames - 1) * g_stride + K = "
                         "%llu %s", (unsigned long long)g_batch_stride, ch ? "(n_ch - 1) * g_ch_stride + " : "",
                         (unsigned long long)(uint64_t)gall, unit);
    if (!pointers) return BHW_OK;
    if (!d_x || !d_g || !d_out) return bhwp_fail(BHW_ERR_BADARG, "d_x / d_g / d_out is NULL");
    if ((uintptr_t)d_x % 4) return bhwp_fail(BHW_ERR_BADARG, "d_x is not 4-byte aligned");
    if (g_elem == 8u && (uintptr_t)d_g % 8)
        return bhwp_fail(BHW_ERR_BADARG, "d_g is not 8-byte aligned: the gains are interleaved float32 pairs (gr, gi), read as 8-byte words");
    if ((uintptr_t)d_g % 4) return bhwp_fail(BHW_ERR_BADARG, "d_g is not 4-byte aligned");
    if ((uintptr_t)d_out % 4) return bhwp_fail(BHW_ERR_BADARG, "d_out is not 4-byte aligned");
    const uint64_t xs = sa->x_stride ? sa->x_stride : ch ? ch->n_ch * xcs : xf * sa->samples, os = ss->x_stride ? ss->x_stride : xf * ss->samples;
    const unsigned __int128 xe = (unsigned __int128)(Bn - 1) * xs + (unsigned __int128)C1 * xcs + xf * sa->samples;
    const unsigned __int128 oe = (unsigned __int128)(Bn - 1) * os + xf * ss->samples;
    const unsigned __int128 ge = (unsigned __int128)(Bn - 1) * g_batch_stride + gall;
    if (xe > (1ull << 60) || ge > (1ull << 60) || oe > (1ull << 60)) return bhwp_fail(BHW_ERR_BADARG, "x, g or out extent beyond 2^60 elements");
    const uint64_t xa = (uint64_t)(uintptr_t)d_x, ga = (uint64_t)(uintptr_t)d_g, oa = (uint64_t)(uintptr_t)d_out;
    const uint64_t xb = (uint64_t)xe * 4u, gb = (uint64_t)ge * g_elem, ob = (uint64_t)oe * 4u;
    if (xa > UINT64_MAX - xb || ga > UINT64_MAX - gb || oa > UINT64_MAX - ob)
        return bhwp_fail(BHW_ERR_BADARG, "x, g or out range wraps the address space");
    // spans read the samples under their halo frames again: the call is not in place
    if (oa < xa + xb && xa < oa + ob) return bhwp_fail(BHW_ERR_BADARG, "d_x and d_out overlap");
    if (oa < ga + gb && ga < oa + ob) return bhwp_fail(BHW_ERR_BADARG, "d_g and d_out overlap");
    return BHW_OK;
}

// The checks of both gain types of the power-of-two family.  g_elem 4: bhw_mask_fft_f32_*, in the words they had; g_elem 8:
// bhw_cmask_fft_f32_*, whose refusals are the same sentences about "the fused complex-gain mask" and name bhw_cmask_mfft_f32_* for the
// mixed-radix lengths it takes.
// ch: bhw_beam_fft_f32_* (g_elem 8), about "the fused beamformer" and naming bhw_beam_mfft_f32_*.
static int mask_fft_checks_of(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                              const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers, uint32_t g_elem,
                              const BhwBeamAxis *ch = nullptr)
{
    int rc = bhwp_f32_checks(p, length, flags);
    if (rc) return rc;
    const char *cg = ch ? "beamformer" : g_elem == 8u ? "complex-gain mask" : "mask";
    const char *mixed_call = ch ? "bhw_beam_mfft_f32_*" : "bhw_cmask_mfft_f32_*";
    // the routes that take what this call does not: named before the parents refuse the same input in their own words
    for (const bhw_stft *s : {sa, ss}) {
        if (!s || s->struct_size != sizeof(bhw_stft)) continue;
        const char *which = s == sa ? "analysis" : "synthesis";
        if (s->channels == 2)
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "channels 2 (%s descriptor): the fused %s takes real input and gives real output; "
                             "bhw_stft_cfft_f32_* + bhw_istft_cfft_f32_* take I/Q", which, cg);
        if (s->n_fft == (1ull << kFftMaxLog))
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu (%s descriptor): the fused %s takes a power of two in %u..%u; "
                             "bhw_stft_fft_f32_* + bhw_istft_fft_f32_* take %llu", (unsigned long long)s->n_fft, which, cg, 1u << kFftMinLog,
                             1u << kMaskFftMaxLog, (unsigned long long)s->n_fft);
        if (g_elem == 8u && (s->n_fft & (s->n_fft - 1)) && s->n_fft <= kMaskMfftMaxN && bhwp_mfft_supported(s->n_fft))
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu (%s descriptor): the fused %s takes a power of two in %u..%u; "
                             "%s takes the mixed-radix lengths up to %u", (unsigned long long)s->n_fft, which, cg, 1u << kFftMinLog,
                             1u << kMaskFftMaxLog, mixed_call, kMaskMfftMaxN);
        if ((s->n_fft & (s->n_fft - 1)) && bhwp_mfft_supported(s->n_fft))
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu (%s descriptor): the fused %s takes a power of two in %u..%u; "
                             "bhw_stft_mfft_f32_* + bhw_istft_mfft_f32_* take the mixed-radix lengths", (unsigned long long)s->n_fft, which, cg,
                             1u << kFftMinLog, 1u << kMaskFftMaxLog);
    }
    // each descriptor by its parent's checks, with packed row strides (no spectrum rows exist here)
    bhw_stft ta, ts;
    rc = bhwp_stft_fft_checks(p, length, packed_strides(sa, ta), 0, nullptr, nullptr, false);
    if (rc) return rc;
    rc = bhwp_istft_fft_checks(p, length, packed_strides(ss, ts), flags, nullptr, nullptr, false);
    if (rc) return rc;
    return mask_tail_checks(sa, ss, d_x, d_g, g_stride, g_batch_stride, d_out, pointers, g_elem, 1, ch);
}

int bhwp_mask_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                         const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers)
{
    return mask_fft_checks_of(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out, pointers, 4u);
}

int bhwp_cmask_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                          const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers)
{
    return mask_fft_checks_of(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out, pointers, 8u);
}

BhwMaskFftPlan bhwp_mask_fft_plan(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                                  uint64_t g_stride, uint64_t g_batch_stride, bool from_table)
{
    BhwMaskFftPlan pl{};
    static_cast<BhwIstftFftPlan &>(pl) = bhwp_istft_fft_plan(p, length, ss, flags, from_table);
    pl.lds_bytes = 2u * pl.fy * pl.m * 8u + 2u * pl.m * 8u + (uint32_t)ss->n_fft * 4u;     // the forward table beside the inverse one
    pl.in_stride = sa->x_stride ? sa->x_stride : sa->samples;
    pl.g_stride = g_stride;
    pl.g_bstride = g_batch_stride;
    return pl;
}

// The describe line of a fused mask of `family` ("fft", "mfft") from its parent's: parent_of(line, size) writes the inverse describe
// line of ss and gives the mask plan's t0 and LDS bytes.  The parent's plan fields stand in its line from the row count on, and stay
// in the parent's words, schedule text included, but for the LDS.
struct MaskLine {
    int rc;
    uint64_t t0;
    uint32_t lds_bytes;
};
template <typename ParentOf>
static int describe_mask(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                         uint64_t g_stride, uint64_t g_batch_stride, bool pairs, const char *family, const char *k_direct, const char *k_table,
                         char *buf, uint64_t len, ParentOf parent_of, bool iq = false, const BhwBeamAxis *ch = nullptr)
{
    // "cmask ...", "complex gains: ..." (strides in pairs); with a channel axis "beam ..." and the three gain strides behind "channels C"
    const char *c = ch ? "beam" : pairs ? "cmask" : "mask", *cg = pairs ? "complex " : "";
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const char *route = ct ? "table" : "direct";
    const char *norm = (flags & BHW_OLA_NORMALIZE) ? "normalised by the window envelope" : "not normalised";
    if (!ss->samples) {
        snprintf(buf, len, "%s %s %s (L = %llu, n_fft %llu), %s: nothing (samples 0)", c, family, route, (unsigned long long)length,
                 (unsigned long long)ss->n_fft, norm);
        return BHW_OK;
    }
    char parent[1024];
    const MaskLine ml = parent_of(parent, sizeof parent);
    if (ml.rc) return ml.rc;
    char kern[64], gains[200];
    kernel_name(p, ct, k_direct, k_table, false, kern, sizeof kern);
    if (ch)
        snprintf(gains, sizeof gains, "channels %u, g_stride %llu, g_ch_stride %llu, g_batch_stride %llu", ch->n_ch, (unsigned long long)g_stride,
                 (unsigned long long)ch->g_ch_stride, (unsigned long long)g_batch_stride);
    else if (!g_stride && !g_batch_stride) snprintf(gains, sizeof gains, "one gain row for every frame and every signal");
    else if (!g_stride) snprintf(gains, sizeof gains, "one gain row for every frame, g_batch_stride %llu", (unsigned long long)g_batch_stride);
    else if (!g_batch_stride) snprintf(gains, sizeof gains, "g_stride %llu, one set of gain rows for every signal", (unsigned long long)g_stride);
    else snprintf(gains, sizeof gains, "g_stride %llu, g_batch_stride %llu", (unsigned long long)g_stride, (unsigned long long)g_batch_stride);
    if (iq) {                                                              // the I/Q masks: which bin a gain column holds
        const size_t at = strlen(gains);
        snprintf(gains + at, sizeof gains - at, ", gain columns %s", (flags & BHW_CFFT_SHIFT) ? "shifted" : "in order");
    }
    const char *fields = strstr(parent, " signals x ");
    while (fields && fields > parent && fields[-1] != ' ') --fields;
    const char *lds_end = fields ? strstr(fields, " bytes of LDS") : nullptr;
    const char *lds = lds_end;
    while (lds && lds > fields && lds[-1] != ' ') --lds;
    if (!lds) return bhwp_fail(BHW_ERR_BADARG, "buf: the inverse describe line has no plan fields");
    const char *pad = sa->pad_mode == BHW_PAD_REFLECT ? "reflect" : "constant";
    snprintf(buf, len, "%s %s %s (L = %llu, n_fft %llu, col0 %llu, pad %llu: t0 = %llu; analysis of %llu samples, pad %llu %s), %s: %s, "
             "forward + inverse FFT, %sgains: %s, %.*s%u%s", c, family, route, (unsigned long long)length, (unsigned long long)ss->n_fft,
             (unsigned long long)ss->col0, (unsigned long long)ss->pad, (unsigned long long)ml.t0, (unsigned long long)sa->samples,
             (unsigned long long)sa->pad, pad, norm, kern, cg, gains, (int)(lds - fields), fields, ml.lds_bytes, lds_end);
    return BHW_OK;
}

static int describe_mask_fft_of(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                               uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, bool pairs, char *buf, uint64_t len)
{
    return describe_mask(p, ct, length, sa, ss, flags, g_stride, g_batch_stride, pairs, "fft", pairs ? "k_cmask_fft_direct" : "k_mask_fft_direct",
                         pairs ? "k_cmask_fft_table" : "k_mask_fft_table", buf, len,
                         [&](char *parent, uint64_t size) {
                             const int rc = bhwp_describe_istft_fft(p, ct, length, ss, flags, parent, size);
                             if (rc) return MaskLine{rc, 0, 0};
                             const BhwMaskFftPlan pl = bhwp_mask_fft_plan(p, length, sa, ss, flags, g_stride, g_batch_stride, ct != nullptr);
                             return MaskLine{0, pl.t0, pl.lds_bytes};
                         });
}

int bhwp_describe_mask_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                           uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len)
{
    return describe_mask_fft_of(p, ct, length, sa, ss, flags, g_stride, g_batch_stride, false, buf, len);
}

int bhwp_describe_cmask_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                            uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len)
{
    return describe_mask_fft_of(p, ct, length, sa, ss, flags, g_stride, g_batch_stride, true, buf, len);
}

// ---- fused STFT, spectral mask and inverse STFT at mixed-radix n_fft ---------------------------------------------------------------------

// The checks of both gain types of the mixed-radix family, as mask_fft_checks_of is the power-of-two one: g_elem 8 names
// bhw_cmask_fft_f32_* for a power of two.
// ch: bhw_beam_mfft_f32_* (g_elem 8), about "the mixed-radix fused beamformer" and naming bhw_beam_fft_f32_*.
static int mask_mfft_checks_of(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                               const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers, uint32_t g_elem,
                               const BhwBeamAxis *ch = nullptr)
{
    int rc = bhwp_f32_checks(p, length, flags);
    if (rc) return rc;
    const char *cg = ch ? "beamformer" : g_elem == 8u ? "complex-gain mask" : "mask";
    const char *pow2_call = ch ? "bhw_beam_fft_f32_*" : g_elem == 8u ? "bhw_cmask_fft_f32_*" : "bhw_mask_fft_f32_*";
    // the routes that take what this call does not: named before the parents refuse the same input in their own words
    for (const bhw_stft *s : {sa, ss}) {
        if (!s || s->struct_size != sizeof(bhw_stft)) continue;
        const char *which = s == sa ? "analysis" : "synthesis";
        const bool pow2 = s->n_fft && !(s->n_fft & (s->n_fft - 1));
        if (s->channels == 2)
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "channels 2 (%s descriptor): the mixed-radix fused %s takes real input and gives real "
                             "output; bhw_stft_cmfft_f32_* + bhw_istft_cmfft_f32_* take I/Q", which, cg);
        if (pow2 && s->n_fft >= (1ull << kFftMinLog) && s->n_fft <= (1ull << kMaskFftMaxLog))
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu (%s descriptor) is a power of two: %s takes it; the mixed-radix "
                             "fused %s takes an even 2^a 3^b 5^c in %u..%u", (unsigned long long)s->n_fft, which, pow2_call, cg, kMfftMinN,
                             kMaskMfftMaxN);
        if (s->n_fft == (1ull << kFftMaxLog))
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu (%s descriptor) is a power of two: bhw_stft_fft_f32_* + bhw_istft_fft_f32_* "
                             "take it; the mixed-radix fused %s takes an even 2^a 3^b 5^c in %u..%u", (unsigned long long)s->n_fft, which,
                             cg, kMfftMinN, kMaskMfftMaxN);
        if (s->n_fft > kMaskMfftMaxN && bhwp_mfft_supported(s->n_fft))
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu (%s descriptor): the mixed-radix fused %s takes an even 2^a 3^b 5^c in "
                             "%u..%u; bhw_stft_mfft_f32_* + bhw_istft_mfft_f32_* take the larger ones", (unsigned long long)s->n_fft, which,
                             cg, kMfftMinN, kMaskMfftMaxN);
    }
    // each descriptor by its parent's checks, with packed row strides (no spectrum rows exist here)
    bhw_stft ta, ts;
    rc = bhwp_stft_mfft_checks(p, length, packed_strides(sa, ta), 0, nullptr, nullptr, nullptr, false);
    if (rc) return rc;
    rc = bhwp_istft_mfft_checks(p, length, packed_strides(ss, ts), flags, nullptr, nullptr, false);
    if (rc) return rc;
    return mask_tail_checks(sa, ss, d_x, d_g, g_stride, g_batch_stride, d_out, pointers, g_elem, 1, ch);
}

int bhwp_mask_mfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                          const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers)
{
    return mask_mfft_checks_of(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out, pointers, 4u);
}

int bhwp_cmask_mfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                           const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers)
{
    return mask_mfft_checks_of(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out, pointers, 8u);
}

BhwMaskMfftPlan bhwp_mask_mfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                                    uint64_t g_stride, uint64_t g_batch_stride, bool from_table)
{
    BhwMaskMfftPlan pl{};
    static_cast<BhwIstftMfftPlan &>(pl) = bhwp_istft_mfft_plan(p, length, ss, flags, from_table);
    pl.lds_bytes = 2u * pl.fy * pl.m * 8u + 2u * pl.m * 8u + (uint32_t)ss->n_fft * 4u;     // the forward table beside the inverse one
    pl.in_stride = sa->x_stride ? sa->x_stride : sa->samples;
    pl.g_stride = g_stride;
    pl.g_bstride = g_batch_stride;
    return pl;
}

static int describe_mask_mfft_of(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                                uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, bool pairs, char *buf, uint64_t len)
{
    return describe_mask(p, ct, length, sa, ss, flags, g_stride, g_batch_stride, pairs, "mfft", pairs ? "k_cmask_mfft_direct" : "k_mask_mfft_direct",
                         pairs ? "k_cmask_mfft_table" : "k_mask_mfft_table", buf, len,
                         [&](char *parent, uint64_t size) {
                             const int rc = bhwp_describe_istft_mfft(p, ct, length, ss, flags, parent, size);
                             if (rc) return MaskLine{rc, 0, 0};
                             const BhwMaskMfftPlan pl = bhwp_mask_mfft_plan(p, length, sa, ss, flags, g_stride, g_batch_stride, ct != nullptr);
                             return MaskLine{0, pl.t0, pl.lds_bytes};
                         });
}

int bhwp_describe_mask_mfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                            uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len)
{
    return describe_mask_mfft_of(p, ct, length, sa, ss, flags, g_stride, g_batch_stride, false, buf, len);
}

int bhwp_describe_cmask_mfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                             uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len)
{
    return describe_mask_mfft_of(p, ct, length, sa, ss, flags, g_stride, g_batch_stride, true, buf, len);
}

// ---- fused multichannel filter-and-sum: the complex-gain mask's checks, plan and line with the channel axis --------------------------------

int bhwp_beam_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                         const BhwBeamAxis &ch, const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers)
{
    return mask_fft_checks_of(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out, pointers, 8u, &ch);
}

BhwBeamFftPlan bhwp_beam_fft_plan(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                                  const BhwBeamAxis &ch, uint64_t g_stride, uint64_t g_batch_stride, bool from_table)
{
    BhwBeamFftPlan pl{};
    static_cast<BhwMaskFftPlan &>(pl) = bhwp_mask_fft_plan(p, length, sa, ss, flags, g_stride, g_batch_stride, from_table);
    pl.n_ch = ch.n_ch;
    pl.x_cstride = ch.x_ch_stride ? ch.x_ch_stride : sa->samples;
    pl.g_cstride = ch.g_ch_stride;
    pl.in_stride = sa->x_stride ? sa->x_stride : ch.n_ch * pl.x_cstride;
    return pl;
}

int bhwp_describe_beam_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                           uint32_t flags, const BhwBeamAxis &ch, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len)
{
    return describe_mask(p, ct, length, sa, ss, flags, g_stride, g_batch_stride, true, "fft", "k_beam_fft_direct", "k_beam_fft_table", buf, len,
                         [&](char *parent, uint64_t size) {
                             const int rc = bhwp_describe_istft_fft(p, ct, length, ss, flags, parent, size);
                             if (rc) return MaskLine{rc, 0, 0};
                             const BhwBeamFftPlan pl = bhwp_beam_fft_plan(p, length, sa, ss, flags, ch, g_stride, g_batch_stride, ct != nullptr);
                             return MaskLine{0, pl.t0, pl.lds_bytes};
                         }, false, &ch);
}

int bhwp_beam_mfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                         const BhwBeamAxis &ch, const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers)
{
    return mask_mfft_checks_of(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out, pointers, 8u, &ch);
}

BhwBeamMfftPlan bhwp_beam_mfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                                  const BhwBeamAxis &ch, uint64_t g_stride, uint64_t g_batch_stride, bool from_table)
{
    BhwBeamMfftPlan pl{};
    static_cast<BhwMaskMfftPlan &>(pl) = bhwp_mask_mfft_plan(p, length, sa, ss, flags, g_stride, g_batch_stride, from_table);
    pl.n_ch = ch.n_ch;
    pl.x_cstride = ch.x_ch_stride ? ch.x_ch_stride : sa->samples;
    pl.g_cstride = ch.g_ch_stride;
    pl.in_stride = sa->x_stride ? sa->x_stride : ch.n_ch * pl.x_cstride;
    return pl;
}

int bhwp_describe_beam_mfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                           uint32_t flags, const BhwBeamAxis &ch, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len)
{
    return describe_mask(p, ct, length, sa, ss, flags, g_stride, g_batch_stride, true, "mfft", "k_beam_mfft_direct", "k_beam_mfft_table", buf, len,
                         [&](char *parent, uint64_t size) {
                             const int rc = bhwp_describe_istft_mfft(p, ct, length, ss, flags, parent, size);
                             if (rc) return MaskLine{rc, 0, 0};
                             const BhwBeamMfftPlan pl = bhwp_beam_mfft_plan(p, length, sa, ss, flags, ch, g_stride, g_batch_stride, ct != nullptr);
                             return MaskLine{0, pl.t0, pl.lds_bytes};
                         }, false, &ch);
}

// ---- fused inverse mixed-radix FFT, window and overlap-add ----------------------------------------------------------------------------------

int bhwp_istft_mfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_Y, const void *d_x,
                           bool pointers)
{
    const int rc = istft_descriptor_checks(p, length, s, flags, false);
    if (rc) return rc;
    if (s->channels != 1)
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "channels %u: the mixed-radix fused inverse FFT gives real output (1)", s->channels);
    if (!(s->n_fft & (s->n_fft - 1)))
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu is a power of two: bhw_istft_fft_f32_* transforms it (one transform per n_fft)",
                         (unsigned long long)s->n_fft);
    if (!bhwp_mfft_supported(s->n_fft))
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu: the mixed-radix fused inverse FFT takes an even 2^a 3^b 5^c in %u..%u",
                         (unsigned long long)s->n_fft, kMfftMinN, kMfftMaxN);
    return istft_io_checks(s, s->n_fft + 2, "2 * K", 1, d_Y, d_x, pointers);
}

BhwIstftMfftPlan bhwp_istft_mfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table)
{
    // the lane layout and the radix schedule are the forward's
    bhw_stft fw = *s;
    fw.frames = 0;
    const BhwStftMfftPlan f = bhwp_stft_mfft_plan(p, length, &fw, 0, nullptr, from_table);
    BhwIstftMfftPlan pl{};
    static_cast<BhwIstftRuns &>(pl) = istft_runs(length, s, flags, f.fy, f.route, s->n_fft + 2, 1);
    pl.m = f.m;
    pl.lpf = f.lpf;
    pl.fy = f.fy;
    pl.cpl = f.cpl;
    pl.passes = f.passes;
    for (uint32_t i = 0; i < f.passes; ++i) pl.radix[i] = f.radix[i];
    pl.lds_bytes = 2u * pl.fy * pl.m * 8u + pl.m * 8u + (uint32_t)s->n_fft * 4u;
    return pl;
}

int bhwp_describe_istft_mfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                             uint64_t len)
{
    return describe_istft(p, ct, length, s, flags, "mfft", "k_istft_mfft_direct", "k_istft_mfft_table", false, buf, len, [&](IstftLanes &ln) {
        const BhwIstftMfftPlan pl = bhwp_istft_mfft_plan(p, length, s, flags, ct != nullptr);
        ln.points = pl.m, ln.lpf = pl.lpf, ln.fy = pl.fy, ln.cpl = pl.cpl, ln.lds_bytes = pl.lds_bytes;
        istft_mfft_schedule(pl, ln);
        return static_cast<const BhwIstftRuns &>(pl);
    });
}

// ---- fused inverse complex FFT, window and overlap-add for I/Q output ----------------------------------------------------------------------

int bhwp_istft_cfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_Y, const void *d_x,
                           bool pointers)
{
    // 1., 2. (the steps of include/bhw.h)
    const int rc = istft_descriptor_checks(p, length, s, flags, true);
    if (rc) return rc;
    // 3.
    if (s->channels != 2)
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "channels %u: the fused inverse complex FFT gives interleaved I/Q output (2); real output: "
                                              "bhw_istft_fft_f32_*", s->channels);
    if ((s->n_fft & (s->n_fft - 1)) || s->n_fft < (1ull << kCfftMinLog) || s->n_fft > (1ull << kCfftMaxLog))
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu: the fused inverse complex FFT takes a power of two in %u..%u",
                         (unsigned long long)s->n_fft, 1u << kCfftMinLog, 1u << kCfftMaxLog);
    // 4., 5.
    return istft_io_checks(s, 2 * s->n_fft, "2 * n_fft", 2, d_Y, d_x, pointers);
}

BhwIstftCfftPlan bhwp_istft_cfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table)
{
    // the lane layout and the radix schedule are the forward's
    bhw_stft fw = *s;
    fw.frames = 0;
    const BhwStftCfftPlan f = bhwp_stft_cfft_plan(p, length, &fw, 0, from_table);
    BhwIstftCfftPlan pl{};
    static_cast<BhwIstftRuns &>(pl) = istft_runs(length, s, flags, f.fy, f.route, 2 * s->n_fft, 2);
    pl.shifted = (flags & BHW_CFFT_SHIFT) != 0;
    pl.log2n = f.log2n;
    pl.n = f.n;
    pl.lpf = f.lpf;
    pl.fy = f.fy;
    pl.cpl = f.cpl;
    pl.radix4 = f.radix4;
    pl.radix2 = f.radix2;
    pl.lds_bytes = 2u * pl.fy * pl.n * 8u + pl.n / 2u * 8u + pl.n * 4u;
    return pl;
}

int bhwp_describe_istft_cfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                             uint64_t len)
{
    return describe_istft(p, ct, length, s, flags, "cfft", "k_istft_cfft_direct", "k_istft_cfft_table", true, buf, len, [&](IstftLanes &ln) {
        const BhwIstftCfftPlan pl = bhwp_istft_cfft_plan(p, length, s, flags, ct != nullptr);
        ln.points = pl.n, ln.lpf = pl.lpf, ln.fy = pl.fy, ln.cpl = pl.cpl, ln.lds_bytes = pl.lds_bytes;
        istft_fft_schedule(pl, ln);
        return static_cast<const BhwIstftRuns &>(pl);
    });
}

// ---- fused inverse mixed-radix complex FFT, window and overlap-add for I/Q output ----------------------------------------------------------

int bhwp_istft_cmfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_Y, const void *d_x,
                            bool pointers)
{
    const int rc = istft_descriptor_checks(p, length, s, flags, true);
    if (rc) return rc;
    // 3.: each refusal names the route that takes the call
    if (s->channels != 2)
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "channels %u: the mixed-radix fused inverse complex FFT gives interleaved I/Q output (2); real "
                                              "output: bhw_istft_mfft_f32_*", s->channels);
    if (!(s->n_fft & (s->n_fft - 1)))
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu is a power of two: bhw_istft_cfft_f32_* transforms it (one transform per n_fft)",
                         (unsigned long long)s->n_fft);
    if (!bhwp_cmfft_supported(s->n_fft))
        return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu: the mixed-radix fused inverse complex FFT takes 2^a 3^b 5^c in %u..%u",
                         (unsigned long long)s->n_fft, kCmfftMinN, kCmfftMaxN);
    // 4., 5.
    return istft_io_checks(s, 2 * s->n_fft, "2 * n_fft", 2, d_Y, d_x, pointers);
}

BhwIstftCmfftPlan bhwp_istft_cmfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table)
{
    // the lane layout, the radix schedule and the twiddle-table form are the forward's
    bhw_stft fw = *s;
    fw.frames = 0;
    const BhwStftCmfftPlan f = bhwp_stft_cmfft_plan(p, length, &fw, 0, from_table);
    BhwIstftCmfftPlan pl{};
    static_cast<BhwIstftRuns &>(pl) = istft_runs(length, s, flags, f.fy, f.route, 2 * s->n_fft, 2);
    pl.shifted = (flags & BHW_CFFT_SHIFT) != 0;
    pl.n = f.n;
    pl.fold = f.fold;
    pl.lpf = f.lpf;
    pl.fy = f.fy;
    pl.cpl = f.cpl;
    pl.passes = f.passes;
    for (uint32_t i = 0; i < f.passes; ++i) pl.radix[i] = f.radix[i];
    pl.lds_bytes = 2u * pl.fy * pl.n * 8u + pl.fold * 8u + pl.n * 4u;
    return pl;
}

int bhwp_describe_istft_cmfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                              uint64_t len)
{
    return describe_istft(p, ct, length, s, flags, "cmfft", "k_istft_cmfft_direct", "k_istft_cmfft_table", true, buf, len, [&](IstftLanes &ln) {
        const BhwIstftCmfftPlan pl = bhwp_istft_cmfft_plan(p, length, s, flags, ct != nullptr);
        ln.points = pl.n, ln.lpf = pl.lpf, ln.fy = pl.fy, ln.cpl = pl.cpl, ln.lds_bytes = pl.lds_bytes, ln.twiddles = pl.fold;
        istft_mfft_schedule(pl, ln);
        return static_cast<const BhwIstftRuns &>(pl);
    });
}

// ---- fused STFT, real or complex gain per bin and inverse STFT for I/Q input --------------------------------------------------------------

// The checks of the four I/Q masks: one text per family, the gain element size an argument.  The refusals that name a route come before
// the parents refuse the same input in their own words.
static int mask_cfft_checks_of(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                               const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers, uint32_t g_elem)
{
    int rc = bhwp_f32_checks(p, length, flags & BHW_OLA_NORMALIZE);
    if (rc) return rc;
    const char *cg = g_elem == 8u ? "complex-gain " : "", *c = g_elem == 8u ? "c" : "";
    for (const bhw_stft *s : {sa, ss}) {
        if (!s || s->struct_size != sizeof(bhw_stft)) continue;
        const char *which = s == sa ? "analysis" : "synthesis";
        if (s->channels == 1)
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "channels 1 (%s descriptor): the fused I/Q %smask takes interleaved I/Q input and gives "
                             "I/Q output (2); bhw_%smask_fft_f32_* takes a real signal", which, cg, c);
        if (bhwp_cmfft_supported(s->n_fft))
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu (%s descriptor): the fused I/Q %smask takes a power of two in %u..%u; "
                             "bhw_%smask_cmfft_f32_* takes the mixed-radix lengths up to %u", (unsigned long long)s->n_fft, which, cg,
                             1u << kCfftMinLog, 1u << kCfftMaxLog, c, kCmfftMaxN);
        if (s->n_fft == (2ull << kCfftMaxLog))
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu (%s descriptor): the fused I/Q %smask takes a power of two in %u..%u, the range of "
                             "bhw_stft_cfft_f32_* + bhw_istft_cfft_f32_*", (unsigned long long)s->n_fft, which, cg, 1u << kCfftMinLog,
                             1u << kCfftMaxLog);
    }
    // each descriptor by its parent's checks, with packed row strides (no spectrum rows exist here); the analysis side takes no flag
    bhw_stft ta, ts;
    rc = bhwp_stft_cfft_checks(p, length, packed_strides(sa, ta), 0, nullptr, nullptr, false);
    if (rc) return rc;
    rc = bhwp_istft_cfft_checks(p, length, packed_strides(ss, ts), flags, nullptr, nullptr, false);
    if (rc) return rc;
    return mask_tail_checks(sa, ss, d_x, d_g, g_stride, g_batch_stride, d_out, pointers, g_elem, 2);
}

static int mask_cmfft_checks_of(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                                const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers, uint32_t g_elem)
{
    int rc = bhwp_f32_checks(p, length, flags & BHW_OLA_NORMALIZE);
    if (rc) return rc;
    const char *cg = g_elem == 8u ? "complex-gain " : "", *c = g_elem == 8u ? "c" : "";
    for (const bhw_stft *s : {sa, ss}) {
        if (!s || s->struct_size != sizeof(bhw_stft)) continue;
        const char *which = s == sa ? "analysis" : "synthesis";
        const bool pow2 = s->n_fft && !(s->n_fft & (s->n_fft - 1));
        if (s->channels == 1)
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "channels 1 (%s descriptor): the mixed-radix fused I/Q %smask takes interleaved I/Q input "
                             "and gives I/Q output (2); bhw_%smask_mfft_f32_* takes a real signal", which, cg, c);
        if (pow2 && s->n_fft >= (1ull << kCfftMinLog) && s->n_fft <= (1ull << kCfftMaxLog))
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu (%s descriptor) is a power of two: bhw_%smask_cfft_f32_* takes it; the mixed-radix "
                             "fused I/Q %smask takes 2^a 3^b 5^c in %u..%u", (unsigned long long)s->n_fft, which, c, cg, kCmfftMinN, kCmfftMaxN);
        if (s->n_fft > kCmfftMaxN && s->n_fft <= 2u * kCmfftMaxN + 2u && (pow2 || bhwp_mfft_supported(s->n_fft)))
            return bhwp_fail(BHW_ERR_UNSUPPORTED, "n_fft %llu (%s descriptor): the mixed-radix fused I/Q %smask takes 2^a 3^b 5^c in %u..%u, "
                             "the range of bhw_stft_cmfft_f32_* + bhw_istft_cmfft_f32_*", (unsigned long long)s->n_fft, which, cg, kCmfftMinN,
                             kCmfftMaxN);
    }
    bhw_stft ta, ts;
    rc = bhwp_stft_cmfft_checks(p, length, packed_strides(sa, ta), 0, nullptr, nullptr, false);
    if (rc) return rc;
    rc = bhwp_istft_cmfft_checks(p, length, packed_strides(ss, ts), flags, nullptr, nullptr, false);
    if (rc) return rc;
    return mask_tail_checks(sa, ss, d_x, d_g, g_stride, g_batch_stride, d_out, pointers, g_elem, 2);
}

int bhwp_mask_cfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                          const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers)
{
    return mask_cfft_checks_of(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out, pointers, 4u);
}

int bhwp_cmask_cfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                           const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers)
{
    return mask_cfft_checks_of(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out, pointers, 8u);
}

int bhwp_mask_cmfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                           const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers)
{
    return mask_cmfft_checks_of(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out, pointers, 4u);
}

int bhwp_cmask_cmfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                            const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers)
{
    return mask_cmfft_checks_of(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out, pointers, 8u);
}

BhwMaskCfftPlan bhwp_mask_cfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                                    uint64_t g_stride, uint64_t g_batch_stride, bool from_table)
{
    BhwMaskCfftPlan pl{};
    static_cast<BhwIstftCfftPlan &>(pl) = bhwp_istft_cfft_plan(p, length, ss, flags, from_table);
    pl.lds_bytes = 2u * pl.fy * pl.n * 8u + 2u * (pl.n / 2u) * 8u + pl.n * 4u;              // the forward table beside the inverse one
    pl.in_stride = sa->x_stride ? sa->x_stride : 2 * sa->samples;
    pl.g_stride = g_stride;
    pl.g_bstride = g_batch_stride;
    return pl;
}

BhwMaskCmfftPlan bhwp_mask_cmfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                                      uint64_t g_stride, uint64_t g_batch_stride, bool from_table)
{
    BhwMaskCmfftPlan pl{};
    static_cast<BhwIstftCmfftPlan &>(pl) = bhwp_istft_cmfft_plan(p, length, ss, flags, from_table);   // one table serves both directions
    pl.in_stride = sa->x_stride ? sa->x_stride : 2 * sa->samples;
    pl.g_stride = g_stride;
    pl.g_bstride = g_batch_stride;
    return pl;
}

static int describe_mask_cfft_of(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                                uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, bool pairs, char *buf, uint64_t len)
{
    return describe_mask(p, ct, length, sa, ss, flags, g_stride, g_batch_stride, pairs, "cfft", pairs ? "k_cmask_cfft_direct" : "k_mask_cfft_direct",
                         pairs ? "k_cmask_cfft_table" : "k_mask_cfft_table", buf, len,
                         [&](char *parent, uint64_t size) {
                             const int rc = bhwp_describe_istft_cfft(p, ct, length, ss, flags, parent, size);
                             if (rc) return MaskLine{rc, 0, 0};
                             const BhwMaskCfftPlan pl = bhwp_mask_cfft_plan(p, length, sa, ss, flags, g_stride, g_batch_stride, ct != nullptr);
                             return MaskLine{0, pl.t0, pl.lds_bytes};
                         }, true);
}

static int describe_mask_cmfft_of(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                                 uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, bool pairs, char *buf, uint64_t len)
{
    return describe_mask(p, ct, length, sa, ss, flags, g_stride, g_batch_stride, pairs, "cmfft",
                         pairs ? "k_cmask_cmfft_direct" : "k_mask_cmfft_direct", pairs ? "k_cmask_cmfft_table" : "k_mask_cmfft_table", buf, len,
                         [&](char *parent, uint64_t size) {
                             const int rc = bhwp_describe_istft_cmfft(p, ct, length, ss, flags, parent, size);
                             if (rc) return MaskLine{rc, 0, 0};
                             const BhwMaskCmfftPlan pl = bhwp_mask_cmfft_plan(p, length, sa, ss, flags, g_stride, g_batch_stride, ct != nullptr);
                             return MaskLine{0, pl.t0, pl.lds_bytes};
                         }, true);
}

int bhwp_describe_mask_cfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                            uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len)
{
    return describe_mask_cfft_of(p, ct, length, sa, ss, flags, g_stride, g_batch_stride, false, buf, len);
}

int bhwp_describe_cmask_cfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                             uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len)
{
    return describe_mask_cfft_of(p, ct, length, sa, ss, flags, g_stride, g_batch_stride, true, buf, len);
}

int bhwp_describe_mask_cmfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                             uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len)
{
    return describe_mask_cmfft_of(p, ct, length, sa, ss, flags, g_stride, g_batch_stride, false, buf, len);
}

int bhwp_describe_cmask_cmfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                              uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len)
{
    return describe_mask_cmfft_of(p, ct, length, sa, ss, flags, g_stride, g_batch_stride, true, buf, len);
}

// ---- the pure entry points of the C ABI (include/bhw.h) -------------------------------------------------------------------------------
extern "C" {

uint64_t bhw_welch_csd_workspace_bytes(const bhw_csd *d)
{
    return bhwp_csd_checks(d, nullptr, nullptr, nullptr, nullptr, 0, false) ? 0 : bhwp_csd_plan(d).ws_bytes;
}

int bhw_describe_csd(const bhw_csd *d, char *buf, uint64_t len)
{
    const int rc = bhwp_csd_checks(d, nullptr, nullptr, nullptr, nullptr, 0, false);
    return rc ? rc : bhwp_describe_csd(d, buf, len);
}

uint32_t bhw_abi_version(void) { return BHW_ABI_VERSION; }

uint64_t bhw_welch_workspace_bytes(const bhw_stft *s, uint32_t flags) { return bhwp_welch_workspace_bytes(s, flags); }

uint64_t bhw_welch_psd_workspace_bytes(const bhw_psd *d)
{
    return bhwp_psd_checks(d, nullptr, nullptr, nullptr, 0, false) ? 0 : bhwp_psd_plan(d).ws_bytes;
}

const char *bhw_strerror(int code)
{
    switch (code) {
    case BHW_OK: return "ok";
    case BHW_ERR_BADARG: return "bad argument";
    case BHW_ERR_UNSUPPORTED: return "unsupported parameter combination";
    case BHW_ERR_HIP: return "HIP runtime error or no device";
    case BHW_ERR_WORKSPACE: return "workspace too small";
    default: return "unknown error";
    }
}

const char *bhw_last_error(void) { return g_last_error.c_str(); }

int bhw_coeffs_from_float(uint32_t win_type, uint32_t dat_width, const double *a, int32_t aa[7])
{
    const int K = bhwp_terms_of(win_type);
    if (!K) return bhwp_fail(BHW_ERR_BADARG, "win_type %u", win_type);
    if (dat_width < 8 || dat_width > 32) return bhwp_fail(BHW_ERR_BADARG, "dat_width %u outside 8..32", dat_width);
    if (!aa) return bhwp_fail(BHW_ERR_BADARG, "aa is NULL");
    if (!a) {
        switch (win_type) {
        case BHW_WIN_HAMMING: a = kHamming; break;
        case BHW_WIN_HANN: a = kHann; break;
        case BHW_WIN_BH3: a = kBh3; break;
        case BHW_WIN_BH4: a = kBh4; break;
        case BHW_WIN_BH5: a = kBh5; break;
        default: a = kBh7; break;
        }
    }
    // s = 1: win_function.cpp:176-177,210-212,258-261; s = 2: :312-316,349-355.  C round(): half away from zero.
    const unsigned s = (K >= 5) ? 2 : 1;
    const double scale = std::pow(2.0, (double)(dat_width - s)) - 1.0;
    for (int k = 0; k < 7; ++k) aa[k] = 0;
    for (int k = 0; k < K; ++k) {
        const double v = std::round(a[k] * scale);
        if (!(v >= -2147483648.0 && v <= 2147483647.0)) return bhwp_fail(BHW_ERR_BADARG, "weight %d (%g) does not fit int32 at dat_width %u", k, a[k], dat_width);
        aa[k] = (int32_t)(int64_t)v;
    }
    return BHW_OK;
}

int bhw_coeffs_preset(uint32_t preset, uint32_t dat_width, uint32_t *win_type, double a[7], int32_t aa[7])
{
    // hls/windows/win_function.cpp:241-250 (Nuttall, Blackman-Nuttall), :292-303 (flat-top 1 / 2), README.md:30-51
    static const struct { uint32_t win; double a[7]; } kPresets[] = {
        {0, {0}},
        {BHW_WIN_BH4, {0.355768, 0.487396, 0.144232, 0.012604}},
        {BHW_WIN_BH4, {0.3635819, 0.4891775, 0.1365995, 0.0106411}},
        {BHW_WIN_BH5, {0.25, 0.4925, 0.3225, 0.097, 0.0075}},
        {BHW_WIN_BH5, {0.215578950, 0.416631580, 0.277263158, 0.083578947, 0.006947368}},
        {BHW_WIN_BH7, {0.27105140069342, 0.43329793923448, 0.21812299954311, 0.06592544638803, 0.01081174209837,
                       0.00077658482522, 0.00001388721735}},
        {BHW_WIN_BH3, {0.42, 0.5, 0.08}},
        {BHW_WIN_BH3, {0.42323, 0.49755, 0.07922}},
    };
    if (preset < 1 || preset >= sizeof kPresets / sizeof kPresets[0]) return bhwp_fail(BHW_ERR_BADARG, "preset %u", preset);
    if (win_type) *win_type = kPresets[preset].win;
    if (a) memcpy(a, kPresets[preset].a, 7 * sizeof(double));
    if (aa) return bhw_coeffs_from_float(kPresets[preset].win, dat_width, kPresets[preset].a, aa);
    return BHW_OK;
}

int bhw_params_init(bhw_params *p, uint32_t win_type, uint32_t phi_width, uint32_t dat_width)
{
    if (!p) return bhwp_fail(BHW_ERR_BADARG, "params is NULL");
    memset(p, 0, sizeof *p);
    p->struct_size = sizeof *p;
    p->model = BHW_MODEL_HLS;
    p->combine = BHW_COMBINE_HLS;
    p->sin_type = BHW_SIN_CORDIC;
    p->win_type = win_type;
    p->n_terms = (uint32_t)bhwp_terms_of(win_type);
    p->phi_width = phi_width;
    p->dat_width = dat_width;
    p->precision = 1;
    p->lut_size = 9;
    if (!p->n_terms) return bhwp_fail(BHW_ERR_BADARG, "win_type %u", win_type);
    int rc = bhw_coeffs_from_float(win_type, dat_width, nullptr, p->aa);
    if (rc) return rc;
    return bhwp_validate(p);
}

int bhw_params_validate(const bhw_params *p) { return bhwp_validate(p); }

int bhw_constant_tables(uint32_t which, int64_t table[48], int64_t gains[2])
{
    if (which > 1) return bhwp_fail(BHW_ERR_BADARG, "which %u", which);
    if (table) memcpy(table, which ? kAtanT4 : kAtanT2, 48 * sizeof(int64_t));
    if (gains) { gains[0] = kGain46; gains[1] = kGain47; }
    return BHW_OK;
}

// Upper bound over every table format the call may use (8 bytes per table entry: the plain format).  bhw_workspace_bytes_ex
// gives the figure for the format the call would use right now.
uint64_t bhw_workspace_bytes(const bhw_params *p, uint64_t n0, uint64_t count, uint32_t algo)
{
    if (bhwp_validate(p)) return 0;
    if (p->sin_type != BHW_SIN_CORDIC) return 0;
    BhwCordicCfg c;
    bhwp_resolve_cordic(p, c);
    BhwWinCfg w;
    bhwp_resolve_window(p, w);
    return bhwp_pick_algo(p, c, w, n0, count, algo) == BHW_ALGO_TABLE ? bhwp_table_entries(c) * 8ull : 0;
}

uint64_t bhw_workspace_bytes_ex(const bhw_params *p, uint64_t n0, uint64_t count, const bhw_exec *ex)
{
    if (bhwp_validate(p) || bhwp_check_exec(ex)) return 0;
    if (p->sin_type != BHW_SIN_CORDIC) return 0;
    BhwCordicCfg c;
    bhwp_resolve_cordic(p, c);
    BhwWinCfg w;
    bhwp_resolve_window(p, w);
    if (bhwp_pick_algo(p, c, w, n0, count, ex ? ex->algo : (uint32_t)BHW_ALGO_AUTO) != BHW_ALGO_TABLE) return 0;
    const BhwTableCall t = bhwp_table_call(p, c, w, n0, count, false);
    return bhwp_format_walk(p, c, t.tiled, bhwp_exec_table_format(ex), false).scratch_bytes;
}

int bhw_describe_plan(const bhw_params *p, uint64_t n0, uint64_t count, const bhw_exec *ex, char *buf, uint64_t len)
{
    int rc = bhwp_validate(p);
    if (rc) return rc;
    rc = bhwp_check_exec(ex);
    if (rc) return rc;
    if (!buf || !len) return bhwp_fail(BHW_ERR_BADARG, "buf is NULL or empty");
    const bool period = bhwp_has_whole_period(p, n0, count);
    if (p->sin_type != BHW_SIN_CORDIC) {
        snprintf(buf, len, "taylor: %s", period && p->phi_width >= 5 ? "k_taylor_window_fold (+ k_taylor_window on ragged ends)" : "k_taylor_window");
        return BHW_OK;
    }
    BhwCordicCfg c;
    bhwp_resolve_cordic(p, c);
    BhwWinCfg w;
    bhwp_resolve_window(p, w);
    const uint32_t algo = bhwp_pick_algo(p, c, w, n0, count, ex ? ex->algo : (uint32_t)BHW_ALGO_AUTO);
    if (algo == BHW_ALGO_DIRECT) {
        snprintf(buf, len, "direct: %s", direct_form(c) == 2 ? "k_direct_fast" : "k_direct");
        return BHW_OK;
    }
    if (algo == BHW_ALGO_FUSED) {
        // one launch over the whole ring [0, N/8) per period: the form bhwk_fold_direct picks for that many lanes
        const int form = bhwp_fold_form(c, w, 1ull << (p->phi_width - 3));
        if (form == BHWP_FOLD_SPLIT) snprintf(buf, len, "fused: k_fold_split<%u,%d,%u> (+ k_direct_fast on ragged ends)", p->n_terms, mode_of(c, w), (unsigned)fold_chains((int)p->n_terms));
        else snprintf(buf, len, "fused: k_fold_direct<%u,%d,%d> (+ k_direct_fast on ragged ends)", p->n_terms, mode_of(c, w), form);
        return BHW_OK;
    }
    const BhwTableCall t = bhwp_table_call(p, c, w, n0, count, false);
    c.tab_split = (t.tiled && c.z_shr == 0) ? 1u : 0u;
    // the format the call builds first: the narrowest one still open (tried with the check word), else the one known exact
    const BhwFormatWalk fw = bhwp_format_walk(p, c, t.tiled, bhwp_exec_table_format(ex), false);
    c.tab_dlog = fw.n_open ? fw.open[0] : fw.kept;
    char build[64], combine[96];
    bhwk_describe_table(c, w, t.tiled, t.images, build, combine, sizeof build);
    if (period && c.tab_dlog == 0 && bhwk_runlength_applicable(c, w, nullptr))     // generate_impl's period(): dropped phase bits
        snprintf(combine, sizeof combine, "k_runlength_window<%u,%d,%s> (16-byte aligned output; else k_table_combine_fold_t)", p->n_terms,
                 mode_of(c, w), rl_narrow(c) ? "true" : "false");
    snprintf(buf, len, "table[%s%s]: %s + %s%s", bhwp_format_name(c.tab_dlog), fw.n_open ? ", unverified" : "", build, (period || t.images) ? combine : "k_table_combine",
             t.images ? " (image subset)" : period && count != (1ull << p->phi_width) ? " (+ k_table_combine / k_replicate on the rest)" : "");
    return BHW_OK;
}

int bhw_part_segments(const bhw_params *p, uint32_t part, uint32_t n_parts, bhw_segment *segs, uint32_t capacity, uint32_t *n_segs)
{
    int rc = bhwp_part_checks(p, part, n_parts);
    if (rc) return rc;
    if (!n_segs) return bhwp_fail(BHW_ERR_BADARG, "n_segs is NULL");
    BhwCordicCfg c;
    bhwp_resolve_cordic(p, c);
    BhwWinCfg w;
    bhwp_resolve_window(p, w);
    BhwFoldRun runs[32];
    uint32_t t0, tc;
    const int n_runs = bhwk_part_runs(c, w, part, n_parts, runs, &t0, &tc);
    std::vector<bhw_segment> all;
    const uint64_t H = 1ull << (p->phi_width - 3);
    for (int i = 0; i < n_runs; ++i)
        for (uint64_t img = 0; img < 8; ++img)
            all.push_back(bhw_segment{runs[i].r0 + img * H, (uint64_t)(runs[i].r_end - runs[i].r0)});
    // sorted, touching or overlapping segments merged
    for (size_t i = 1; i < all.size(); ++i)
        for (size_t j = i; j > 0 && all[j - 1].n0 > all[j].n0; --j) std::swap(all[j - 1], all[j]);
    std::vector<bhw_segment> merged;
    for (const bhw_segment &sg : all) {
        if (!merged.empty() && sg.n0 <= merged.back().n0 + merged.back().count) {
            const uint64_t end = sg.n0 + sg.count;
            if (end > merged.back().n0 + merged.back().count) merged.back().count = end - merged.back().n0;
        } else merged.push_back(sg);
    }
    *n_segs = (uint32_t)merged.size();
    if (segs) {
        if (capacity < merged.size()) return bhwp_fail(BHW_ERR_BADARG, "capacity %u < %zu segments", capacity, merged.size());
        for (size_t i = 0; i < merged.size(); ++i) segs[i] = merged[i];
    }
    return BHW_OK;
}

// Verdict cache of the packed formats (0 unknown, 1 exact, 2 overflows); set != 0 overrides it (tests of the fallback).
int bhw_dbg_table_format_verdict(const bhw_params *p, uint32_t dlog, int set)
{
    if (bhwp_validate(p)) return BHW_ERR_BADARG;
    if (set) bhwp_fmt_set_verdict(p, dlog, set);
    return bhwp_fmt_verdict(p, dlog);
}

// The key check of the resident tables on its own (no device): BHW_OK when a table built from p_table serves calls with p_call.
int bhw_dbg_table_key_matches(const bhw_params *p_table, const bhw_params *p_call)
{
    int rc = bhwp_table_create_checks(p_table, BHW_TABLE_BEST);
    if (!rc) rc = bhwp_validate(p_call);
    return rc ? rc : bhwp_table_key_check(p_table, p_call);
}

// The describe hooks below: their checks, and the table of p_table as bhw_table_create would hold it if every packed format under
// `table_format` were exact (the first candidate).
static int dbg_resident_table(const bhw_params *p_table, uint32_t table_format, const bhw_params *p_call, BhwCordicCfg &c, bool *tiled)
{
    int rc = bhw_dbg_table_key_matches(p_table, p_call);
    if (!rc && table_format > BHW_TABLE_NIBBLE_ESC) rc = bhwp_fail(BHW_ERR_BADARG, "table_format %u", table_format);
    if (rc) return rc;
    bhwp_resident_layout(p_table, c, tiled);
    uint32_t cand[kMaxFormats];
    bhwp_table_format_candidates(c, *tiled, table_format, cand);
    c.tab_dlog = cand[0];
    return BHW_OK;
}

// bhw_table_describe from parameters alone (no device, no table): the kernels a call of (p_call, n0, count) launches over that table.
int bhw_dbg_describe_from_table(const bhw_params *p_table, uint32_t table_format, const bhw_params *p_call, uint64_t n0, uint64_t count,
                                char *buf, uint64_t len)
{
    BhwCordicCfg c;
    bool tiled;
    const int rc = dbg_resident_table(p_table, table_format, p_call, c, &tiled);
    return rc ? rc : bhwp_describe_from_table(p_call, c, tiled, n0, count, buf, len);
}

// bhw_apply_frames_describe of a from-table call from parameters alone (no device, no table), over that table.
int bhw_dbg_describe_frames_from_table(const bhw_params *p_table, uint32_t table_format, const bhw_params *p_call, const bhw_frames *f,
                                       char *buf, uint64_t len)
{
    BhwCordicCfg c;
    bool tiled;
    int rc = dbg_resident_table(p_table, table_format, p_call, c, &tiled);
    if (!rc) rc = bhwp_frames_checks(p_call, f, nullptr, nullptr, false);
    return rc ? rc : bhwp_describe_frames(p_call, &c, f, buf, len);
}

// bhw_overlap_add_describe of a from-table call from parameters alone (no device, no table), over that table.
int bhw_dbg_describe_ola_from_table(const bhw_params *p_table, uint32_t table_format, const bhw_params *p_call, const bhw_ola *o,
                                    char *buf, uint64_t len)
{
    BhwCordicCfg c;
    bool tiled;
    int rc = dbg_resident_table(p_table, table_format, p_call, c, &tiled);
    if (!rc) rc = bhwp_ola_checks(p_call, o, nullptr, nullptr, false);
    return rc ? rc : bhwp_describe_ola(p_call, &c, o, buf, len);
}

// tab_dlog the residual format would use for `p` (0: not applicable) and whether delta16 applies
int bhw_dbg_table_format_info(const bhw_params *p, uint32_t *resid_dlog, uint32_t *delta16_ok)
{
    if (bhwp_validate(p)) return BHW_ERR_BADARG;
    BhwCordicCfg c;
    bhwp_resolve_cordic(p, c);
    if (resid_dlog) *resid_dlog = c.n_iter >= 21 ? bhwk_resid_dlog(c) : 0u;
    if (delta16_ok) *delta16_ok = (c.n_iter >= 21 && bhwk_packed_ok(c)) ? 1u : 0u;
    return BHW_OK;
}

} // extern "C"
