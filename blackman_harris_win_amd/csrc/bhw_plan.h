// bhw_plan.h -- the HIP-free half of the host side: everything the library decides from parameters alone.
//
// Parameter validation, resolution of a (model, widths) tuple into kernel constants, strategy and table-format choice, the
// tile plan of the combine pass, ownership parts and their segments, scratch sizing, and the text of bhw_describe_plan.  No
// hip* include and no device state: bhw_plan.cpp compiles with a plain C++ compiler and runs under AddressSanitizer / UBSan over
// the whole parameter lattice (tests/test_sanitizers.py), which the launch code in bhw_api.cpp and the kernel units cannot.
// The kernel units include this header (through bhw_device.h) for the shapes they share with the planner.
//
// Host mirror of the reference's own host code: cpp/cordic_sincos.cpp:12-36 derives the rescaled ROM, gain and z scaling per
// call; hls/windows/win_function.cpp:74-96 does the same for the HLS model; src/cordic_dds.vhd:97-131,159-166 at elaboration.
#pragma once
#include "bhw_internal.h"

#if defined(__HIPCC__)
#define BHW_HD __host__ __device__
#else
#define BHW_HD
#endif
#include "bhw_len.h"

// ---- table formats (bhw_device.h documents the encodings) -----------------------------------------------------------------------
constexpr uint32_t kPackLog = 6;                // cfg.tab_dlog = 6: delta16
constexpr uint32_t kNibbleFlag = 16;            // cfg.tab_dlog = kNibbleFlag + d: nibble; d = 7..9 alone: residual; 0: plain
constexpr uint32_t kEscFlag = 32;               // cfg.tab_dlog = kEscFlag + kNibbleFlag + d: nibble with escapes (format 5)
constexpr uint32_t kEscSlots = 128;             // escape table of one build workgroup: open addressing, one int4 {entry, c, s, -} per slot
constexpr uint32_t kEscBias = 1;                // ... records carry c + 1, s + 1: the chord of a concave arc lies below it, and the deviations lean positive
constexpr uint32_t kEscFill = 96;               // ... entries it may hold before the format is refused (cpp at 2^26 / 32 bits: 547 in all, at most 36 in one)
BHW_HD constexpr uint32_t fmt_cell_log(uint32_t tab_dlog) { return tab_dlog & (kNibbleFlag - 1u); }
BHW_HD constexpr int fmt_of(uint32_t tab_dlog) { return tab_dlog == 0 ? 0 : tab_dlog == kPackLog ? 1 : tab_dlog >= kEscFlag ? 5 : tab_dlog >= kNibbleFlag ? 3 : 2; }

BHW_HD constexpr bool fmt_is_resid(int fmt) { return fmt == 2 || fmt == 3 || fmt == 5; }     // straight-line records + a deviation per entry
BHW_HD constexpr bool fmt_is_nibble(int fmt) { return fmt == 3 || fmt == 5; }               // ... in one byte, natural layout

// The layout goes with the format: nibble tables are always in the natural order (resid_offset), whatever the caller asked for.
inline BhwCordicCfg table_layout(const BhwCordicCfg &c)
{
    BhwCordicCfg n = c;
    if (fmt_of(c.tab_dlog) == 3 || fmt_of(c.tab_dlog) == 5) n.tab_split = 0u;
    return n;
}

// One table inside a scratch buffer: [ entries | records or block heads at coarse_off | check word at check_off ], each part
// 256-byte aligned.  bytes = what a call in this format needs.
struct BhwTableLayout {
    uint64_t coarse_off, check_off, bytes;
    uint64_t esc_off;       // nibble + escapes: the per-workgroup escape lists (0 otherwise)
    uint32_t esc_wg_log;    // ... log2 of the entries one build workgroup owns
};
BhwTableLayout bhwp_table_layout(uint64_t entries, uint32_t tab_dlog);

// ---- shapes shared with the kernels ---------------------------------------------------------------------------------------------
constexpr int kTileThreads = 960;   // combine pass, 15-run tiles: 5 thread groups x 192 lanes (bhw_combine.hip)
constexpr int kTileLanes = 192;
constexpr int kRlRun = 16;          // run-length kernel: consecutive ring lanes per thread, threads per workgroup
constexpr int kRlBlock = 64;
constexpr int kFoldRunsMax = 32;    // fused kernel: runs per launch, threads per workgroup
constexpr int kFoldBlock = 256;

// Kernel forms: each rule is read by the launcher, as a template argument, and by the describe strings that name the instance.
// cosine-sum rule of the combine kernels (MODE): 0 HLS rule, 1 HLS rule with the one's-complement quadrant map (cpp model), 2 VHDL rule
inline int mode_of(const BhwCordicCfg &c, const BhwWinCfg &w) { return (w.combine != BHW_COMBINE_HLS) ? 2 : (c.ones_neg ? 1 : 0); }
// direct CORDIC (k_direct, k_sincos, k_frames_direct, k_ola_direct): 2 the mad-form rotation (|x| < 2^33, quarter circle <= 2^32;
// k_direct_fast, k_sincos_fast), else 1 the 64-bit state or 0 the 32-bit state
inline int direct_form(const BhwCordicCfg &c) { return (c.dat_width + c.out_shr <= 34 && c.n_iter >= 7) ? 2 : c.wide ? 1 : 0; }
// run-length kernel (k_runlength_window NARROW): coefficients fit int16, half-size LDS tile
inline bool rl_narrow(const BhwCordicCfg &c) { return c.dat_width <= 16; }
// fused kernel, split form (k_fold_split NCH): first-quadrant chains per ring lane, one wave each
BHW_HD constexpr int fold_chains(int n_terms) { return n_terms == 2 ? 2 : n_terms == 3 ? 3 : n_terms == 4 ? 5 : n_terms == 5 ? 6 : 9; }

struct BhwTilePlan {
    uint32_t offs[16];   // (i3*inv3 + i5*inv5) mod ring, index i3 + 3*i5; padded by repeating the last run
    uint32_t n_tiles;    // tiles that cover the ring once
    uint32_t tile0;      // first tile of this launch (interleaved ownership parts launch a sub-range of the tiles)
    uint32_t img_mask;   // MASKED instances: bit 2j + h set = image (h, j), i.e. stream indices [(2j + h) N/8, +N/8), is wanted
    uint32_t n0mod;      // MASKED instances: stream index (mod N) that `out` points at; image m lands at ((m N/8 - n0mod) mod N)
};
// The tile plan of a configuration: run offsets on the ring [0, N/8), runs per tile (1, 3 or 15), lanes per run, tiles that cover the ring.
void bhwp_tile_plan(const BhwCordicCfg &c, const BhwWinCfg &w, BhwTilePlan &tp, int &nb, uint32_t &lanes);
// one-instruction products in the 15-run tile kernel (tile_harmonic FAST) for these weights and this cosine-sum rule
bool bhwp_tile_fast(const BhwCordicCfg &c, const BhwWinCfg &w, int nb);
// k_tile9 (bhw_tile9.hip), the 15-run tile kernel compiled for one-byte tables with cells of 2^9 entries: applies to whole 15-run
// tiles with one-instruction products and all eight images, where it measured faster (everything else: k_table_combine_tile)
constexpr uint32_t kTile9CellLog = 9;
bool bhwk_tile9_applicable(const BhwCordicCfg &c, const BhwWinCfg &w, int nb, bool fast, bool masked);
int bhwk_tile9(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwTilePlan &tp, uint32_t tile_count, const int32_t *d_table, int32_t *d_out);

// Form of the fused kernel for a launch of `total` ring lanes: which kernel bhwk_fold_direct starts (and bhw_describe_plan names).
enum { BHWP_FOLD_SEQUENTIAL = 0, BHWP_FOLD_LOCKSTEP = 1, BHWP_FOLD_NARROW = 2, BHWP_FOLD_SPLIT = 3 };
int bhwp_fold_form(const BhwCordicCfg &c, const BhwWinCfg &w, uint64_t total);
// first rotation from which x >> k and the ROM word fit the 24-bit factors of v_mad_i32_i24 (narrow form)
uint32_t bhwp_fold_k24(const BhwCordicCfg &c);

// workgroup size of the octant-mirror build kernel for a table of `entries`
unsigned bhwk_build_mirror_threads(uint32_t entries);

// ---- resolution, validation, strategy -------------------------------------------------------------------------------------------
int  bhwp_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));   // sets the thread's bhw_last_error() text, returns code
int  bhwp_terms_of(uint32_t win_type);
int  bhwp_validate(const bhw_params *p, bool sincos_only = false);
int  bhwp_validate_atan2(const bhw_atan2_params *p);
void bhwp_resolve_cordic(const bhw_params *p, BhwCordicCfg &c);
void bhwp_resolve_window(const bhw_params *p, BhwWinCfg &w);
void bhwp_resolve_prerot(const bhw_params *p, BhwPrerotCfg &c);
void bhwp_resolve_atan2(const bhw_atan2_params *p, BhwAtan2Cfg &c);
inline uint64_t bhwp_table_entries(const BhwCordicCfg &c) { return 1ull << (c.phi_width - 2 - c.z_shr); }
bool bhwp_has_whole_period(const bhw_params *p, uint64_t n0, uint64_t count);
// Argument checks of bhw_apply_device / bhw_apply_from_table, before any other: BHW_OK or BADARG.
int  bhwp_apply_checks(uint64_t count, const void *d_x, const void *d_y, uint32_t shift);
uint32_t bhwp_pick_algo(const bhw_params *p, const BhwCordicCfg &c, const BhwWinCfg &w, uint64_t n0, uint64_t count, uint32_t requested);
int  bhwp_check_exec(const bhw_exec *ex);
uint32_t bhwp_exec_table_format(const bhw_exec *ex);

// Table formats a tiled whole-period call may use, narrowest first (tab_dlog values); plain (0) is always the last one.
constexpr int kMaxFormats = 5;
int bhwp_table_format_candidates(const BhwCordicCfg &c, bool tiled, uint32_t limit, uint32_t out[kMaxFormats]);
// verdict cache of the packed formats: a property of (model, PW, W, PRECISION, format), settled on the device once per process
enum { kFmtUnknown = 0, kFmtOk = 1, kFmtBad = 2 };
int  bhwp_fmt_verdict(const bhw_params *p, uint32_t dlog);
void bhwp_fmt_set_verdict(const bhw_params *p, uint32_t dlog, int v);
// The candidates of a call read against the verdict cache, once: every format decision of the rebuilt and the resident tables
// (scratch size, trial order, the format bhw_describe_plan names, the format a resident table keeps) is taken from it.
struct BhwFormatWalk {
    uint32_t kept;                  // the narrowest candidate known to be exact (0: plain, always exact)
    uint32_t open[kMaxFormats];     // packed candidates narrower than `kept` with no verdict yet, narrowest first: the trial order
    int n_open;                     // ... (none while `capturing`: a capture cannot read a check word back)
    uint64_t scratch_bytes;         // what a table-strategy call needs right now: the largest of `kept` and the open formats
};
BhwFormatWalk bhwp_format_walk(const bhw_params *p, const BhwCordicCfg &c, bool tiled, uint32_t limit, bool capturing);
// the name of a table format (tab_dlog) in the describe strings
const char *bhwp_format_name(uint32_t tab_dlog);

// What a table-strategy call over [n0, n0 + count) does with its whole periods.
struct BhwTableCall {
    bool has_period;      // the range holds at least one whole period
    bool images;          // a contiguous range of whole eighths of one window: the tile kernel over those images
    bool tiled;           // tile kernel (else quadrant fold / run-length / general gather)
    uint32_t img_mask, n0mod;
};
BhwTableCall bhwp_table_call(const bhw_params *p, const BhwCordicCfg &c, const BhwWinCfg &w, uint64_t n0, uint64_t count, bool apply);

// ---- resident tables (bhw_table_create and the *_from_table calls) ------------------------------------------------------------
// Argument checks of bhw_table_create, before any HIP call: BADARG / UNSUPPORTED as documented in bhw.h.
int  bhwp_table_create_checks(const bhw_params *p, uint32_t table_format);
// `p` may be used with a table built from `pt`: same model, phi_width, dat_width (and precision, VHDL model), CORDIC source.
// BHW_ERR_BADARG naming the first field that differs.  aa, n_terms, win_type and combine are free.
int  bhwp_table_key_check(const bhw_params *pt, const bhw_params *p);
// The layout a resident table of `p` is held in: resolves `c` and sets c.tab_split; *tiled = whole periods take the tile kernel
// (split layout at z_shr == 0, the one-run tile form over the natural layout otherwise), else the fold / run-length kernels
// over the natural plain table.
void bhwp_resident_layout(const bhw_params *p, BhwCordicCfg &c, bool *tiled);
// Kernel of a ragged piece over a resident table: k_range_combine<fmt, nt, mode> (nt: the term-count bound 3, 5 or 7 of the
// instance).  Every table format a resident table can hold has instances, so this never declines today; false would send the
// piece to k_table_combine (format read at run time).
bool bhwp_range_form(const BhwCordicCfg &c, const BhwWinCfg &w, int *fmt, int *nt, int *mode);
// bhw_table_describe: one line for a from-table call of (p, n0, count) over a table whose c.tab_dlog / c.tab_split are set
int  bhwp_describe_from_table(const bhw_params *p, const BhwCordicCfg &ct, bool tiled, uint64_t n0, uint64_t count, char *buf, uint64_t len);

// ownership parts
int  bhwp_part_checks(const bhw_params *p, uint32_t part, uint32_t n_parts);
// strategy of bhw_generate_part_device: true = fused kernel over the part's runs, false = full table + the part's tiles; rc != 0: neither applies
bool bhwp_part_fused(const bhw_params *p, const BhwCordicCfg &c, const BhwFoldRun *runs, int n_runs, uint32_t tile_count, uint32_t requested, int *rc);

// ---- overlapped-frame apply (bhw_apply_frames_device / _from_table) -------------------------------------------------------------
// Routes: the frames kernel with the direct CORDIC source, the frames kernel over a resident table, or one bhw_apply_device per frame.
enum { BHWP_FRAMES_DIRECT = 0, BHWP_FRAMES_TABLE = 1, BHWP_FRAMES_PER_FRAME = 2 };
constexpr uint32_t kFramesBlock = 256;          // lanes of a workgroup: min(N, 256) along k, the rest side by side over frames
constexpr uint32_t kFramesTargetWg = 4096;      // workgroups the frame groups are cut for (16 per CU on 256 CUs) ...
constexpr uint64_t kFramesOnePassGx = 1024;     // ... unless one pass over the window is this many already: then G = every frame
constexpr uint32_t kFramesMaxGridY = 65535;
// Per-frame route of a one-channel CORDIC call: below this many frames one bhw_apply_device per frame costs
// less than the direct CORDIC of every coefficient in the frames kernel.  Measured with BH-7 / 32 bits (192 rotations per
// coefficient: (n_terms - 1) * n_iter) at 2^18, 2^20 and 2^22 (profiles/r07_apply_frames.json: 22 / 65 / 230 us for the frames
// kernel against 7.7 / 11.4 / 28 us per frame); other configurations scale it by their rotations per coefficient.
constexpr uint32_t kFramesPerFrameRef = 192;
inline uint32_t bhwp_frames_crossover(uint32_t phi_width) { return phi_width >= 22 ? 8u : phi_width >= 20 ? 6u : phi_width >= 18 ? 3u : 0u; }
struct BhwFramesPlan {
    int route;           // BHWP_FRAMES_*
    uint32_t kx;         // lanes of a workgroup along k: min(N, kFramesBlock)
    uint32_t fy;         // frames a workgroup runs side by side: kFramesBlock / kx
    uint64_t group;      // G: frames one lane applies its coefficient to (in steps of fy)
    uint64_t grid_x;     // N / kx
    uint64_t grid_y;     // ceil(frames / (fy * G)) <= kFramesMaxGridY
    uint64_t y_stride;   // resolved (0 -> N * channels)
    uint64_t len;        // N = 2^phi_width, or the length L of the any-length kernels
};
// Every argument check of the two calls that needs no table handle, before any HIP call: BHW_OK, BADARG or UNSUPPORTED (Taylor with
// two channels).  frames == 0 passes with the pointers unchecked (nothing to do); `pointers` false: the describe call, no pointers.
// length > 0: the checks of a window of that length (bhwp_len_checks passed), with L in place of N.
int  bhwp_frames_checks(const bhw_params *p, const bhw_frames *f, const void *d_x, const void *d_y, bool pointers = true, uint64_t length = 0);
// route, frame-group size and grid of a call that passed bhwp_frames_checks; force_route >= 0 overrides the route rule (A/B runs).
// length > 0: the any-length kernels (k_frames_direct_len / k_frames_table_len) over a window of length L: kx the power of two at or
// above min(L, kFramesBlock), grid_x = ceil(L / kx).  At a power-of-two L the shape is the one of length 0.
// f32: the float32 kernels (bhw_frames_f32.hip), which have no per-frame route: the direct or the table route, same shape.
BhwFramesPlan bhwp_frames_plan(const bhw_params *p, const bhw_frames *f, bool from_table, int force_route = -1, uint64_t length = 0,
                               bool f32 = false);
// bhw_apply_frames_describe: ct = the resident table's resolved configuration (format and layout set), or NULL for the library call
int  bhwp_describe_frames(const bhw_params *p, const BhwCordicCfg *ct, const bhw_frames *f, char *buf, uint64_t len);
// the frames kernel of a plan (bhw_frames.hip): d_table NULL = k_frames_direct, else k_frames_table over the resident table of c;
// lp != NULL: their any-length forms over the window of length lp->len
int  bhwk_frames(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwFramesPlan &pl, const bhw_frames *f,
                 const int32_t *d_x, int32_t *d_y, const int32_t *d_table, const BhwLenPhase *lp = nullptr);

// ---- weighted overlap-add (bhw_overlap_add_device / _from_table) --------------------------------------------------------------
// Output t = q * hop + r.  A lane owns one residue r and a block of Q consecutive hops q: it computes w[r + j * hop] once per j and
// adds y[(q - j) * y_stride + (r + j * hop) * C + c] * w into Q * C int64 registers, so every element of y is read once and every
// output written once.  Lanes are numbered relative to t0: lane s < min(hop, count) holds the residue of t0 + s, row i the output
// u = i * hop + s (u < count).
enum { BHWP_OLA_DIRECT = 0, BHWP_OLA_TABLE = 1 };
constexpr uint32_t kOlaBlock = 256;           // lanes of a workgroup: rx along the residue, fy = kOlaBlock / rx side by side over rows
constexpr uint32_t kOlaQMax = 16;             // Q: rows (hops) of one lane, the int64 accumulators it holds per channel
constexpr uint32_t kOlaQMaxNorm = 8;          // ... of the float32 overlap-add with the envelope division (Q more binary64 sums)
constexpr uint32_t kOlaTargetWg = 4096;       // workgroups Q is cut for (16 per CU on 256 CUs) ...
constexpr uint64_t kOlaOnePassGx = 1024;      // ... unless the residues alone give this many: then Q = kOlaQMax
constexpr uint32_t kOlaMaxGridY = 65535;      // row blocks beyond it are taken by a grid-stride loop
struct BhwOlaPlan {
    int route;           // BHWP_OLA_*
    uint32_t rx;         // lanes along the residue (a power of two <= kOlaBlock)
    uint32_t fy;         // rows a workgroup runs side by side: kOlaBlock / rx
    uint32_t q;          // Q: consecutive rows of one lane, 1..kOlaQMax
    uint64_t lanes;      // residues in use: min(hop, count)
    uint64_t rows;       // ceil(count / hop)
    uint64_t row_blocks; // ceil(rows / (fy * Q)): workgroup rows
    uint64_t grid_x;     // ceil(lanes / rx)
    uint64_t grid_y;     // min(row_blocks, kOlaMaxGridY)
    uint64_t jmax;       // ceil(N / hop): frames that reach the output of residue 0
    uint64_t y_stride;   // resolved (0 -> N * channels)
    uint64_t q0, r0;     // t0 = q0 * hop + r0
    uint64_t len;        // N = 2^phi_width, or the length L of the any-length kernels
};
// Every argument check of the two calls that needs no table handle, before any HIP call: BHW_OK, BADARG or UNSUPPORTED (the Taylor
// sources).  count == 0 passes with the pointers unchecked; `pointers` false: the describe call, no pointers.
// length > 0: the checks of a window of that length (bhwp_len_checks passed), with L in place of N.
int  bhwp_ola_checks(const bhw_params *p, const bhw_ola *o, const void *d_y, const void *d_x, bool pointers = true, uint64_t length = 0);
// route, Q, lane layout and grid of a call that passed bhwp_ola_checks with count > 0; force_q / force_rx > 0 override the rule
// (bhw_dbg_overlap_add_shape: Q in 1..kOlaQMax, rx a power of two <= kOlaBlock; other values are ignored)
// length > 0: the plan of the any-length kernels (k_ola_direct_len / k_ola_table_len) over a window of length L (jmax = ceil(L / hop));
// at a power-of-two L it is the plan of length 0.
// q_max: the Q bound of the kernel (kOlaQMax; kOlaQMaxNorm for the float32 overlap-add with BHW_OLA_NORMALIZE, which holds Q more
// binary64 sums and is compiled for that many rows).
// batch: the signals of a batched launch (bhwp_stft_ola), which share the workgroup target: gy_target is cut for grid_x * batch.
BhwOlaPlan bhwp_ola_plan(const bhw_params *p, const bhw_ola *o, bool from_table, uint32_t force_q = 0, uint32_t force_rx = 0,
                         uint64_t length = 0, uint32_t q_max = kOlaQMax, uint64_t batch = 1);
// bhw_overlap_add_describe: ct = the resident table's resolved configuration (format and layout set), or NULL for the library call
int  bhwp_describe_ola(const bhw_params *p, const BhwCordicCfg *ct, const bhw_ola *o, char *buf, uint64_t len);
// the overlap-add kernel of a plan (bhw_ola.hip): d_table NULL = k_ola_direct, else k_ola_table over the resident table of c
// lp != NULL: their any-length forms over the window of length lp->len (= pl.len)
int  bhwk_ola(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwOlaPlan &pl, const bhw_ola *o,
              const int32_t *d_y, int32_t *d_x, const int32_t *d_table, const BhwLenPhase *lp = nullptr);

// ---- windows of any length (the *_len entry points; the phase map is bhw_len.h) -------------------------------------------------
// Argument checks of every *_len call on (p, length), before any other and before any HIP call: p valid, 1 <= length <= 2^phi_width
// (BADARG), CORDIC source (UNSUPPORTED, as for tables; the models DDS48 / SCALED are refused by bhwp_validate).
int  bhwp_len_checks(const bhw_params *p, uint64_t length);
// the call takes the any-length kernels: L != 2^phi_width, or `force` (bhw_dbg_len_force_kernels)
inline bool bhwp_len_kernels(const bhw_params *p, uint64_t length, bool force) { return force || length != (1ull << p->phi_width); }
// bhw_describe_len: one line naming the route, the kernel and whether the power-of-two route was taken.  Exactly one of: f (frames),
// o (overlap-add), neither (generate [n0, n0 + count)).  ct / tiled: the resident table's resolved configuration and layout, or NULL
// (library call).
int  bhwp_describe_len(const bhw_params *p, const BhwCordicCfg *ct, bool tiled, uint64_t length, bool force, uint64_t n0, uint64_t count,
                       const bhw_frames *f, const bhw_ola *o, char *buf, uint64_t len);
// ---- float32 frame apply and overlap-add (the *_f32 entry points) ---------------------------------------------------------------
// Argument checks of every *_f32 call on (p, length, flags), before any other and before any HIP call: bhwp_len_checks, then flags
// outside {0, BHW_OLA_NORMALIZE} (BADARG).  The frames and overlap-add checks follow with L in place of N.
int  bhwp_f32_checks(const bhw_params *p, uint64_t length, uint32_t flags);
// bhw_describe_f32: one line naming the route, the plan, the kernel and whether the overlap-add normalises.  length: L (2^phi_width:
// the power-of-two kernels unless `force`, as bhwp_len_kernels); exactly one of f and o; ct the resident table's resolved
// configuration, or NULL (library call).
int  bhwp_describe_f32(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, bool force, const bhw_frames *f, const bhw_ola *o,
                       uint32_t flags, char *buf, uint64_t len);
// The signals of a batched float32 overlap-add: `batch` of them (a grid dimension), the rows of signal b at d_y + b * y_bstride and
// its outputs at d_x + b * x_bstride (float elements).  {1, 0, 0}: the one signal of bhw_overlap_add_f32_*.
struct BhwOlaBatch {
    uint64_t batch, y_bstride, x_bstride;
};
constexpr uint32_t kOlaMaxGridZ = 65535;      // signals of one launch (grid z); a larger batch takes several launches
// the float32 kernels (bhw_frames_f32.hip, bhw_ola_f32.hip / bhw_ola_f32_norm.hip): d_table NULL = the direct CORDIC chains, else
// the gather over the resident table of c; lp != NULL: the any-length forms over the window of length lp->len
int  bhwk_frames_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwFramesPlan &pl, const bhw_frames *f,
                     const float *d_x, float *d_y, const int32_t *d_table, const BhwLenPhase *lp);
int  bhwk_ola_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwOlaPlan &pl, const bhw_ola *o, bool normalize,
                  const float *d_y, float *d_x, const int32_t *d_table, const BhwLenPhase *lp, const BhwOlaBatch &bt = BhwOlaBatch{1, 0, 0});

// ---- batched, centred STFT framing and overlap-add (bhw_stft_frames_f32_* / bhw_istft_ola_f32_*) ----------------------------------
// Frames: the lanes of a workgroup run along the row columns j in [0, n_fft) (kx of them, a power of two), fy = kFramesBlock / kx rows
// side by side.  The rows (b, f) of the whole batch form one pool, row r = b * frames + f, which is cut into groups of G * fy rows as
// bhwp_frames_plan cuts frames: a lane computes v[j - col0] once and applies it to G rows of any signals.  Row blocks past
// kFramesMaxGridY are taken by a grid-stride loop.
struct BhwStftPlan {
    int route;            // BHWP_FRAMES_DIRECT or BHWP_FRAMES_TABLE
    uint32_t kx;          // lanes along the row: the power of two at or above min(n_fft, kFramesBlock)
    uint32_t fy;          // rows a workgroup runs side by side: kFramesBlock / kx
    uint64_t rows;        // B * frames: the row pool
    uint64_t group;       // G: rows one lane applies its coefficient to (in steps of fy)
    uint64_t row_blocks;  // ceil(rows / (fy * G))
    uint64_t grid_x;      // ceil(n_fft / kx)
    uint64_t grid_y;      // min(row_blocks, kFramesMaxGridY)
    uint64_t step_b, step_f;        // fy = step_b * frames + step_f: the (b, f) step of a lane from one of its rows to the next
    uint64_t x_stride, y_stride, y_bstride;   // resolved (0 -> T * C, n_fft * C, frames * y_stride)
    uint64_t len;         // L
};
// Every argument check of the four calls (include/bhw.h) that needs no table handle, before any HIP call.  inverse: the overlap-add
// (flags 0 or BHW_OLA_NORMALIZE), else the frames call (flags must be 0).  frames 0 (frames call) / samples 0 (overlap-add) pass with
// the pointers unchecked; `pointers` false: the describe call.
// welch: the frames call of bhw_welch_frames_f32_*, whose segments read L samples each, not n_fft (bhwp_welch_checks).
int  bhwp_stft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, bool inverse, uint32_t flags, const void *d_x,
                      const void *d_y, bool pointers = true, bool welch = false);
// the plan of a frames call that passed bhwp_stft_checks with frames > 0
BhwStftPlan bhwp_stft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, bool from_table);
// The overlap-add of a call that passed bhwp_stft_checks with samples > 0, mapped onto the one-signal overlap-add: o (t0 = pad - col0,
// count = samples, y_stride resolved) over rows that start col0 * C floats into each frame row, and the batch strides.  The extent
// check of bhwp_ola_checks does not apply: outputs past the frames' extent are empty sums.
void bhwp_stft_ola(const bhw_stft *s, bhw_ola &o, BhwOlaBatch &bt);
// bhw_describe_stft: ct = the resident table's resolved configuration, or NULL (library call)
int  bhwp_describe_stft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, bool inverse, uint32_t flags,
                        char *buf, uint64_t len);
// the frames kernel (bhw_stft_f32.hip): d_table NULL = the direct CORDIC chains, else the gather over the resident table of c, both
// at the angles of the length-L phase map lp (every L, 2^phi_width included)
int  bhwk_stft_frames_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwStftPlan &pl, const bhw_stft *s,
                          const float *d_x, float *d_y, const int32_t *d_table, const BhwLenPhase &lp);

// ---- Welch's method: window sums, detrended segments, averaged periodogram (bhw_window_sums_* / bhw_welch_*) ----------------------
// Window sums: one lane per coefficient in a grid-stride loop, a wave and workgroup reduction of (s1, low and high halves of u^2), then
// three 64-bit integer atomics per workgroup (bhw_welch_sums.hip).
constexpr uint32_t kSumsBlock = 256;            // lanes of a workgroup
constexpr uint32_t kSumsPerLane = 8;            // coefficients a lane aims at before the grid stops growing
constexpr uint32_t kSumsMaxGrid = 4096;         // workgroups at most (each ends in three atomics)
struct BhwSumsPlan {
    uint64_t len;         // L
    uint32_t grid;        // workgroups of kSumsBlock lanes; lane g takes k = g, g + grid * kSumsBlock, ...
    uint32_t trips;       // ceil(L / (grid * kSumsBlock)): the loop count of every lane (uniform: the table gather is wave-wide)
};
int  bhwp_sums_checks(const bhw_params *p, uint64_t length, uint32_t flags, const void *d_sums, bool pointers = true);
BhwSumsPlan bhwp_sums_plan(uint64_t length);
// the 128-bit sum of squares from the two counters of the result: lo + hi * 2^32
inline unsigned __int128 bhwp_sums_join(uint64_t lo, uint64_t hi) { return (unsigned __int128)lo + ((unsigned __int128)hi << 32); }

// Segments with BHW_WELCH_DETREND_CONSTANT: a mean pass, one wave per (row, both channels), kWelchMeanBlock / 64 rows per workgroup and
// a grid-stride loop over the row pool past kWelchMeanMaxGrid workgroups; then the frames loop of bhwp_stft_plan with the row's mean.
constexpr uint32_t kWelchMeanBlock = 256;
constexpr uint32_t kWelchMeanMaxGrid = 1u << 20;
struct BhwWelchPlan {
    BhwStftPlan frames;   // the plan of the frames launch (flags 0: the stft kernel itself)
    bool detrend;
    uint64_t mean_grid;   // workgroups of the mean pass (0 without detrending)
    uint64_t ws_bytes;    // workspace the call needs: rows * C floats (0 without detrending)
};
// bhwp_stft_checks of the frames call, then the Welch restrictions and the workspace (pointers false: the describe call)
int  bhwp_welch_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_x, const void *d_y,
                       const void *workspace, uint64_t workspace_bytes, bool pointers = true);
uint64_t bhwp_welch_workspace_bytes(const bhw_stft *s, uint32_t flags);
BhwWelchPlan bhwp_welch_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table);

// Periodogram: one workgroup per (signal, frame block, bin tile), kPsdLanes lanes along the bins and kPsdWaves waves over the frames of a
// pass (each loads `unroll` of them; wave 0 adds the pass in ascending order); a frame block is BHW_WELCH_BLOCK frames (part of the
// contract, include/bhw.h).  One block: the first launch writes P.  More: it writes the block sums to the workspace,
// [(b * blocks + blk) * K + k], and k_welch_psd_join adds them in block order.
constexpr uint32_t kPsdLanes = 64;
constexpr uint32_t kPsdWaves = 4;
constexpr uint32_t kPsdUnrollMax = 16;          // frames one wave loads per pass, all in flight: 16 (a pass of 64 frames, 32 KiB of binary64
constexpr uint32_t kPsdUnrollMin = 8;           // squares in LDS) up to kPsdSmallGrid workgroups, 8 (32 frames, 16 KiB) above
constexpr uint32_t kPsdSmallGrid = 1024;
struct BhwPsdPlan {
    uint64_t blocks;      // ceil(F / BHW_WELCH_BLOCK)
    uint64_t tiles;       // ceil(K / kPsdLanes)
    uint64_t grid;        // B * blocks * tiles workgroups
    uint32_t unroll;      // kPsdUnrollMax or kPsdUnrollMin
    uint64_t join_grid;   // workgroups of the second launch (0 for one block)
    uint64_t y_stride, y_bstride, p_stride;   // resolved
    uint64_t ws_bytes;
};
int  bhwp_psd_checks(const bhw_psd *d, const void *d_Y, const void *d_P, const void *workspace, uint64_t workspace_bytes,
                     bool pointers = true);
BhwPsdPlan bhwp_psd_plan(const bhw_psd *d);
// s_k's factor: 2 for the bins scipy doubles under BHW_PSD_ONESIDED
BHW_HD inline bool bhw_psd_doubled(uint32_t flags, uint64_t k, uint64_t bins, uint64_t n_fft)
{
    return (flags & BHW_PSD_ONESIDED) && k != 0 && !(n_fft % 2 == 0 && k == bins - 1);
}
// bhw_describe_welch: s: the segments; d: the periodogram; neither: the window sums.  ct as bhwp_describe_stft.
int  bhwp_describe_welch(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_psd *d,
                         char *buf, uint64_t len);
// the kernels (bhw_welch_sums.hip, bhw_welch_f32.hip): d_table NULL = the direct CORDIC chains, else the gather over the resident table
int  bhwk_window_sums(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwSumsPlan &pl, uint32_t flags,
                      const int32_t *d_table, const BhwLenPhase &lp, uint64_t *d_sums);
int  bhwk_welch_frames_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwWelchPlan &pl, const bhw_stft *s,
                           const float *d_x, float *d_y, float *d_mean, const int32_t *d_table, const BhwLenPhase &lp);
int  bhwk_welch_psd_f32(const BhwLaunch &l, const BhwPsdPlan &pl, const bhw_psd *d, const float *d_Y, float *d_P, double *d_ws);

// Cross spectra (bhw_welch_csd.hip): the periodogram's grid -- one workgroup per (signal of Y, frame block, bin tile), kPsdLanes lanes
// along the bins, kPsdWaves waves over the frames of a pass -- with two operands and `chains` ordered sums per bin: 2 (C_re, C_im) when
// P_xy is the only output, else 4 (S_xx, S_yy, C_re, C_im).  Wave w loads `unroll` frames of X and of Y per pass and puts their `chains`
// binary64 terms in LDS; then wave c < chains adds chain c of the pass in ascending order.  unroll = kCsdPassBytes / (waves * lanes *
// chains * 8): a pass always fills kCsdPassBytes = 32 KiB of LDS (16 frames of four terms, 32 frames of two), so four workgroups fit the
// CU's 160 KiB.  One block: the first launch writes the outputs.  More: the block sums go to the workspace,
// [((b * blocks + blk) * chains + c) * K + k], and k_welch_csd_join adds them in block order and writes the outputs.
constexpr uint32_t kCsdPassBytes = 32u * 1024u;
constexpr uint32_t kCsdOutputs = 5;              // d_Pxy, d_Pxx, d_Pyy, d_Cxy, d_H1: the order of the output mask's bits
constexpr uint32_t kCsdOutputMask = BHW_CSD_PXY | BHW_CSD_PXX | BHW_CSD_PYY | BHW_CSD_COHERENCE | BHW_CSD_H1;
struct BhwCsdPlan {
    uint64_t blocks;      // ceil(F / BHW_WELCH_BLOCK)
    uint64_t tiles;       // ceil(K / kPsdLanes)
    uint64_t grid;        // B * blocks * tiles workgroups
    uint32_t chains;      // 2 or 4
    uint32_t unroll;      // frames one wave loads per pass: 8 (two chains) or 4 (four)
    uint32_t lds_bytes;   // waves * unroll * lanes * chains * 8
    uint64_t join_grid;   // workgroups of the second launch (0 for one block)
    uint64_t x_stride, x_bstride, y_stride, y_bstride, o_stride;   // resolved; x_bstride 0 under BHW_CSD_BROADCAST_X
    uint64_t ws_bytes;
};
// outs: the five output pointers in the order of kCsdOutputs (pointers false: the describe / workspace-size calls, outs may be NULL)
int  bhwp_csd_checks(const bhw_csd *d, const void *d_X, const void *d_Y, const void *const *outs, const void *workspace,
                     uint64_t workspace_bytes, bool pointers = true);
BhwCsdPlan bhwp_csd_plan(const bhw_csd *d);
int  bhwp_describe_csd(const bhw_csd *d, char *buf, uint64_t len);
int  bhwk_welch_csd_f32(const BhwLaunch &l, const BhwCsdPlan &pl, const bhw_csd *d, const float *d_X, const float *d_Y, float *const *outs,
                        double *d_ws);

// ---- fused window and real FFT (bhw_stft_fft_f32_*; bhw_stft_fft.hip) ---------------------------------------------------------------
// A workgroup of kFftBlock lanes owns whole rows.  M = n_fft / 2 complex points per row (the real row taken as pairs); lpf lanes work
// on a row (one radix-4 butterfly per lane and pass up to M = 1024), fy = kFftBlock / lpf rows side by side; a lane holds cpl =
// n_fft / lpf columns of its row (column c * lpf + lane) and their window coefficients in registers.  The rows (b, f) of the batch are
// one pool cut into groups of fy consecutive rows; workgroup w takes the groups w, w + grid, ... (the last group may be ragged).
// LDS: two buffers of fy * M complex64 (Stockham ping-pong; the first also stages the window and the raw row of the detrend mean), the
// n_fft / 2 twiddles exp(-2 pi i k / n_fft) and fy means.
constexpr uint32_t kFftBlock = 256;
constexpr uint32_t kFftMinLog = 4, kFftMaxLog = 12;   // n_fft = 2^4 .. 2^12
constexpr uint32_t kFftMaxCpl = 16;                   // columns of one lane at most (n_fft 4096 on 256 lanes)
constexpr uint32_t kFftMaxGrid = 2048;                // workgroups at most: the window and the twiddles are computed once per workgroup
struct BhwStftFftPlan {
    int route;            // BHWP_FRAMES_DIRECT or BHWP_FRAMES_TABLE
    bool detrend;
    uint32_t log2n;       // n_fft = 2^log2n
    uint32_t m;           // M = n_fft / 2
    uint32_t lpf;         // lanes per row: min(kFftBlock, max(4, M / 4))
    uint32_t fy;          // rows side by side: kFftBlock / lpf
    uint32_t cpl;         // columns per lane: n_fft / lpf (4, 8 or 16)
    uint32_t radix4;      // radix-4 passes: floor(log2(M) / 2)
    uint32_t radix2;      // 1: a last radix-2 pass (log2(M) odd)
    uint32_t lds_bytes;   // 2 * fy * M * 8 + M * 8 + fy * 4  (<= 64 KiB)
    uint64_t rows;        // B * frames
    uint64_t groups;      // ceil(rows / fy)
    uint64_t grid;        // min(groups, kFftMaxGrid)
    uint64_t x_stride, y_stride, y_bstride;   // resolved (0 -> T, 2K, frames * y_stride)
    uint64_t len;         // L
};
// Every check of the two calls that needs no table handle, before any HIP call (include/bhw.h).  frames 0 passes with the pointers
// unchecked; `pointers` false: the describe call.
int  bhwp_stft_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_x, const void *d_Y,
                          bool pointers = true);
// the plan of a call that passed the checks (frames 0: rows, groups and grid are 0)
BhwStftFftPlan bhwp_stft_fft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table);
// the radix schedule as text, "4x4x4x2"
void bhwp_stft_fft_schedule(const BhwStftFftPlan &pl, char *buf, uint64_t len);
int  bhwp_describe_stft_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                            uint64_t len);
int  bhwk_stft_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwStftFftPlan &pl, const bhw_stft *s,
                       const float *d_x, float *d_Y, const int32_t *d_table, const BhwLenPhase &lp);

// ---- fused power and filter-bank spectrogram (bhw_spectrogram_f32_*; bhw_spectrogram.hip) ----------------------------------------------
// The forward kernel with another epilogue: the plan is bhwp_stft_fft_plan's (lanes per row, rows per workgroup, columns per lane,
// schedule, groups, grid, LDS bytes) with y_stride / y_bstride resolved in floats of the output rows of W = K (power) or filters (bank).
constexpr uint32_t kSpecMaxFilters = 4096;
constexpr uint32_t kSpecMaxWeights = 1u << 24;
// Every check of the two calls that needs no table handle, before any HIP call (include/bhw.h): the input side by
// bhwp_stft_fft_checks, the bank's fields, the output rules with W in place of 2K, the pointers.  frames 0 passes with the pointers
// unchecked; `pointers` false: the describe call.
int  bhwp_spectrogram_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb, const void *d_x,
                             const void *d_P, bool pointers = true);
BhwStftFftPlan bhwp_spectrogram_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                                     bool from_table);
int  bhwp_describe_spectrogram(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                               const bhw_fbank *fb, char *buf, uint64_t len);
int  bhwk_spectrogram_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwStftFftPlan &pl, const bhw_stft *s,
                          const bhw_fbank *fb, const float *d_x, float *d_P, const int32_t *d_table, const BhwLenPhase &lp);

// ---- fused Welch PSD (bhw_welch_fft_f32_*; bhw_welch_fft.hip) ----------------------------------------------------------------------------
// The forward kernel's lanes, LDS, schedule and row steps (fft: bhwp_stft_fft_plan's, with groups and grid recounted) under another
// ownership: a workgroup owns RUNS.  A run is max(BHW_WELCH_FFT_CHUNK, fy) consecutive frames of one signal on the frame axis padded to
// fpad = whole runs, so it is a whole number of chunks and never crosses a signal; gpr = max(1, 16 / fy) groups make a run; workgroup
// w takes the runs w, w + grid, ...; grid = min(runs, kFftMaxGrid).  acc: the binary64 accumulators a lane carries over a run
// (fy < 16: ceil(K / kFftBlock), at most kWelchFftMaxAcc; fy >= 16: none is carried, a lane sums one (chunk, bin) at a time).
// Workspace: B * chunks * K chunk sums, then (blocks > 1) B * blocks * K block sums.
constexpr uint32_t kWelchFftMaxAcc = 9;               // ceil(2049 / 256)
// The run plan of every fused Welch and hold call (real and I/Q input, both radix families), from the batch, the frames, the rows side
// by side, the bins of an output row and the caller's p_stride: one text for the four bhwp_welch_*_plan and, with `pairs` for fy,
// bhwp_csd_fft_plan.  frames 0: everything but bins, p_stride, run, gpr and acc is 0.
struct BhwWelchRuns {
    uint64_t bins;        // columns of an output row: K = n_fft / 2 + 1 (real input, one-sided) or n_fft (I/Q, two-sided)
    uint64_t p_stride;    // resolved (0 -> bins)
    uint64_t run;         // frames of a run: max(BHW_WELCH_FFT_CHUNK, fy)
    uint32_t gpr;         // groups per run: run / fy
    uint32_t acc;         // accumulators a lane carries over a run: ceil(bins / kFftBlock); 0 for fy >= 16
    uint64_t fpad;        // frames of a signal padded to whole runs
    uint64_t chunks;      // ceil(F / BHW_WELCH_FFT_CHUNK) per signal
    uint64_t blocks;      // ceil(F / BHW_WELCH_BLOCK) per signal
    uint64_t runs;        // B * fpad / run
    uint64_t groups;      // runs * gpr = B * fpad / fy
    uint64_t grid;        // min(runs, kFftMaxGrid)
    uint64_t blocks_grid; // workgroups of the launch that adds the chunks of a block
    uint64_t join_grid;   // workgroups of the launch that adds the blocks (0 for one block)
    uint64_t ws_bytes;    // 8 * B * bins * (chunks + (blocks > 1 ? blocks : 0)); 0 beyond 2^60
};
BhwWelchRuns bhwp_welch_runs(uint64_t batch, uint64_t frames, uint32_t fy, uint64_t bins, uint64_t p_stride = 0);
// A Welch plan IS the run plan (its base: wp.chunks, wp.p_stride, ...) plus the family's forward plan.
struct BhwWelchFftPlan : BhwWelchRuns {   // bins = K = n_fft / 2 + 1
    BhwStftFftPlan fft;   // groups = B * fpad / fy and grid = min(runs, kFftMaxGrid) as in the base; rows = B * frames; the y strides are 0
};
// Every check of the two calls that needs no table handle, before any HIP call (include/bhw.h).  frames 0 passes with the pointers
// unchecked; `pointers` false: the describe call.
int  bhwp_welch_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint32_t psd_flags,
                           uint64_t p_stride, const void *d_x, const void *d_P, const void *workspace, uint64_t workspace_bytes,
                           bool pointers = true);
// bhw_welch_fft_workspace_bytes: from batch, frames and n_fft alone (0 for a NULL descriptor, frames 0 or a product beyond 2^60)
uint64_t bhwp_welch_fft_workspace_bytes(const bhw_stft *s);
BhwWelchFftPlan bhwp_welch_fft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                    bool from_table);
int  bhwp_describe_welch_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                             uint64_t len);
int  bhwk_welch_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwWelchFftPlan &pl, const bhw_stft *s,
                        double scale, uint32_t psd_flags, const float *d_x, float *d_P, double *d_ws, const int32_t *d_table,
                        const BhwLenPhase &lp);

// ---- fused Welch cross spectra (bhw_csd_fft_f32_*; bhw_csd_fft.hip) -------------------------------------------------------------------
// The forward kernel's row function with frames of x and of y side by side: of the fy slots of a group the first pairs = fy / 2 carry
// the frames f0 .. f0 + pairs - 1 of x and the others the same frames of y, so fy >= 2: lpf = min(kCsdFftMaxLpf, max(4, M / 4)), and
// n_fft 2048 runs as n_fft 4096 runs in the forward kernel (two butterflies per lane and pass, cpl 16, 40 KB of LDS).  Ownership is
// bhwp_welch_runs' with `pairs` in place of fy: a run is max(16, pairs) frames of one pair of signals.  acc: the binary64
// accumulators a lane carries over a run PER CHAIN (pairs < 16: ceil(K / kFftBlock), at most kCsdFftMaxAcc; else none); there are
// always kCsdFftChains chains.  Workspace: the chain index is part of the bin axis, [(b * chunks + c) * 4 K + chain * K + k], then
// (blocks > 1) the block sums likewise, so stage 1 of the join is k_welch_fft_join over 4 K bins.
constexpr uint32_t kCsdFftMaxLpf = 128;
constexpr uint32_t kCsdFftMaxLog = 11;                // n_fft <= 2048
constexpr uint32_t kCsdFftChains = 4;                 // S_xx, S_yy, C_re, C_im
constexpr uint32_t kCsdFftMaxAcc = 5;                 // ceil(1025 / 256)
struct BhwCsdFftPlan {
    BhwStftFftPlan fft;   // lpf, fy, cpl, lds_bytes as above; groups = B * fpad / pairs, grid = min(runs, kFftMaxGrid); rows = B * frames
    uint64_t bins;        // K = n_fft / 2 + 1
    uint32_t pairs;       // frame pairs side by side: fy / 2
    uint32_t gpr;         // groups per run: run / pairs
    uint64_t run;         // frames of a run: max(BHW_WELCH_FFT_CHUNK, pairs)
    uint32_t acc;         // accumulators a lane carries per chain (0 for pairs >= 16)
    uint32_t flags;       // the csd_flags
    uint64_t fpad, chunks, blocks, runs;   // bhwp_welch_runs'
    uint64_t blocks_grid; // workgroups of the launch that adds the chunks of a block, over 4 K bins (blocks > 1 only)
    uint64_t out_grid;    // workgroups of the launch that adds the last level and writes the outputs
    uint64_t o_stride;    // resolved
    uint64_t ws_bytes;
};
// Every check of the two calls that needs no table handle, before any HIP call (include/bhw.h).  frames 0 passes with the pointers
// unchecked; `pointers` false: the describe call.  outs: the five output pointers in the order of kCsdOutputs.
int  bhwp_csd_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint32_t csd_flags,
                         uint64_t o_stride, const void *d_x, const void *d_y, const void *const *outs, const void *workspace,
                         uint64_t workspace_bytes, bool pointers = true);
uint64_t bhwp_csd_fft_workspace_bytes(const bhw_stft *s);
BhwCsdFftPlan bhwp_csd_fft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint32_t csd_flags,
                                uint64_t o_stride, bool from_table);
int  bhwp_describe_csd_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                           uint32_t csd_flags, char *buf, uint64_t len);
int  bhwk_csd_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwCsdFftPlan &pl, const bhw_stft *s,
                      double scale, const float *d_x, const float *d_y, float *const *outs, double *d_ws, const int32_t *d_table,
                      const BhwLenPhase &lp);

// ---- mixed-radix fused window and real FFT (bhw_stft_mfft_f32_*; bhw_stft_mfft.hip) -----------------------------------------------------
// The forward kernel's layout for n_fft = 2^a 3^b 5^c that is even and NOT a power of two, 16 <= n_fft < 4096: M = n_fft / 2 complex
// points per row, lpf = the smallest power of two >= M / 4 (clamped to 4 .. kFftBlock, so the slot of a lane stays a shift) lanes on a
// row, fy = kFftBlock / lpf rows side by side, cpl = ceil(n_fft / lpf) <= kFftMaxCpl columns per lane; the last column of a lane need
// not exist.  The schedule is a function of n_fft alone: the radix-5 passes of M, then its radix-3 passes, then floor(a' / 2) radix-4
// passes for M = 2^a' ..., then one radix-2 pass when a' is odd.  LDS, groups, grid and the stride resolution are BhwStftFftPlan's.
// Three output forms: spectrum rows of K = M + 1 complex64, their powers (BHW_MFFT_POWER), the powers folded through a filter bank.
constexpr uint32_t kMfftMinN = 16, kMfftMaxN = 4095;
constexpr uint32_t kMfftMaxPasses = 8;                // 2916 = 2^2 3^6 runs 3x3x3x3x3x3x2: seven
enum { BHWP_MFFT_SPECTRUM = 0, BHWP_MFFT_POWER = 1, BHWP_MFFT_BANK = 2 };
struct BhwStftMfftPlan {
    int route;            // BHWP_FRAMES_DIRECT or BHWP_FRAMES_TABLE
    bool detrend;
    uint32_t form;        // BHWP_MFFT_SPECTRUM, _POWER or _BANK
    uint32_t m;           // M = n_fft / 2
    uint32_t lpf;         // lanes per row
    uint32_t fy;          // rows side by side: kFftBlock / lpf
    uint32_t cpl;         // columns per lane: ceil(n_fft / lpf)
    uint32_t passes;      // radix passes before the split pass
    uint8_t radix[kMfftMaxPasses];
    uint32_t lds_bytes;   // 2 * fy * M * 8 + M * 8 + fy * 4  (<= 64 KiB)
    uint64_t rows;        // B * frames
    uint64_t groups;      // ceil(rows / fy)
    uint64_t grid;        // min(groups, kFftMaxGrid)
    uint64_t x_stride, y_stride, y_bstride;   // resolved (0 -> T, W, frames * y_stride; W = 2K, K or filters floats)
    uint64_t len;         // L
};
// n_fft the mixed-radix calls take
bool bhwp_mfft_supported(uint64_t n_fft);
// Every check of the two calls that needs no table handle, before any HIP call (include/bhw.h).  frames 0 passes with the pointers
// unchecked; `pointers` false: the describe call.
int  bhwp_stft_mfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb, const void *d_x,
                           const void *d_out, bool pointers = true);
BhwStftMfftPlan bhwp_stft_mfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                                    bool from_table);
// the radix schedule as text, "5x5x4x2"
void bhwp_stft_mfft_schedule(const BhwStftMfftPlan &pl, char *buf, uint64_t len);
int  bhwp_describe_stft_mfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                             const bhw_fbank *fb, char *buf, uint64_t len);
int  bhwk_stft_mfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwStftMfftPlan &pl, const bhw_stft *s,
                        const bhw_fbank *fb, const float *d_x, float *d_out, const int32_t *d_table, const BhwLenPhase &lp);

// ---- fused log spectrogram, log-mel and MFCC (bhw_logspec_f32_*, bhw_logspec_mfft_f32_*; bhw_logspec.hip, bhw_logspec_mfft.hip) ----------
// The two real-input forward kernels under one more epilogue (bhw_logspec.h): the parent's plan field for field -- grid, LDS bytes,
// lanes, schedule -- with y_stride / y_bstride resolved in floats of output rows of W = coeffs (DCT), filters (bank) or K (power).
// `mixed` false: the power-of-two family (parent bhw_spectrogram_f32_*); true: the mixed-radix one (bhw_stft_mfft_f32_* + BHW_MFFT_POWER).
constexpr uint32_t kLogMaxCoeffs = 4096;
constexpr uint64_t kLogMaxDct = 1ull << 24;
// Every check of the calls that needs no table handle, before any HIP call and in the order of include/bhw.h: ONE function for both
// families.  frames 0 passes with the pointers unchecked; `pointers` false: the describe call.
int  bhwp_logspec_checks(bool mixed, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                         const bhw_logspec *ls, const void *d_x, const void *d_out, bool pointers = true);
uint64_t bhwp_logspec_width(const bhw_stft *s, const bhw_fbank *fb, const bhw_logspec *ls);
BhwStftFftPlan  bhwp_logspec_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                                  const bhw_logspec *ls, bool from_table);
BhwStftMfftPlan bhwp_logspec_mfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                                       const bhw_logspec *ls, bool from_table);
int  bhwp_describe_logspec(bool mixed, const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                           const bhw_fbank *fb, const bhw_logspec *ls, char *buf, uint64_t len);
int  bhwk_logspec_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwStftFftPlan &pl, const bhw_stft *s,
                      const bhw_fbank *fb, const bhw_logspec *ls, const float *d_x, float *d_out, const int32_t *d_table,
                      const BhwLenPhase &lp);
int  bhwk_logspec_mfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwStftMfftPlan &pl, const bhw_stft *s,
                           const bhw_fbank *fb, const bhw_logspec *ls, const float *d_x, float *d_out, const int32_t *d_table,
                           const BhwLenPhase &lp);

// ---- fused window and complex FFT for I/Q input (bhw_stft_cfft_f32_*; bhw_stft_cfft.hip) ----------------------------------------------
// The lane layout of the real forward kernel for rows of n = n_fft COMPLEX points: lpf lanes work on a row (one radix-4 butterfly per
// lane and pass up to n = 1024, two at 2048), fy = kFftBlock / lpf rows side by side, a lane holds cpl = n / lpf complex columns of its
// row and their coefficients in registers.  The passes are those bhwp_stft_fft_plan gives for 2n real points, without the split pass.
// LDS: two buffers of fy * n complex64 (the first also stages the window and the raw row of the detrend means), the n / 2 twiddles
// exp(-2 pi i k / n) and 2 * fy means.  n_fft 4096 would need 80 KiB of LDS and 16 complex columns per lane: not built.
constexpr uint32_t kCfftMinLog = 4, kCfftMaxLog = 11;  // n_fft = 2^4 .. 2^11
constexpr uint32_t kCfftMaxCpl = 8;                    // complex columns of one lane at most (n_fft 2048 on 256 lanes)
constexpr uint32_t kCfftFlags = BHW_WELCH_DETREND_CONSTANT | BHW_CFFT_POWER | BHW_CFFT_SHIFT;
struct BhwStftCfftPlan {
    int route;            // BHWP_FRAMES_DIRECT or BHWP_FRAMES_TABLE
    bool detrend, power, shifted;
    uint32_t log2n;       // n_fft = 2^log2n
    uint32_t n;           // the points of a row: n_fft
    uint32_t lpf;         // lanes per row: min(kFftBlock, max(4, n / 4))
    uint32_t fy;          // rows side by side: kFftBlock / lpf
    uint32_t cpl;         // complex columns per lane: n / lpf (4 or 8)
    uint32_t radix4;      // radix-4 passes: floor(log2(n) / 2)
    uint32_t radix2;      // 1: a last radix-2 pass (log2(n) odd)
    uint32_t lds_bytes;   // 2 * fy * n * 8 + n / 2 * 8 + fy * 8  (<= 40 KiB + 8)
    uint64_t rows;        // B * frames
    uint64_t groups;      // ceil(rows / fy)
    uint64_t grid;        // min(groups, kFftMaxGrid)
    uint64_t x_stride, y_stride, y_bstride;   // resolved, in floats (0 -> 2T; 2n or n; frames * y_stride)
    uint64_t len;         // L
};
// Every check of the two calls that needs no table handle, before any HIP call and in the order of include/bhw.h.  frames 0 passes
// with the pointers unchecked; `pointers` false: the describe call.
int  bhwp_stft_cfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_x, const void *d_Y,
                           bool pointers = true);
// the plan of a call that passed the checks (frames 0: rows, groups and grid are 0)
BhwStftCfftPlan bhwp_stft_cfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table);
int  bhwp_describe_stft_cfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                             uint64_t len);
int  bhwk_stft_cfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwStftCfftPlan &pl, const bhw_stft *s,
                        const float *d_x, float *d_Y, const int32_t *d_table, const BhwLenPhase &lp);

// ---- mixed-radix fused window and complex FFT for I/Q input (bhw_stft_cmfft_f32_*; bhw_stft_cmfft.hip) --------------------------------
// The complex kernel's layout for n = n_fft = 2^a 3^b 5^c that is NOT a power of two, odd lengths included, 16 <= n < 2048: lpf = the
// smallest power of two >= n / 4 (clamped to 4 .. kFftBlock) lanes on a row of n complex points, fy = kFftBlock / lpf rows side by
// side, cpl = ceil(n / lpf) <= kCfftMaxCpl complex columns per lane; the last column of a lane need not exist.  The schedule is
// bhwp_stft_mfft_plan's rule applied to n itself: the radix-5 passes, the radix-3 passes, the radix-4 passes, then one radix-2 pass;
// seven at most (1458 = 2 3^6).  fold: the entries of the twiddle table exp(-2 pi i k / n): n / 2 for an even n (the upper half is
// the negated lower one), n for an odd n.  LDS: two buffers of fy * n complex64 (the first also stages the window and the raw row of
// the detrend means), the fold twiddles and 2 * fy means.  Rows, groups, grid and the stride resolution are BhwStftCfftPlan's.
constexpr uint32_t kCmfftMinN = 16, kCmfftMaxN = 2047;
struct BhwStftCmfftPlan {
    int route;            // BHWP_FRAMES_DIRECT or BHWP_FRAMES_TABLE
    bool detrend, power, shifted;
    uint32_t n;           // the points of a row: n_fft
    uint32_t fold;        // twiddle table entries: n / 2 (n even) or n (n odd)
    uint32_t lpf;         // lanes per row
    uint32_t fy;          // rows side by side: kFftBlock / lpf
    uint32_t cpl;         // complex columns per lane: ceil(n / lpf) (3 .. 8)
    uint32_t passes;
    uint8_t radix[kMfftMaxPasses];
    uint32_t lds_bytes;   // 2 * fy * n * 8 + fold * 8 + fy * 8  (<= 48 608: n = 2025)
    uint64_t rows;        // B * frames
    uint64_t groups;      // ceil(rows / fy)
    uint64_t grid;        // min(groups, kFftMaxGrid)
    uint64_t x_stride, y_stride, y_bstride;   // resolved, in floats (0 -> 2T; 2n or n; frames * y_stride)
    uint64_t len;         // L
};
// n_fft the mixed-radix I/Q calls take
bool bhwp_cmfft_supported(uint64_t n_fft);
// Every check of the two calls that needs no table handle, before any HIP call and in the order of bhwp_stft_cfft_checks.  frames 0
// passes with the pointers unchecked; `pointers` false: the describe call.
int  bhwp_stft_cmfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_x, const void *d_Y,
                            bool pointers = true);
// the plan of a call that passed the checks (frames 0: rows, groups and grid are 0)
BhwStftCmfftPlan bhwp_stft_cmfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table);
int  bhwp_describe_stft_cmfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                              uint64_t len);
int  bhwk_stft_cmfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwStftCmfftPlan &pl, const bhw_stft *s,
                         const float *d_x, float *d_Y, const int32_t *d_table, const BhwLenPhase &lp);

// ---- fused Welch PSD for I/Q input (bhw_welch_cfft_f32_*; bhw_welch_cfft.hip) ---------------------------------------------------------------
// BhwWelchCfftPlan wraps BhwStftCfftPlan as BhwWelchFftPlan wraps BhwStftFftPlan: the lanes, LDS, schedule and row steps are
// bhwp_stft_cfft_plan's field for field (fft, with groups and grid recounted), the ownership is bhwp_welch_runs' with bins = n_fft.
// acc: the binary64 accumulators a lane carries over a run (fy < 16: ceil(n_fft / kFftBlock), at most kWelchCfftMaxAcc; fy >= 16:
// none).  Workspace: B * chunks * n_fft chunk sums, then (blocks > 1) B * blocks * n_fft block sums.
constexpr uint32_t kWelchCfftMaxAcc = 8;              // 2048 / 256
constexpr uint32_t kWelchCfftFlags = BHW_WELCH_DETREND_CONSTANT | BHW_CFFT_SHIFT;
struct BhwWelchCfftPlan : BhwWelchRuns {  // bins = n_fft: the estimate is two-sided
    BhwStftCfftPlan fft;  // groups and grid as in the base; rows = B * frames; the y strides are 0; power false
};
// Every check of the two calls that needs no table handle, before any HIP call and in the order of include/bhw.h.  frames 0 passes
// with the pointers unchecked; `pointers` false: the describe call.
int  bhwp_welch_cfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint64_t p_stride,
                            const void *d_x, const void *d_P, const void *workspace, uint64_t workspace_bytes, bool pointers = true);
// bhw_welch_cfft_workspace_bytes: from batch, frames and n_fft alone (0 for a NULL descriptor, frames 0 or a product beyond 2^60)
uint64_t bhwp_welch_cfft_workspace_bytes(const bhw_stft *s);
BhwWelchCfftPlan bhwp_welch_cfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                      bool from_table);
int  bhwp_describe_welch_cfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                              uint64_t len);
int  bhwk_welch_cfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwWelchCfftPlan &pl, const bhw_stft *s,
                         double scale, const float *d_x, float *d_P, double *d_ws, const int32_t *d_table, const BhwLenPhase &lp);

// ---- fused Welch PSD for I/Q input at mixed-radix n_fft (bhw_welch_cmfft_f32_*; bhw_welch_cmfft.hip) ---------------------------------------
// BhwWelchCmfftPlan wraps BhwStftCmfftPlan as BhwWelchCfftPlan wraps BhwStftCfftPlan: the lanes, LDS, schedule and row steps are
// bhwp_stft_cmfft_plan's field for field (fft, with groups and grid recounted), the ownership is bhwp_welch_runs' with bins = n_fft.
// fy is a power of two from 1 to 32 at these sizes (lpf is a power of two: 32 at n_fft 18 .. 32, 1 from 513 on), so run = max(16, fy)
// and gpr = max(1, 16 / fy) hold unchanged.  acc: the binary64 accumulators a lane carries over a run (fy < 16: ceil(n_fft /
// kFftBlock), at most kWelchCmfftMaxAcc; fy >= 16: none).  Workspace: B * chunks * n_fft chunk sums, then (blocks > 1) B * blocks *
// n_fft block sums.  The flags are kWelchCfftFlags.
constexpr uint32_t kWelchCmfftMaxAcc = 8;             // ceil(2025 / 256)
struct BhwWelchCmfftPlan : BhwWelchRuns { // bins = n_fft: the estimate is two-sided
    BhwStftCmfftPlan fft; // groups and grid as in the base; rows = B * frames; the y strides are 0; power false
};
// Every check of the two calls that needs no table handle, before any HIP call and in the order of include/bhw.h: the checks of
// bhwp_stft_cmfft_checks, then the output side of bhwp_welch_cfft_checks (one text for both).  frames 0 passes with the pointers
// unchecked; `pointers` false: the describe call.
int  bhwp_welch_cmfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint64_t p_stride,
                             const void *d_x, const void *d_P, const void *workspace, uint64_t workspace_bytes, bool pointers = true);
// bhw_welch_cmfft_workspace_bytes: from batch, frames and n_fft alone (0 for a NULL descriptor, frames 0 or a product beyond 2^60)
uint64_t bhwp_welch_cmfft_workspace_bytes(const bhw_stft *s);
BhwWelchCmfftPlan bhwp_welch_cmfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                        bool from_table);
int  bhwp_describe_welch_cmfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                               uint64_t len);
int  bhwk_welch_cmfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwWelchCmfftPlan &pl, const bhw_stft *s,
                          double scale, const float *d_x, float *d_P, double *d_ws, const int32_t *d_table, const BhwLenPhase &lp);

// ---- fused max-hold / min-hold traces for I/Q input (bhw_hold_cfft_f32_*, bhw_hold_cmfft_f32_*; bhw_hold_cfft.hip, bhw_hold_cmfft.hip) -----
// The plan of a hold call IS the plan of its Welch sibling (welch: the lanes, LDS, schedule, runs, chunks, blocks, grids and the
// workspace bytes, field for field) plus the traces that are stored.  A (max, min) pair of float32 words is the 8 bytes of a chunk sum,
// so bhwp_welch_runs' figures hold unchanged; welch.acc counts the PAIRS a lane carries over a run here (at most kHoldMaxAcc).
constexpr uint32_t kHoldMaxAcc = 8;                   // kWelchCfftMaxAcc, kWelchCmfftMaxAcc
struct BhwHoldCfftPlan {
    BhwWelchCfftPlan welch;
    uint32_t traces;      // BHW_HOLD_MAX | BHW_HOLD_MIN: what is stored (both are always computed)
};
struct BhwHoldCmfftPlan {
    BhwWelchCmfftPlan welch;
    uint32_t traces;
};
// Every check of the calls that needs no table handle, before any HIP call and in the order of include/bhw.h: the Welch sibling's
// check function for everything but the pointers (bhwp_welch_cfft_checks / bhwp_welch_cmfft_checks, `pointers` false), then the two
// outputs and the workspace (one text for both families).  frames 0 passes with the pointers unchecked; `pointers` false: the
// describe call.
int  bhwp_hold_cfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint64_t p_stride,
                           const void *d_x, const void *d_max, const void *d_min, const void *workspace, uint64_t workspace_bytes,
                           bool pointers = true);
int  bhwp_hold_cmfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint64_t p_stride,
                            const void *d_x, const void *d_max, const void *d_min, const void *workspace, uint64_t workspace_bytes,
                            bool pointers = true);
// bhw_hold_c(m)fft_workspace_bytes: the Welch sibling's figure
uint64_t bhwp_hold_cfft_workspace_bytes(const bhw_stft *s);
uint64_t bhwp_hold_cmfft_workspace_bytes(const bhw_stft *s);
BhwHoldCfftPlan  bhwp_hold_cfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                     uint32_t traces, bool from_table);
BhwHoldCmfftPlan bhwp_hold_cmfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                      uint32_t traces, bool from_table);
// traces: a non-empty subset of BHW_HOLD_MAX | BHW_HOLD_MIN (checked by the caller)
int  bhwp_describe_hold_cfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                             uint32_t traces, char *buf, uint64_t len);
int  bhwp_describe_hold_cmfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                              uint32_t traces, char *buf, uint64_t len);
int  bhwp_hold_traces_check(uint32_t traces);
int  bhwk_hold_cfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwHoldCfftPlan &pl, const bhw_stft *s,
                        double scale, const float *d_x, float *d_max, float *d_min, void *d_ws, const int32_t *d_table,
                        const BhwLenPhase &lp);
int  bhwk_hold_cmfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwHoldCmfftPlan &pl, const bhw_stft *s,
                         double scale, const float *d_x, float *d_max, float *d_min, void *d_ws, const int32_t *d_table,
                         const BhwLenPhase &lp);

// ---- fused Welch PSD at mixed-radix n_fft (bhw_welch_mfft_f32_*; bhw_welch_mfft.hip) --------------------------------------------------------
// BhwWelchMfftPlan wraps BhwStftMfftPlan as BhwWelchCfftPlan wraps BhwStftCfftPlan: the lanes, LDS, schedule and row steps are
// bhwp_stft_mfft_plan's field for field (fft, form BHWP_MFFT_SPECTRUM, with groups and grid recounted), the ownership is
// bhwp_welch_runs' with bins = K = n_fft / 2 + 1.  fy is a power of two from 1 to 64 at these sizes (64 for n_fft <= 32, 1 from 1080
// on), so run = max(16, fy) and gpr = max(1, 16 / fy) hold unchanged.  acc: the binary64 accumulators a lane carries over a run
// (fy < 16: ceil(K / kFftBlock), at most kWelchMfftMaxAcc; fy >= 16: none).  Workspace: B * chunks * K chunk sums, then (blocks > 1)
// B * blocks * K block sums.
constexpr uint32_t kWelchMfftMaxAcc = 8;              // ceil(2026 / 256): n_fft 4050
struct BhwWelchMfftPlan : BhwWelchRuns {  // bins = K = n_fft / 2 + 1: the estimate is one-sided
    BhwStftMfftPlan fft;  // groups and grid as in the base; rows = B * frames; the y strides are 0; form BHWP_MFFT_SPECTRUM
};
// Every check of the two calls that needs no table handle, before any HIP call and in the order of include/bhw.h.  frames 0 passes
// with the pointers unchecked; `pointers` false: the describe call.
int  bhwp_welch_mfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint32_t psd_flags,
                            uint64_t p_stride, const void *d_x, const void *d_P, const void *workspace, uint64_t workspace_bytes,
                            bool pointers = true);
// bhw_welch_mfft_workspace_bytes: from batch, frames and n_fft alone (0 for a NULL descriptor, frames 0 or a product beyond 2^60)
uint64_t bhwp_welch_mfft_workspace_bytes(const bhw_stft *s);
BhwWelchMfftPlan bhwp_welch_mfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                      bool from_table);
int  bhwp_describe_welch_mfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                              uint64_t len);
int  bhwk_welch_mfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwWelchMfftPlan &pl, const bhw_stft *s,
                         double scale, uint32_t psd_flags, const float *d_x, float *d_P, double *d_ws, const int32_t *d_table,
                         const BhwLenPhase &lp);

// ---- fused max-hold / min-hold traces for real input (bhw_hold_fft_f32_*, bhw_hold_mfft_f32_*; bhw_hold_fft.hip, bhw_hold_mfft.hip) --------
// As BhwHoldCfftPlan: the plan of a hold call IS the plan of its Welch sibling (bins = K = n_fft / 2 + 1) plus the traces that are
// stored, and a (max, min) pair of float32 words is the 8 bytes of a chunk sum.  welch.acc counts the PAIRS a lane carries over a run
// (at most kHoldFftMaxAcc, the ninth being bin M on lane 0 at n_fft 4096; kHoldMfftMaxAcc).
constexpr uint32_t kHoldFftMaxAcc = kWelchFftMaxAcc;  // 9
constexpr uint32_t kHoldMfftMaxAcc = kWelchMfftMaxAcc; // 8
struct BhwHoldFftPlan {
    BhwWelchFftPlan welch;
    uint32_t traces;      // BHW_HOLD_MAX | BHW_HOLD_MIN: what is stored (both are always computed)
};
struct BhwHoldMfftPlan {
    BhwWelchMfftPlan welch;
    uint32_t traces;
};
// Every check of the calls that needs no table handle, before any HIP call and in the order of include/bhw.h: the Welch sibling's
// check function for everything but the pointers (bhwp_welch_fft_checks / bhwp_welch_mfft_checks, `pointers` false), then the two
// outputs and the workspace (hold_pointer_checks, the I/Q hold calls' text with K bins and T floats of a signal).  frames 0 passes
// with the pointers unchecked; `pointers` false: the describe call.
int  bhwp_hold_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint32_t psd_flags,
                          uint64_t p_stride, const void *d_x, const void *d_max, const void *d_min, const void *workspace,
                          uint64_t workspace_bytes, bool pointers = true);
int  bhwp_hold_mfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, double scale, uint32_t psd_flags,
                           uint64_t p_stride, const void *d_x, const void *d_max, const void *d_min, const void *workspace,
                           uint64_t workspace_bytes, bool pointers = true);
// bhw_hold_(m)fft_workspace_bytes: the Welch sibling's figure
uint64_t bhwp_hold_fft_workspace_bytes(const bhw_stft *s);
uint64_t bhwp_hold_mfft_workspace_bytes(const bhw_stft *s);
BhwHoldFftPlan  bhwp_hold_fft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                   uint32_t traces, bool from_table);
BhwHoldMfftPlan bhwp_hold_mfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint64_t p_stride,
                                    uint32_t traces, bool from_table);
// traces: a non-empty subset of BHW_HOLD_MAX | BHW_HOLD_MIN (checked by the caller)
int  bhwp_describe_hold_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                            uint32_t traces, char *buf, uint64_t len);
int  bhwp_describe_hold_mfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags,
                             uint32_t traces, char *buf, uint64_t len);
int  bhwk_hold_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwHoldFftPlan &pl, const bhw_stft *s,
                       double scale, uint32_t psd_flags, const float *d_x, float *d_max, float *d_min, void *d_ws, const int32_t *d_table,
                       const BhwLenPhase &lp);
int  bhwk_hold_mfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwHoldMfftPlan &pl, const bhw_stft *s,
                        double scale, uint32_t psd_flags, const float *d_x, float *d_max, float *d_min, void *d_ws, const int32_t *d_table,
                        const BhwLenPhase &lp);

// ---- fused inverse real FFT, window and overlap-add (bhw_istft_fft_f32_*; bhw_istft_fft.hip) ------------------------------------------
// The lane layout of the forward kernel (lpf lanes along a row, fy slots side by side, cpl columns per lane).  The window-start axis
// w = t + pad - col0 of every signal (frame f covers w in [f * hop, f * hop + L)) is cut into spans of S * hop positions; the spans
// (b, s) of the batch are one pool cut into groups of fy consecutive spans, one per slot; workgroup g takes the groups g, g + grid, ...
// A slot walks, in ascending f, every frame that reaches its span's outputs -- at most S of its own and halo = ceil(L / hop) - 1
// before them, which the previous span transforms too -- and adds (double) r * (double) v into a ring of n_fft binary64 accumulators
// per slot, cpl of them (and cpl of the envelope) in the registers of each lane: ring position w mod n_fft belongs to lane
// (w mod n_fft) mod lpf.  After frame f every w < (f + 1) * hop is complete, is stored and cleared.
// S: the largest span that still leaves kIfftTargetGroups groups, but at least kIfftHaloFactor * halo frames, so that at most one
// transform in kIfftHaloFactor + 1 is a repeat.  LDS: the two Stockham buffers of fy * M complex64, the n_fft / 2 conjugated
// twiddles and the n_fft floats of the window (a function of n_fft alone, 64 KiB at 4096).
constexpr uint32_t kIfftTargetGroups = 1024;          // span groups the planner asks for before spans grow (four per CU)
constexpr uint32_t kIfftHaloFactor = 4;               // S >= 4 * halo
// The span plan of every fused inverse call (real and I/Q output, both radix families), from the descriptor, the flags, the fy slots
// of the family's forward plan, the floats of a spectrum row and the floats of an output sample: one text (istft_runs in
// bhw_plan.cpp) for the four bhwp_istft_*_plan.
struct BhwIstftRuns {
    int route;            // BHWP_FRAMES_DIRECT or BHWP_FRAMES_TABLE
    bool normalize;
    uint64_t t0;          // pad - col0: output t is position w = t + t0
    uint64_t hop;         // min(hop, t0 + samples): a larger hop leaves frame 0 alone under the outputs either way
    uint64_t halo;        // ceil(L / hop) - 1
    uint64_t span;        // S
    uint64_t spans;       // spans per signal: ceil((t0 + samples) / (S * hop))
    uint64_t groups;      // ceil(batch * spans / fy)
    uint64_t grid;        // min(groups, kFftMaxGrid)
    uint64_t trips;       // frames one slot walks at most: min(S + halo, frames)
    bool halo_bound;      // S was set by the halo, not by the grid target: few workgroups under heavy overlap
    uint64_t x_stride, y_stride, y_bstride;   // resolved, in floats (0 -> samples, 2K, frames * y_stride; I/Q: 2 * samples, 2 * n_fft)
    uint64_t len;         // L
};
// An inverse plan IS the span plan (its base: pl.t0, pl.trips, ...) plus the lane and radix fields of the family's forward plan.
struct BhwIstftFftPlan : BhwIstftRuns {
    uint32_t log2n, m, lpf, fy, cpl, radix4, radix2;   // as BhwStftFftPlan
    uint32_t lds_bytes;   // 2 * fy * M * 8 + M * 8 + n_fft * 4  (<= 64 KiB)
};
// Span s of a signal: its outputs [wlo, whi) on the w axis and the frames [f_lo, f_hi) that reach them (both may be empty).
struct BhwIstftSpan {
    uint64_t wlo, whi, f_lo, f_hi;
};
BHW_HD inline BhwIstftSpan bhwp_istft_span(uint64_t s, uint64_t span, uint64_t hop, uint64_t len, uint64_t t0, uint64_t samples, uint64_t frames)
{
    BhwIstftSpan r;
    const uint64_t a = s * span * hop, b = a + span * hop, end = t0 + samples;
    r.wlo = a > t0 ? a : t0;
    r.whi = b < end ? b : end;
    if (r.whi <= r.wlo) {
        r.whi = r.wlo;
        r.f_lo = r.f_hi = 0;
        return r;
    }
    r.f_lo = r.wlo >= len ? (r.wlo - len) / hop + 1 : 0;                  // f * hop + L > wlo
    r.f_hi = (r.whi - 1) / hop + 1;                                       // f * hop < whi
    if (r.f_hi > frames) r.f_hi = frames;
    if (r.f_lo > r.f_hi) r.f_lo = r.f_hi;
    return r;
}
// Every check of the two calls that needs no table handle, before any HIP call (include/bhw.h).  samples 0 passes with the pointers
// unchecked; `pointers` false: the describe call.
int  bhwp_istft_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_Y, const void *d_x,
                           bool pointers = true);
// the plan of a call that passed the checks with samples > 0
BhwIstftFftPlan bhwp_istft_fft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table);
int  bhwp_describe_istft_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                             uint64_t len);
int  bhwk_istft_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwIstftFftPlan &pl, const bhw_stft *s,
                        const float *d_Y, float *d_x, const int32_t *d_table, const BhwLenPhase &lp);

// ---- fused STFT, spectral mask and inverse STFT (bhw_mask_fft_f32_*; bhw_mask_fft.hip) -------------------------------------------------
// The inverse kernel with its frames formed from the signal: the plan IS bhwp_istft_fft_plan of the synthesis descriptor, field for
// field, but for the LDS, which holds a second (forward) twiddle table: 40 960 bytes at 2048, the largest n_fft (at 4096 the inverse
// alone fills the 64 KiB).  Beside it the resolved strides of what the frame source reads.
constexpr uint32_t kMaskFftMaxLog = 11;               // n_fft <= 2048
struct BhwMaskFftPlan : BhwIstftFftPlan {             // lds_bytes: 2 * fy * M * 8 + 2 * M * 8 + n_fft * 4  (<= 40 KiB)
    uint64_t in_stride;   // floats between the input signals (0 -> the analysis descriptor's samples)
    uint64_t g_stride, g_bstride;   // gains (floats; pairs for bhw_cmask_*) between the gain rows of a signal and between the signals' gains, as given (0: one row)
};
// Every check of the two calls that needs no table handle, before any HIP call and in the order of include/bhw.h: the params, the two
// descriptors by the checks of bhw_stft_fft_f32_* and bhw_istft_fft_f32_* (in their words), the rules that tie them, the gain strides,
// the pointers and the overlaps.  ss->samples 0 passes with the pointers unchecked; `pointers` false: the describe call.
int  bhwp_mask_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                          const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers = true);
// the plan of a call that passed the checks with ss->samples > 0
BhwMaskFftPlan bhwp_mask_fft_plan(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                                  uint64_t g_stride, uint64_t g_batch_stride, bool from_table);
int  bhwp_describe_mask_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                            uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);
int  bhwk_mask_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwMaskFftPlan &pl, const bhw_stft *sa,
                       const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp);
// The same call with a complex gain per bin (bhw_cmask_fft_f32_*; k_cmask_fft_* in bhw_mask_fft.hip): d_g holds interleaved float32 pairs
// (gr, gi) and both gain strides count pairs.  The checks are bhwp_mask_fft_checks' with 8-byte gain elements (extents, overlaps, an
// 8-byte aligned d_g) and refusals that name the complex-gain call of the other family; the plan IS bhwp_mask_fft_plan's, strides in
// pairs: the gains live in registers, so lanes, spans, columns and LDS do not change.
int  bhwp_cmask_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                           const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers = true);
int  bhwp_describe_cmask_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                             uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);
int  bhwk_cmask_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwMaskFftPlan &pl, const bhw_stft *sa,
                        const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp);

// ---- fused inverse mixed-radix FFT, window and overlap-add (bhw_istft_mfft_f32_*; bhw_istft_mfft.hip) ---------------------------------
// The lane layout and the radix schedule of bhwp_stft_mfft_plan (lpf lanes along a row of M = n_fft / 2 complex points, fy slots side
// by side, cpl = ceil(n_fft / lpf) ring positions per lane, the last of which need not exist) under the span plan (BhwIstftRuns: the
// same S, halo, trips, halo_bound, grid cap and hop clamp) and bhwp_istft_span as it is.  LDS is BhwIstftFftPlan's formula: 16 000
// bytes at n_fft 400, 64 800 at 4050, the largest.
struct BhwIstftMfftPlan : BhwIstftRuns {
    uint32_t m, lpf, fy, cpl, passes;                  // as BhwStftMfftPlan
    uint8_t radix[kMfftMaxPasses];
    uint32_t lds_bytes;   // 2 * fy * M * 8 + M * 8 + n_fft * 4  (<= 64 800)
};
// Every check of the two calls that needs no table handle, before any HIP call (include/bhw.h).  samples 0 passes with the pointers
// unchecked; `pointers` false: the describe call.
int  bhwp_istft_mfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_Y, const void *d_x,
                            bool pointers = true);
// the plan of a call that passed the checks with samples > 0
BhwIstftMfftPlan bhwp_istft_mfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table);
int  bhwp_describe_istft_mfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                              uint64_t len);
int  bhwk_istft_mfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwIstftMfftPlan &pl, const bhw_stft *s,
                         const float *d_Y, float *d_x, const int32_t *d_table, const BhwLenPhase &lp);

// ---- fused STFT, spectral mask and inverse STFT at mixed-radix n_fft (bhw_mask_mfft_f32_*; bhw_mask_mfft.hip) ---------------------------
// The inverse mixed-radix kernel with its frames formed from the signal, as BhwMaskFftPlan is the power-of-two one: the plan IS
// bhwp_istft_mfft_plan of the synthesis descriptor, field for field, but for the LDS, which holds a second (forward) twiddle table:
// 40 000 bytes at 2000, the largest n_fft.  Below 2048 the forward planner gives lpf >= n_fft / 8, so a lane keeps at most 8 ring
// columns; the 22 sizes from 2160 to 4050 need 16 and up to 81 000 bytes, and are refused.
constexpr uint32_t kMaskMfftMaxN = 2047;              // n_fft < 2048
struct BhwMaskMfftPlan : BhwIstftMfftPlan {           // lds_bytes: 2 * fy * M * 8 + 2 * M * 8 + n_fft * 4  (<= 40 000)
    uint64_t in_stride;   // floats between the input signals (0 -> the analysis descriptor's samples)
    uint64_t g_stride, g_bstride;   // gains (floats; pairs for bhw_cmask_*) between the gain rows of a signal and between the signals' gains, as given (0: one row)
};
// Every check of the two calls that needs no table handle, before any HIP call and in the order of include/bhw.h: the params, the
// refusals that name a route, the two descriptors by the checks of bhw_stft_mfft_f32_* and bhw_istft_mfft_f32_* (in their words), then
// what bhwp_mask_fft_checks checks after its parents, from the same function.  `pointers` false: the describe call.
int  bhwp_mask_mfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                           const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers = true);
// the plan of a call that passed the checks with ss->samples > 0
BhwMaskMfftPlan bhwp_mask_mfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                                    uint64_t g_stride, uint64_t g_batch_stride, bool from_table);
int  bhwp_describe_mask_mfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                             uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);
int  bhwk_mask_mfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwMaskMfftPlan &pl, const bhw_stft *sa,
                        const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp);
// The same call with a complex gain per bin (bhw_cmask_mfft_f32_*; k_cmask_mfft_* in bhw_mask_mfft.hip), as bhwp_cmask_fft_checks and
// its siblings are the power-of-two one: pairs (gr, gi), strides in pairs, bhwp_mask_mfft_plan as it is.
int  bhwp_cmask_mfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                            const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers = true);
int  bhwp_describe_cmask_mfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                              uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);
int  bhwk_cmask_mfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwMaskMfftPlan &pl, const bhw_stft *sa,
                         const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp);

// ---- fused multichannel filter-and-sum (bhw_beam_fft_f32_*, bhw_beam_mfft_f32_*; k_beam_* in bhw_mask_fft.hip / bhw_mask_mfft.hip;
// ---- DESIGN.md section 45) --------------------------------------------------------------------------------------------------------------
// The complex-gain mask over n_ch channels of each signal, summed per bin before the one inverse transform.  The channel axis of a
// call: the channel count and the strides between the channels of one signal, of d_x in floats (0: the analysis samples) and of d_g
// in pairs.
struct BhwBeamAxis {
    uint32_t n_ch;
    uint64_t x_ch_stride, g_ch_stride;
};
// The plans ARE bhwp_mask_fft_plan's / bhwp_mask_mfft_plan's for the B output signals, field for field (the sums live in registers:
// lanes, spans, columns per lane and LDS do not change), beside the channel axis resolved; in_stride 0 resolves to n_ch channel strides.
struct BhwBeamFftPlan : BhwMaskFftPlan {
    uint32_t n_ch;
    uint64_t x_cstride, g_cstride;
};
struct BhwBeamMfftPlan : BhwMaskMfftPlan {
    uint32_t n_ch;
    uint64_t x_cstride, g_cstride;
};
// The checks of bhwp_cmask_[m]fft_checks in their order, about "the fused beamformer", with the channel axis: n_ch and the channel
// strides behind the fields that must agree, extents with the channel axis, d_out against every channel of d_x and against d_g.
int  bhwp_beam_fft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                          const BhwBeamAxis &ch, const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out,
                          bool pointers = true);
int  bhwp_beam_mfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                           const BhwBeamAxis &ch, const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out,
                           bool pointers = true);
BhwBeamFftPlan  bhwp_beam_fft_plan(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                                   const BhwBeamAxis &ch, uint64_t g_stride, uint64_t g_batch_stride, bool from_table);
BhwBeamMfftPlan bhwp_beam_mfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                                    const BhwBeamAxis &ch, uint64_t g_stride, uint64_t g_batch_stride, bool from_table);
int  bhwp_describe_beam_fft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                            uint32_t flags, const BhwBeamAxis &ch, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);
int  bhwp_describe_beam_mfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                             uint32_t flags, const BhwBeamAxis &ch, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);
int  bhwk_beam_fft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwBeamFftPlan &pl, const bhw_stft *sa,
                       const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp);
int  bhwk_beam_mfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwBeamMfftPlan &pl, const bhw_stft *sa,
                        const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp);

// ---- fused inverse complex FFT, window and overlap-add for I/Q output (bhw_istft_cfft_f32_*; bhw_istft_cfft.hip) ----------------------
// The lane layout and the passes of bhwp_stft_cfft_plan (lpf lanes along a row of n = n_fft complex points, fy slots side by side,
// cpl complex columns per lane) under the span plan (BhwIstftRuns: the same S, halo, trips, halo_bound, grid cap and hop clamp, the
// strides in floats of two per sample) and bhwp_istft_span as it is.  A lane keeps cpl ring positions of two binary64
// sums (re, im) and one envelope sum.  LDS: the two Stockham buffers of fy * n complex64, the n / 2 conjugated twiddles and the n
// floats of the window: 48 KiB at 2048, three workgroups on a CU.
constexpr uint32_t kIcfftFlags = BHW_OLA_NORMALIZE | BHW_CFFT_SHIFT;
struct BhwIstftCfftPlan : BhwIstftRuns {
    bool shifted;
    uint32_t log2n, n, lpf, fy, cpl, radix4, radix2;   // as BhwStftCfftPlan
    uint32_t lds_bytes;   // 2 * fy * n * 8 + n / 2 * 8 + n * 4  (<= 48 KiB)
};
// Every check of the two calls that needs no table handle, before any HIP call and in the order of include/bhw.h.  samples 0 passes
// with the strides and the pointers unchecked; `pointers` false: the describe call.
int  bhwp_istft_cfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_Y, const void *d_x,
                            bool pointers = true);
// the plan of a call that passed the checks with samples > 0
BhwIstftCfftPlan bhwp_istft_cfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table);
int  bhwp_describe_istft_cfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                              uint64_t len);
int  bhwk_istft_cfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwIstftCfftPlan &pl, const bhw_stft *s,
                         const float *d_Y, float *d_x, const int32_t *d_table, const BhwLenPhase &lp);

// ---- fused inverse mixed-radix complex FFT, window and overlap-add for I/Q output (bhw_istft_cmfft_f32_*; bhw_istft_cmfft.hip) --------
// The lane layout, the radix schedule and the twiddle-table form of bhwp_stft_cmfft_plan (lpf lanes along a row of n = n_fft complex
// points, fy slots side by side, cpl = ceil(n / lpf) <= kCfftMaxCpl ring positions per lane, the last of which need not exist; fold
// entries of the FORWARD table exp(-2 pi i k / n): the kernel swaps the parts of its input and of its result instead of conjugating
// the transform) under the span plan (BhwIstftRuns: the same S, halo, trips, halo_bound, grid cap and hop clamp, the strides in
// floats of two per sample) and bhwp_istft_span as it is.  A lane keeps cpl ring positions of two binary64 sums
// (re, im) and one envelope sum.  LDS: the two Stockham buffers of fy * n complex64, the fold twiddles and the n floats of the
// window: 48 000 bytes at 2000, 56 700 at 2025, the largest.
struct BhwIstftCmfftPlan : BhwIstftRuns {
    bool shifted;
    uint32_t n, fold, lpf, fy, cpl, passes;            // as BhwStftCmfftPlan
    uint8_t radix[kMfftMaxPasses];
    uint32_t lds_bytes;   // 2 * fy * n * 8 + fold * 8 + n * 4  (<= 56 700)
};
// Every check of the two calls that needs no table handle, before any HIP call and in the order of bhwp_istft_cfft_checks.  samples 0
// passes with the strides and the pointers unchecked; `pointers` false: the describe call.
int  bhwp_istft_cmfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const void *d_Y, const void *d_x,
                             bool pointers = true);
// the plan of a call that passed the checks with samples > 0
BhwIstftCmfftPlan bhwp_istft_cmfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, bool from_table);
int  bhwp_describe_istft_cmfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf,
                               uint64_t len);
int  bhwk_istft_cmfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwIstftCmfftPlan &pl, const bhw_stft *s,
                          const float *d_Y, float *d_x, const int32_t *d_table, const BhwLenPhase &lp);

// ---- fused STFT, real or complex gain per bin and inverse STFT for I/Q input (bhw_[c]mask_cfft_f32_*, bhw_[c]mask_cmfft_f32_*;
// ---- bhw_mask_cfft.hip, bhw_mask_cmfft.hip) ----------------------------------------------------------------------
// The inverse I/Q kernels with their frames formed from the signal, as BhwMaskFftPlan is the real-signal one: each plan IS
// bhwp_istft_cfft_plan / bhwp_istft_cmfft_plan of the synthesis descriptor, field for field, but for the LDS of the power-of-two
// family, which holds a second (forward) twiddle table of n / 2 entries: 56 KiB at 2048 where the parent has 48, two workgroups on a
// CU by LDS where the parent has three.  The mixed-radix parent already runs the forward passes over the forward table, so its LDS
// bytes stand.  `shifted` (BHW_CFFT_SHIFT in flags) is of the gain columns here: the gain of bin k is in column (k + n_fft / 2) mod
// n_fft, where the parents keep bin k under the same flag.  K = n_fft gains a row; in_stride counts floats, two per sample.
struct BhwMaskCfftPlan : BhwIstftCfftPlan {           // lds_bytes: 2 * fy * n * 8 + 2 * (n / 2) * 8 + n * 4  (<= 56 KiB)
    uint64_t in_stride;   // floats between the input signals (0 -> 2 * the analysis descriptor's samples)
    uint64_t g_stride, g_bstride;   // gains (floats; pairs for bhw_cmask_*) between the gain rows of a signal and between the signals' gains, as given (0: one row)
};
struct BhwMaskCmfftPlan : BhwIstftCmfftPlan {         // lds_bytes: the parent's
    uint64_t in_stride;
    uint64_t g_stride, g_bstride;
};
// Every check of the calls that needs no table handle, before any HIP call: the params, the refusals that name a route, the two
// descriptors by the checks of bhw_stft_c[m]fft_f32_* (flags 0: detrending is refused with the flag bits) and bhw_istft_c[m]fft_f32_*
// (in their words, packed row strides), then mask_tail_checks with K = n_fft and two floats a sample.  bhwp_cmask_*: 8-byte gains.
int  bhwp_mask_cfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                           const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers = true);
int  bhwp_cmask_cfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                            const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers = true);
int  bhwp_mask_cmfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                            const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers = true);
int  bhwp_cmask_cmfft_checks(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const void *d_x,
                             const void *d_g, uint64_t g_stride, uint64_t g_batch_stride, const void *d_out, bool pointers = true);
// the plans of a call that passed the checks with ss->samples > 0 (one per family: the pair-gain calls run it with strides in pairs)
BhwMaskCfftPlan  bhwp_mask_cfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                                     uint64_t g_stride, uint64_t g_batch_stride, bool from_table);
BhwMaskCmfftPlan bhwp_mask_cmfft_plan(const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                                      uint64_t g_stride, uint64_t g_batch_stride, bool from_table);
int  bhwp_describe_mask_cfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                             uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);
int  bhwp_describe_cmask_cfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                              uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);
int  bhwp_describe_mask_cmfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                              uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);
int  bhwp_describe_cmask_cmfft(const bhw_params *p, const BhwCordicCfg *ct, uint64_t length, const bhw_stft *sa, const bhw_stft *ss,
                               uint32_t flags, uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);
int  bhwk_mask_cfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwMaskCfftPlan &pl, const bhw_stft *sa,
                        const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp);
int  bhwk_cmask_cfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwMaskCfftPlan &pl, const bhw_stft *sa,
                         const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp);
int  bhwk_mask_cmfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwMaskCmfftPlan &pl, const bhw_stft *sa,
                         const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp);
int  bhwk_cmask_cmfft_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwMaskCmfftPlan &pl, const bhw_stft *sa,
                          const bhw_stft *ss, const float *d_x, const float *d_g, float *d_out, const int32_t *d_table, const BhwLenPhase &lp);

// the generate kernel of a window of any length (bhw_len.hip): d_table NULL = k_direct_len, else k_range_len over the resident table of c
int  bhwk_len_range(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *d_table, const BhwLenPhase &lp,
                    uint64_t n0, uint64_t count, int32_t *d_out);
