/*
 * bhw.h -- C ABI of the MI355X fixed-point window-coefficient generator.
 *
 * Drop-in boundary for the reference's coefficient source.  The reference
 * (hukenovs/blackman_harris_win) has no FFI layer; what a consumer binds is
 *   - the `win_selector` entity, src/win_selector.vhd:60-87
 *       generics PHI_WIDTH, DAT_WIDTH, WIN_TYPE, SIN_TYPE, LUT_SIZE, XSERIES
 *       ports    AA0..AA6 (integer weights), ENABLE, DT_WIN, DT_VLD
 *   - the HLS top   void win_function(char win_type, phi_t i, win_t *out)
 *                                             hls/windows/win_function.h:65-69
 *   - the CORDIC    void cordic(phi_t, win_t *cos, win_t *sin)
 *                                             hls/windows/win_function.cpp:47-51
 *                   void cordic(int theta, long long *lut, int *s, int *c)
 *                                             cpp/cordic_sincos.cpp:10
 * Each entry point below names the reference interface it replaces.
 *
 * Plain C types only: pointers, sizes, PODs.  No exceptions cross the ABI.
 * All compute runs in hand-written HIP kernels on the selected device; there is
 * no CPU fallback -- without a usable HIP device every compute entry point
 * returns BHW_ERR_HIP.
 */
#ifndef BHW_H
#define BHW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BHW_ABI_VERSION 4u   /* 3: bhw_coeffs_preset, bhw_gather_parts_device; 4: bhw_workspace_bytes_ex (nothing removed or changed);
                                the resident tables, the overlapped-frame apply, the overlap-add and the windows of any length
                                were added without a bump (additions only), as were the float32, STFT and Welch calls and the fused
                                window + FFT calls (bhw_stft_fft_f32_*) */

/* CORDIC bit-model (the reference holds three that are not bit-identical). */
enum {
    BHW_MODEL_HLS  = 0,  /* hls/windows/win_function.cpp:47-156 (= hls/cordic/cordic.cpp)   */
    BHW_MODEL_CPP  = 1,  /* cpp/cordic_sincos.cpp:10-92                                      */
    BHW_MODEL_VHDL = 2,  /* src/cordic_dds.vhd:94-249                                        */
    /* The two variant generators of the repository: accepted by bhw_sincos_* only (no window entity instantiates them,
     * so window generation with them is BHW_ERR_UNSUPPORTED).  As written upstream they deliver DT_COS = +cos, DT_SIN = -sin
     * at amplitude 2^(DATA_WIDTH-2) (x/y update sense of src/cordic_dds48.vhd:234-242). */
    BHW_MODEL_DDS48  = 3, /* src/cordic_dds48.vhd:94-260: 48-bit data path, quadrant folded into the start vector */
    BHW_MODEL_SCALED = 4  /* src/cordic_dds_scaled.vhd:98-286: data path SEL_SIZE(DATA_WIDTH-8) bits (:102-107)  */
};
/* Cosine-sum rule. */
enum {
    BHW_COMBINE_HLS  = 0, /* truncating shift, no rounding: hls/windows/win_function.cpp:168-377 */
    BHW_COMBINE_VHDL = 1  /* per-product round + final round: src/bh_win_7term.vhd:353-438 etc.  */
};
/* SIN_TYPE generic of win_selector (src/win_selector.vhd:66).  The reference wires the Taylor source only into the
 * 2- and 3-term windows (src/win_selector.vhd:93-135; the BH4/5/7 entities take no SIN_TYPE, :137-199), so
 * BHW_SIN_TAYLOR with more terms is BHW_ERR_UNSUPPORTED here and the win_selector mirrors fall back to CORDIC exactly as
 * the reference's selector does.  BHW_SIN_TAYLOR_ALL is this library's extension: harmonic
 * k = m * 2^v (m odd) is read from a taylor_sincos generator of PHASE_WIDTH - v at phase (m * n) mod 2^(PHASE_WIDTH - v)
 * -- the rule bh_win_3term.vhd:221-226 applies to its 2nd harmonic, continued to k = 3..6.  For 2 and 3 terms it is
 * identical to BHW_SIN_TAYLOR; for more terms no reference output exists (the oracle defines it). */
enum { BHW_SIN_CORDIC = 0, BHW_SIN_TAYLOR = 1, BHW_SIN_TAYLOR_ALL = 2 };
/* win_type codes of win_function() (hls/windows/win_function.cpp:391-420). */
enum { BHW_WIN_HAMMING = 1, BHW_WIN_HANN = 2, BHW_WIN_BH3 = 3, BHW_WIN_BH4 = 4, BHW_WIN_BH5 = 5, BHW_WIN_BH7 = 7 };
/* Execution strategy (results are bit-identical across strategies). */
enum {
    BHW_ALGO_AUTO   = 0,
    BHW_ALGO_DIRECT = 1, /* one lane per coefficient, K-1 CORDIC chains per lane              */
    BHW_ALGO_TABLE  = 2, /* first-quadrant CORDIC table built once per call, then gather-combine */
    BHW_ALGO_FUSED  = 3  /* whole periods in one launch, no table: one lane per eight coefficients (quadrant + half-period
                            fold), shared rotation prefixes per wave; ragged ends take BHW_ALGO_DIRECT.  Falls back to
                            BHW_ALGO_TABLE where it does not apply (34-bit+ CORDIC state, phi_width < 9)            */
};

enum {
    BHW_OK              = 0,
    BHW_ERR_BADARG      = -1,
    BHW_ERR_UNSUPPORTED = -2,
    BHW_ERR_HIP         = -3,
    BHW_ERR_WORKSPACE   = -4
};

/* The win_selector parameter surface as one POD (src/win_selector.vhd:61-81). */
typedef struct bhw_params {
    uint32_t struct_size;  /* sizeof(bhw_params), for ABI evolution                       */
    uint32_t model;        /* BHW_MODEL_*                                                 */
    uint32_t combine;      /* BHW_COMBINE_*                                               */
    uint32_t sin_type;     /* BHW_SIN_*                      SIN_TYPE                     */
    uint32_t win_type;     /* BHW_WIN_* (informational; n_terms + aa define the window)   */
    uint32_t n_terms;      /* 2,3,4,5,7                      WIN_TYPE                     */
    uint32_t phi_width;    /* 4..30, N = 2^phi_width         PHI_WIDTH (the reference documents up to 26,
                              README.md:2; 27..30 are the same arithmetic on a longer counter)          */
    uint32_t dat_width;    /* 8..32                          DAT_WIDTH                    */
    uint32_t precision;    /* model VHDL only, 1..7          cordic_dds PRECISION         */
    uint32_t lut_size;     /* Taylor only                    LUT_SIZE                     */
    int32_t  aa[7];        /* AA0..AA6, caller-scaled integer weights                     */
} bhw_params;

/* Storage format of the first-quadrant (c, s) table of BHW_ALGO_TABLE (results are bit-identical across formats;
 * a format that does not apply to a configuration falls back to the next wider one). */
enum {
    BHW_TABLE_BEST     = 0, /* narrowest format that is exact for the configuration                 */
    BHW_TABLE_PLAIN    = 1, /* int2 (c, s) per entry, 8 bytes                                       */
    BHW_TABLE_DELTA16  = 2, /* at most: 4 bytes per entry (int16 differences to a 64-entry block head) */
    BHW_TABLE_RESIDUAL = 3, /* at most: 2 bytes per entry against a linear predictor (8-bit fields) */
    BHW_TABLE_NIBBLE   = 4, /* at most: 1 byte per entry, the same predictor with 4-bit fields (what BEST tries first) */
    BHW_TABLE_NIBBLE_ESC = 5 /* at most: the same one-byte entries with a marker for the rare deviation beyond the fields, listed exactly
                                beside the table (second choice of BEST: models whose CORDIC noise is wider, cpp / VHDL at 32 bits)  */
};

/* Optional execution controls for the *_ex entry points. */
typedef struct bhw_exec {
    uint32_t struct_size;     /* sizeof(bhw_exec) (the 32-byte ABI-1 layout without table_format is accepted) */
    uint32_t algo;            /* BHW_ALGO_*                                                */
    void    *workspace;       /* device scratch (NULL: library-owned scratch of this stream) */
    uint64_t workspace_bytes;
    void    *event_after_build; /* optional hipEvent_t recorded on the stream between the table build and the
                                   combine pass (per-kernel timing for profilers); NULL = none      */
    uint32_t table_format;    /* BHW_TABLE_* (diagnostics / A-B runs; 0 = best)            */
    uint32_t reserved;        /* must be 0                                                 */
} bhw_exec;

uint32_t    bhw_abi_version(void);
const char *bhw_strerror(int code);
const char *bhw_last_error(void); /* thread-local detail of the last failure */

/* Defaults: model HLS, combine HLS, CORDIC source, precision 1, lut_size 9, built-in a_k
 * (hls/windows/win_function.cpp:173-355 constants and scaling). */
int bhw_params_init(bhw_params *p, uint32_t win_type, uint32_t phi_width, uint32_t dat_width);
int bhw_params_validate(const bhw_params *p);

/* a_k = round(coe_k * (2^(W-s)-1)), s = 1 (2/3/4-term) or 2 (5/7-term): the HLS derivation
 * (hls/windows/win_function.cpp:176-177,210-212,258-261,312-316,349-355).  a == NULL selects
 * the built-in constants of `win_type`.  Host arithmetic only (doubles -> 7 integers). */
int bhw_coeffs_from_float(uint32_t win_type, uint32_t dat_width, const double *a, int32_t aa[7]);

/* The named coefficient sets the reference lists beside its built-in ones (comments in hls/windows/win_function.cpp:241-250 and
 * :292-303, README.md:30-51): the float weights a[0..6] (unused terms 0), the window type that takes them, and -- when aa != NULL
 * -- the integer weights of the HLS derivation above for dat_width (bhw_coeffs_from_float(*win_type, dat_width, a, aa)).
 * Two upstream slips are not reproduced: the Nuttall a2 is the published 0.144232 (win_function.cpp:244 prints 0.144323, with
 * which the weights no longer sum to one), and flat-top (2) lists its fifth weight as a second "a3" (:302-303). */
enum {
    BHW_PRESET_NUTTALL          = 1,  /* 4-term: 0.355768, 0.487396, 0.144232, 0.012604                 -93 dB (README.md:35) */
    BHW_PRESET_BLACKMAN_NUTTALL = 2,  /* 4-term: 0.3635819, 0.4891775, 0.1365995, 0.0106411             -98 dB (README.md:37) */
    BHW_PRESET_FLATTOP_1        = 3,  /* 5-term: 0.25, 0.4925, 0.3225, 0.097, 0.0075  (win_function.cpp:292-297)             */
    BHW_PRESET_FLATTOP_2        = 4,  /* 5-term: 0.21557895, 0.41663158, 0.277263158, 0.083578947, 0.006947368 (:298-303)   */
    BHW_PRESET_BH7_README       = 5,  /* 7-term set of README.md:45-51 ("up to 180 dB")                                      */
    BHW_PRESET_BLACKMAN         = 6,  /* 3-term: 0.42, 0.5, 0.08                                         -58 dB (README.md:32) */
    BHW_PRESET_BH3              = 7   /* 3-term Blackman-Harris: 0.42323, 0.49755, 0.07922               -71 dB (README.md:33) */
};
int bhw_coeffs_preset(uint32_t preset, uint32_t dat_width, uint32_t *win_type, double a[7], int32_t aa[7]);

/* The 48-entry arctangent ROMs and gains the kernels use (which: 0 = T2 of the cpp model,
 * 1 = T4 of the HLS/VHDL models); gains[0] = G46, gains[1] = G47. */
int bhw_constant_tables(uint32_t which, int64_t table[48], int64_t gains[2]);

/* Replaces: ENABLE held high for `count` clocks on win_selector (src/win_selector.vhd:83-86)
 * after the phase counter reached n0; equivalently `for i in n0..n0+count: win_function(sel, i, &w)`
 * (hls/windows/window_test.cpp:93,193).  Writes count sign-extended int32 coefficients to d_out
 * (device memory of `device`), asynchronously on `hip_stream` (hipStream_t; NULL = default
 * stream).  n wraps modulo 2^phi_width like the hardware counter (src/bh_win_7term.vhd:92-97). */
int bhw_generate_device(const bhw_params *p, int device, void *hip_stream,
                        uint64_t n0, uint64_t count, int32_t *d_out);
int bhw_generate_device_ex(const bhw_params *p, int device, void *hip_stream,
                           uint64_t n0, uint64_t count, int32_t *d_out, const bhw_exec *ex);
/* Device scratch that is enough for the given call with `algo` whatever table format it ends up using (0 for the direct and
 * fused strategies): 8 bytes per first-quadrant table entry.  An upper bound that never changes for a configuration. */
uint64_t bhw_workspace_bytes(const bhw_params *p, uint64_t n0, uint64_t count, uint32_t algo);
/* The same for the call as `ex` describes it (algo, table_format), counting the table format(s) the call would use right now:
 * after bhw_prepare_device (or a first call) has settled the packed formats of the configuration this is the size of the one
 * format in use -- 16.5 MiB instead of 128 MiB for a 2^26-point window at 32 bits -- and it never grows afterwards.  A
 * workspace of at least this size is accepted by bhw_generate_device_ex / bhw_generate_part_device (bhw_apply_device takes no
 * bhw_exec: it always uses the library-owned scratch).  The library-owned scratch of a stream is sized by the same rule:
 * the formats are settled before it is sized, so a stream holds the settled format from its first call, prepared or not. */
uint64_t bhw_workspace_bytes_ex(const bhw_params *p, uint64_t n0, uint64_t count, const bhw_exec *ex);

/* What bhw_generate_device_ex(p, ..., n0, count, ..., ex) would launch right now, as one line of text into buf (NUL-terminated,
 * truncated to len): strategy, table format and the kernel names a profiler will show.  The table format of a configuration
 * is settled on its first use (or by bhw_prepare_device); before that the line says "unverified".  Host arithmetic only. */
int bhw_describe_plan(const bhw_params *p, uint64_t n0, uint64_t count, const bhw_exec *ex, char *buf, uint64_t len);

/* Does every lazy step of later calls with `p` on (device, hip_stream) now: uploads the Taylor quarter-wave ROM
 * (taylor_sincos.vhd:91-111 builds it at elaboration), allocates the library-owned table scratch of this stream, and verifies
 * once, on the device, that the packed table formats are exact for this (model, phi_width, dat_width, precision) -- a property
 * of the configuration, not of the weights.  Synchronous.  After it, bhw_generate_* / bhw_apply_* / bhw_sincos_* calls with
 * these widths on this stream neither allocate nor synchronise, so they can be captured into a HIP graph -- whole periods,
 * partial ranges and explicit bhw_exec.algo alike (the scratch is reserved also for configurations whose whole periods take the
 * table-free fused kernel).  The verdict of every packed format is settled, so an explicit bhw_exec.table_format never meets
 * an open one; the scratch is sized for table_format BEST (the narrowest exact format) and never shrinks, so what an earlier
 * prepare of this stream reserved for another configuration stays.  Two exceptions, both answered by
 * passing bhw_exec.workspace (bhw_workspace_bytes_ex bytes) inside a capture: a range WITHOUT a whole period of a window whose
 * plain table exceeds 64 MiB (phi_width >= 26 at z_shr = 0), and an explicit table_format wider than the one BEST resolves to --
 * either would have to grow the library scratch, which a capturing stream refuses (BHW_ERR_HIP).
 * Without prepare the first call does the same work inline (one synchronisation); during stream capture an unprepared Taylor
 * call fails with BHW_ERR_HIP and an unprepared table call uses the plain table format. */
int bhw_prepare_device(const bhw_params *p, int device, void *hip_stream);

/* Interleaved ownership of ONE window over several devices (every coefficient is an independent function of its
 * index, src/bh_win_7term.vhd:176-197 | hls/windows/win_function.cpp:361-375).  Contiguous index shards -- n0 = g * N / G with
 * bhw_generate_device -- cannot share CORDIC work between the quadrant images of a coefficient; an interleaved part can: part
 * `part` of `n_parts` owns a set of lanes r of the ring [0, N/8) together with the eight coefficients r + h*N/8 + j*N/4 of each,
 * so one first-quadrant CORDIC result still serves up to eight coefficients.  The ownership is a deterministic function of
 * (phi_width, dat_width, model, n_terms, n_parts): bhw_part_segments lists it as sorted contiguous index segments (at most
 * 256); the parts of one window cover [0, N) -- neighbouring parts may both own a few hundred coefficients at the seams of
 * the internal tiling, with identical values.
 * bhw_generate_part_device writes exactly the owned coefficients into d_window, the base of a full-length (2^phi_width)
 * int32 buffer on `device`; all other elements are left untouched.  CORDIC source only.  No collective is involved: a
 * consumer that wants the whole window on one device copies the segments (hipMemcpyPeerAsync). */
typedef struct bhw_segment {
    uint64_t n0;     /* first coefficient index */
    uint64_t count;  /* coefficients            */
} bhw_segment;
int bhw_part_segments(const bhw_params *p, uint32_t part, uint32_t n_parts, bhw_segment *segs, uint32_t capacity, uint32_t *n_segs);
int bhw_generate_part_device(const bhw_params *p, int device, void *hip_stream, uint32_t part, uint32_t n_parts,
                             int32_t *d_window, const bhw_exec *ex);

/* One window on one device from its `n_parts` interleaved ownership parts (optional, outside the metric).  Part g
 * was produced by bhw_generate_part_device(p, src_devices[g], ..., g, n_parts, d_windows[g]) into a full-length buffer on
 * src_devices[g]; every segment part g owns (bhw_part_segments) is copied into d_dst, a full-length buffer on dst_device, with
 * hipMemcpyPeerAsync on dst_stream (xGMI between devices; a plain device copy where source and destination coincide; nothing
 * is copied when d_windows[g] == d_dst).  The caller orders dst_stream after the producing streams (an event per part, or a
 * device synchronise); no collective and no host staging are involved. */
int bhw_gather_parts_device(const bhw_params *p, uint32_t n_parts, const int *src_devices, const int32_t *const *d_windows,
                            int dst_device, void *dst_stream, int32_t *d_dst);

/* Fused apply (the step after the path in every consumer -- the window multiplies the samples in
 * front of an FFT).  d_y[i] = (d_x[i] * w[n0+i]) >> shift with the exact 64-bit product (as int_multNxN_dsp48,
 * src/int_multNxN_dsp48.vhd:102), floor shift (0..62) and the low 32 bits stored; the coefficients are generated
 * on the fly and never written to HBM.  d_y must not overlap d_x. */
int bhw_apply_device(const bhw_params *p, int device, void *hip_stream, uint64_t n0, uint64_t count,
                     const int32_t *d_x, int32_t *d_y, uint32_t shift);

/* `frames` back-to-back periods of the coefficient stream (the streaming-frame workload:
 * ENABLE held for frames * 2^phi_width clocks).  One period is computed, then replicated by a
 * store-only kernel: d_out holds frames * 2^phi_width int32. */
int bhw_generate_batched_device(const bhw_params *p, int device, void *hip_stream,
                                uint32_t frames, int32_t *d_out);

/* Replaces cordic() alone: cpp/cordic_sincos.cpp:10 (model CPP), hls/cordic/cordic.cpp:45
 * (model HLS), the cordic_dds entity src/cordic_dds.vhd:77-92 (model VHDL), or taylor_sincos
 * src/taylor_sincos.vhd:64-80 (sin_type TAYLOR), cordic_dds48 src/cordic_dds48.vhd:98-112 (model DDS48) or
 * cordic_dds_scaled src/cordic_dds_scaled.vhd:81-96 (model SCALED).  Either output pointer may be NULL. */
int bhw_sincos_device(const bhw_params *p, int device, void *hip_stream,
                      uint64_t theta0, uint64_t count, int32_t *d_sin, int32_t *d_cos);

/* Convenience for host consumers (file writers, testbenches): runs bhw_generate_device into
 * library scratch on `device`, then copies the result to host memory.  Synchronous. */
int bhw_generate_to_host(const bhw_params *p, int device, uint64_t n0, uint64_t count, int32_t *h_out);
int bhw_sincos_to_host(const bhw_params *p, int device, uint64_t theta0, uint64_t count,
                       int32_t *h_sin, int32_t *h_cos);

/* Replaces the cordic_atan2 entity (src/cordic_atan2.vhd:64-76): vectoring CORDIC, one angle per (x, y) pair.
 * VEC_DX / VEC_DY are INPUT_WIDTH-bit two's-complement words carried in int32; PHI_DT is the ANGLE_WIDTH-bit output word,
 * sign-extended to int32 (full circle = 2^angle_width; quadrant fix-ups exactly as written at :126-128,:207-213).
 * The entity reads bits 0..ANGLE_WIDTH-2 of its inputs (:142-145), so input_width >= angle_width - 1 is required
 * (upstream's default generics 20/24 do not elaborate).  d_x, d_y, d_phi: `count` int32 each; d_phi may alias neither. */
typedef struct bhw_atan2_params {
    uint32_t struct_size;   /* sizeof(bhw_atan2_params)                                  */
    uint32_t precision;     /* 1..7              PRECISION                               */
    uint32_t input_width;   /* <= 32             INPUT_WIDTH                             */
    uint32_t angle_width;   /* 4..32             ANGLE_WIDTH                             */
} bhw_atan2_params;
int bhw_atan2_device(const bhw_atan2_params *p, int device, void *hip_stream, uint64_t count,
                     const int32_t *d_x, const int32_t *d_y, int32_t *d_phi);
int bhw_atan2_to_host(const bhw_atan2_params *p, int device, uint64_t count,
                      const int32_t *h_x, const int32_t *h_y, int32_t *h_phi);

/* Resident tables (win_selector elaborates its CORDIC from the generics; AA0..AA6 are run-time ports, src/win_selector.vhd:60-87).
 * The first-quadrant (c, s) table of BHW_ALGO_TABLE depends on the CORDIC generics only: model, phi_width, dat_width and, for
 * the VHDL model, precision.  A bhw_table is a caller-owned handle that holds one such table on one device, built once, with the
 * lifetime of a hipFFT plan; every call below then generates or applies any weights over any range from it without rebuilding it.
 *   - Create: any configuration bhw_generate_device_ex accepts with BHW_ALGO_TABLE.  sin_type other than BHW_SIN_CORDIC (the
 *     Taylor ROM is cached by the library already) and the models DDS48 / SCALED are BHW_ERR_UNSUPPORTED; table_format
 *     (BHW_TABLE_*, BEST = the narrowest exact format) limits the format as bhw_exec.table_format does.  All argument checks come
 *     before any HIP call.  Synchronous: settles the packed-format verdicts of the configuration (trial builds, the check word read
 *     back), then holds exactly one table in one allocation, in the layout the configuration's whole periods read -- split and
 *     packed where the tile kernel applies (phi_width >= 22 at z_shr = 0), plain and natural otherwise.  bhw_table_bytes is what
 *     bhw_workspace_bytes_ex gives for a whole-period BHW_ALGO_TABLE call with the same table_format once the formats are settled
 *     (16.5 MiB for a 2^26-point window at 32 bits, model HLS).
 *   - Calls from a table: `p` must match the table on model, phi_width, dat_width, precision (VHDL model only) and have sin_type
 *     BHW_SIN_CORDIC, else BHW_ERR_BADARG and bhw_last_error() names the field; aa, n_terms, win_type and combine are free per call
 *     and `p` is validated as usual.  Same results as bhw_generate_device / bhw_apply_device / bhw_generate_part_device of `p`.
 *     They allocate nothing, neither synchronise nor read anything back, and do not touch the library scratch of any stream: they
 *     can always be captured into a HIP graph, with no bhw_prepare_device.  They run on the table's device (the calling thread's
 *     current device is restored).  The table is immutable after create: any number of streams and host threads may read one table
 *     at the same time.
 *   - bhw_generate_part_from_table needs a table in the tile layout (phi_width >= 22), else BHW_ERR_UNSUPPORTED.
 *   - bhw_table_describe: one line -- the table's format, layout and bytes, and the kernels a from-table call of (p, n0, count) launches.
 *   - Destroy synchronises the table's device and frees the table; NULL is accepted.  The caller must not destroy a table that a
 *     captured graph may still replay (the graph holds its address).  bhw_release_device does not touch tables. */
typedef struct bhw_table_s *bhw_table;
int      bhw_table_create(const bhw_params *p, int device, void *hip_stream, uint32_t table_format, bhw_table *out);
int      bhw_table_destroy(bhw_table t);
uint64_t bhw_table_bytes(bhw_table t);
int      bhw_table_describe(bhw_table t, const bhw_params *p, uint64_t n0, uint64_t count, char *buf, uint64_t len);
int bhw_generate_from_table(bhw_table t, const bhw_params *p, void *hip_stream, uint64_t n0, uint64_t count, int32_t *d_out);
int bhw_apply_from_table(bhw_table t, const bhw_params *p, void *hip_stream, uint64_t n0, uint64_t count,
                         const int32_t *d_x, int32_t *d_y, uint32_t shift);
int bhw_generate_part_from_table(bhw_table t, const bhw_params *p, void *hip_stream, uint32_t part, uint32_t n_parts,
                                 int32_t *d_window);

/* Overlapped-frame apply (the STFT / Welch front end: the window multiplies overlapping frames of one signal in front of an FFT).
 * With N = 2^phi_width, C = channels and w[k] the coefficient bhw_generate_device(p, n0 = 0) gives at index k, for f < frames,
 * k < N, c < C:
 *     d_y[f * y_stride + k * C + c] = low32((int64 d_x[(f * hop + k) * C + c] * w[k]) >> shift)
 * the arithmetic of bhw_apply_device (exact 64-bit product, floor shift 0..62, low 32 bits stored).  Both channels of a time index
 * share one coefficient; hop >= 1 is free (below N: overlap, N: back to back, above N: gaps); y_stride counts int32 elements between
 * frame starts in d_y (0 = N * C; a larger stride lands the frames in a zero-padded FFT input, the elements between N * C and
 * y_stride are never written).  d_x holds ((frames - 1) * hop + N) * C int32; d_y must not overlap d_x.
 *   - All argument checks come before any HIP call: NULL pointers, struct_size, channels outside {1, 2}, hop 0, y_stride below N * C,
 *     shift > 62, reserved != 0, overlap of d_x and d_y, frames * N above 2^34, and (from a table) the key match of the table calls.
 *   - bhw_apply_frames_device accepts every configuration bhw_apply_device accepts.  Each coefficient is computed once per lane and
 *     applied to a group of frames (k_frames_direct: direct CORDIC, no table, no scratch -- capturable with no bhw_prepare_device).
 *     For one channel the planner may instead take the per-frame route, one bhw_apply_device call per frame: always for the Taylor
 *     sources, and for long windows with few frames, where one apply per frame costs less than the direct CORDIC of every
 *     coefficient (the crossover is measured).  The Taylor sources with channels = 2 are BHW_ERR_UNSUPPORTED.
 *   - bhw_apply_frames_from_table accepts what bhw_apply_from_table accepts and keeps its contract: no allocation, no
 *     synchronisation, always capturable; the coefficients are gathered from the resident table (k_frames_table).
 *   - bhw_apply_frames_describe: one line -- the route, the frame-group size and the kernel names.  t may be NULL (the library
 *     call).  Host arithmetic only. */
typedef struct bhw_frames {
    uint32_t struct_size;  /* sizeof(bhw_frames)                                     */
    uint32_t channels;     /* 1 (real) or 2 (interleaved I/Q)                        */
    uint64_t frames;       /* 0 = nothing to do                                      */
    uint64_t hop;          /* time indices between frame starts, >= 1                */
    uint64_t y_stride;     /* int32 elements between frames in d_y; 0 = N * channels  */
    uint32_t shift;        /* 0..62                                                  */
    uint32_t reserved;     /* must be 0                                              */
} bhw_frames;
int bhw_apply_frames_device(const bhw_params *p, int device, void *hip_stream, const bhw_frames *f, const int32_t *d_x, int32_t *d_y);
int bhw_apply_frames_from_table(bhw_table t, const bhw_params *p, void *hip_stream, const bhw_frames *f, const int32_t *d_x,
                                int32_t *d_y);
int bhw_apply_frames_describe(bhw_table t, const bhw_params *p, const bhw_frames *f, char *buf, uint64_t len);

/* Weighted overlap-add (the synthesis side of an STFT: the window multiplies every frame again and the overlapping frames are summed
 * back into one signal).  The transpose of bhw_apply_frames_device.  With N = 2^phi_width, C = channels and w[k] the coefficient
 * bhw_generate_device(p, n0 = 0) gives at index k, for every output time index t in [t0, t0 + count) and every c < C:
 *     S = sum over f < frames with f * hop <= t < f * hop + N of  int64 d_y[f * y_stride + (t - f * hop) * C + c] * int64 w[t - f * hop]
 *     d_x[(t - t0) * C + c] = low32(S >> shift)       (arithmetic shift 0..62; an empty sum is 0 and is written)
 * the arithmetic of bhw_apply_device summed before the shift.  The sum wraps mod 2^64, so the result is bit-exact whatever the
 * order of summation.  Only the first N * C elements of each frame row of d_y are read; y_stride counts int32 elements between
 * frame starts (0 = N * C; a larger stride reads the frames out of a zero-padded inverse-FFT output).  The signal's extent is
 * (frames - 1) * hop + N time indices; t0 / count pick an output range inside it.  A streaming caller calls once per block and passes
 * again the last ceil(N / hop) - 1 frames of the previous block: only the outputs every one of their frames reaches are complete.
 * With hop > N the gaps between frames come out as 0.  d_x holds count * C int32 and must not overlap the rows of d_y read.
 *   - All argument checks come before any HIP call: NULL pointers, struct_size, reserved != 0, channels outside {1, 2}, hop 0,
 *     shift > 62, y_stride below N * C, frames 0 with count > 0, t0 + count beyond the extent, frames * N or the extent above 2^34,
 *     overlap of d_x and d_y, and (from a table) the key match of the table calls.  count == 0 returns BHW_OK, pointers unchecked.
 *   - The Taylor sources (BHW_SIN_TAYLOR*) are BHW_ERR_UNSUPPORTED: they have no per-coefficient form to sum frames with.  Generate
 *     the window once (bhw_generate_device) and form the products and sums in the caller's framework instead.
 *   - bhw_overlap_add_device accepts every CORDIC configuration bhw_apply_device accepts.  Each coefficient is computed once per
 *     lane and applied to a block of Q consecutive hops (k_ola_direct: direct CORDIC); it allocates nothing and uses no scratch,
 *     so it can be captured with no bhw_prepare_device.
 *   - bhw_overlap_add_from_table keeps the contract of the from-table calls: no allocation, no synchronisation, always capturable,
 *     any number of concurrent readers; the coefficients are gathered from the resident table (k_ola_table).
 *   - bhw_overlap_add_describe: one line -- the route, Q, the lane layout, the grid and the kernel name.  t may be NULL (the library
 *     call).  Host arithmetic only. */
typedef struct bhw_ola {
    uint32_t struct_size;  /* sizeof(bhw_ola) = 56                                    */
    uint32_t channels;     /* 1 or 2 (interleaved I/Q, one coefficient per pair)       */
    uint64_t frames;
    uint64_t hop;          /* >= 1                                                     */
    uint64_t y_stride;     /* int32 elements between frame starts in d_y; 0 = N * C   */
    uint64_t t0;           /* first output time index                                  */
    uint64_t count;        /* output time indices; 0 = nothing to do                   */
    uint32_t shift;        /* 0..62                                                    */
    uint32_t reserved;     /* must be 0                                                */
} bhw_ola;
int bhw_overlap_add_device(const bhw_params *p, int device, void *hip_stream, const bhw_ola *o, const int32_t *d_y, int32_t *d_x);
int bhw_overlap_add_from_table(bhw_table t, const bhw_params *p, void *hip_stream, const bhw_ola *o, const int32_t *d_y,
                               int32_t *d_x);
int bhw_overlap_add_describe(bhw_table t, const bhw_params *p, const bhw_ola *o, char *buf, uint64_t len);

/* Windows of any length L, 1 <= L <= 2^phi_width: torch.hann_window(400), a 25 ms frame at 16 kHz, a symmetric filter-design window.
 * The phase accumulator counts modulo L instead of 2^phi_width, and each harmonic is read at the nearest phi_width-bit angle of the
 * exact one.  For a coefficient index n (any uint64) let m = n mod L; for every harmonic k = 1 .. n_terms - 1
 *     theta_k(n) = round(((k * m) mod L) * 2^phi_width / L)  mod 2^phi_width
 * and the coefficient is the model's CORDIC at theta_k(n) combined with aa[] under the configured rule -- exactly what the
 * power-of-two window does with theta_k = (k * n) mod 2^phi_width.
 *   - L = 2^phi_width reproduces the power-of-two windows bit for bit (theta_k = (k * n) mod 2^phi_width, no rounding), and the calls
 *     below then take the existing entry point of their kind unchanged: same kernels, same contracts.
 *   - No rounding ties occur: with L = 2^a * b (b odd) a tie would need 2^(phi_width + 1 - a) * m = b (mod 2b), even against odd.  So
 *     half up and half to even agree, and theta_k(L - m) = -theta_k(m) (mod 2^phi_width).
 *   - The index stream is periodic in L, as the hardware counter is in 2^phi_width.  A symmetric window of length L is
 *     bhw_generate_len_device(length = L - 1, n0 = 0, count = L).
 *   - The rounding of the angle adds up to pi * 2^-phi_width rad of phase error per harmonic: choose phi_width above log2 L by enough
 *     bits for the chosen dat_width (as a rule, phi_width >= dat_width).  The integer window is not promised to be mirror-symmetric
 *     (the power-of-two windows are not either).
 * Each call is its power-of-two counterpart with N replaced by L: the same formulas, limits and contracts (d_x extent
 * (frames - 1) * hop + L, y_stride >= L * C, frames * L <= 2^34, the overlap-add extent (frames - 1) * hop + L, count <= 2^34).
 *   - Argument checks come before any HIP call: those of the counterpart, and length 0 or above 2^phi_width (BHW_ERR_BADARG), a
 *     sin_type other than BHW_SIN_CORDIC (BHW_ERR_UNSUPPORTED; the models DDS48 / SCALED are refused as for every window).
 *   - At L != 2^phi_width the library calls run one lane per coefficient with the direct CORDIC chains (the frames and overlap-add
 *     kernels spread each coefficient over frames or hops as their counterparts do); they allocate nothing and use no scratch, so they
 *     can be captured with no bhw_prepare_device.  The whole-period kernels (fused, tile) need L = 2^phi_width and are not used.
 *   - The from-table calls gather from the resident table (it holds every first-quadrant angle, so it serves any length) in any table
 *     format and layout, and keep the from-table contract: no allocation, no synchronisation, always capturable, any number of
 *     concurrent readers, the same key match.
 *   - bhw_describe_len: one line naming the route ("power-of-two route" with the counterpart's describe text, or "any-length route"),
 *     the kernel and its grid.  f non-NULL: the frames call; o non-NULL: the overlap-add call; both NULL: the generate call of
 *     [n0, n0 + count) (n0, count are ignored otherwise).  t may be NULL (the library call).  Host arithmetic only. */
int bhw_generate_len_device(const bhw_params *p, uint64_t length, int device, void *hip_stream,
                            uint64_t n0, uint64_t count, int32_t *d_out);
int bhw_generate_len_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream,
                                uint64_t n0, uint64_t count, int32_t *d_out);
int bhw_apply_frames_len_device(const bhw_params *p, uint64_t length, int device, void *hip_stream,
                                const bhw_frames *f, const int32_t *d_x, int32_t *d_y);
int bhw_apply_frames_len_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream,
                                    const bhw_frames *f, const int32_t *d_x, int32_t *d_y);
int bhw_overlap_add_len_device(const bhw_params *p, uint64_t length, int device, void *hip_stream,
                               const bhw_ola *o, const int32_t *d_y, int32_t *d_x);
int bhw_overlap_add_len_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream,
                                   const bhw_ola *o, const int32_t *d_y, int32_t *d_x);
int bhw_describe_len(bhw_table t, const bhw_params *p, uint64_t length, uint64_t n0, uint64_t count,
                     const bhw_frames *f, const bhw_ola *o, char *buf, uint64_t len);

/* Float32 frame apply and overlap-add: the STFT front and back ends with the float samples an FFT reads and writes.  Let w[k] be the
 * int32 coefficient the matching int32 call uses at index k -- bhw_generate_device(p, n0 = 0) for length = 2^phi_width, the phase
 * map of the *_len calls otherwise -- and `shift` the descriptor's field (0..62).  The float coefficient is
 *     v[k] = fl32(w[k]) * 2^-shift
 * fl32: conversion to binary32, round to nearest even (exact for |w| < 2^24).  The scaling is exact: |w| >= 1 gives |v| >= 2^-62,
 * a normal number.  N below is the window length `length` (1..2^phi_width; 2^phi_width is the power-of-two window).
 *   - bhw_apply_frames_f32_*: the indexing of bhw_apply_frames_device, one IEEE binary32 multiply rounded to nearest even, subnormals
 *     kept, inf and NaN as IEEE arithmetic has them:
 *         d_y[f * y_stride + k * C + c] = fl32(d_x[(f * hop + k) * C + c] * v[k])
 *   - bhw_overlap_add_f32_*: the indexing and extent of bhw_overlap_add_device.  For each output t in [t0, t0 + count) and c < C
 *         S = sum over the frames f reaching t, in ASCENDING f, of  (double) d_y[f * y_stride + (t - f * hop) * C + c] * (double) v[t - f * hop]
 *     accumulated in binary64 from +0.0.  Each product is exact in binary64 (24 x 24 significand bits), so a fused multiply-add and a
 *     separate multiply and add give the same S.  The summation order is part of the contract: floating-point addition does not
 *     associate (the int64 sums of the int32 call were exact in any order).
 *       flags 0:                  d_x[(t - t0) * C + c] = fl32(S)                (binary64 -> binary32, nearest even; empty sum: +0.0)
 *       flags BHW_OLA_NORMALIZE:  E = sum over the same frames, in the same order, of (double) v[t - f * hop]^2, and
 *                                 d_x[(t - t0) * C + c] = E > 0 ? fl32(S / E) : +0.0    (S / E a correctly rounded binary64 division)
 *     The normalised form is what torch.istft computes, save that torch.istft raises where the envelope E is tiny and a kernel
 *     cannot: the outputs at the edges of the extent, covered only by small edge coefficients of the window, come out amplified.
 *     The caller picks t0 / count to leave them out (the first and last N - hop outputs for a window whose envelope is flat inside).
 *   - y_stride, the extents and every limit count float32 elements exactly as the int32 calls count int32 ones.
 *   - Argument checks come before any HIP call: everything the int32 counterpart checks, flags outside {0, BHW_OLA_NORMALIZE}
 *     (BHW_ERR_BADARG), length 0 or above 2^phi_width (BHW_ERR_BADARG), the Taylor sources (BHW_ERR_UNSUPPORTED: no per-lane
 *     coefficient).  The structs are those of the int32 calls; reserved must be 0.
 *   - The library forms compute the coefficients with the direct CORDIC chains: no allocation, no scratch, capturable with no
 *     bhw_prepare_device.  The from-table forms keep the from-table contract: no allocation, no synchronisation, always capturable,
 *     the same key match.  There is no per-frame route (no float fused apply exists; bhw_apply_device stays int32).
 *   - bhw_describe_f32: one line naming the route, the plan (G, or Q and the lane layout), the kernel and whether the overlap-add
 *     normalises.  Exactly one of f (frames call; flags must be 0) and o (overlap-add call).  t may be NULL (the library call).
 *     Host arithmetic only. */
#define BHW_OLA_NORMALIZE 1u
int bhw_apply_frames_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream,
                                const bhw_frames *f, const float *d_x, float *d_y);
int bhw_apply_frames_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream,
                                    const bhw_frames *f, const float *d_x, float *d_y);
int bhw_overlap_add_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream,
                               const bhw_ola *o, uint32_t flags, const float *d_y, float *d_x);
int bhw_overlap_add_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream,
                                   const bhw_ola *o, uint32_t flags, const float *d_y, float *d_x);
int bhw_describe_f32(bhw_table t, const bhw_params *p, uint64_t length, const bhw_frames *f, const bhw_ola *o, uint32_t flags,
                     char *buf, uint64_t len);

/* Batched, centred STFT framing and overlap-add: the framing of torch.stft / torch.istft (center, pad_mode, win_length < n_fft) for
 * B signals in one launch per side.  One descriptor serves both directions.  L is the window length `length` (1..2^phi_width), v[k]
 * the float coefficient of the *_f32 calls above, C = channels (2: interleaved pairs, complex64; both share a coefficient).
 *   - bhw_stft_frames_f32_*: for b < batch, f < frames, j < n_fft, c < C, with t = f * hop + j - pad (signed),
 *         d_y[b * y_batch_stride + f * y_stride + j * C + c] = col0 <= j < col0 + L ? fl32(X_b(t, c) * v[j - col0]) : +0.0
 *         X_b(t, c) = d_x[b * x_stride + t' * C + c],  t' = t for 0 <= t < samples;
 *                     BHW_PAD_REFLECT: t' = -t (t < 0), 2 * (samples - 1) - t (t >= samples);  BHW_PAD_CONSTANT: X = +0.0 outside
 *     This is F.pad(x, [pad, pad], pad_mode).unfold(-1, n_fft, hop) * window_padded, what torch.stft forms before its FFT, bit for
 *     bit inside the window columns (IEEE special values included).  The one difference: outside the window torch gets x * 0.0
 *     (-0.0 or NaN for some x), these calls write +0.0.  Every element of [0, n_fft * C) of each row is written; the elements
 *     between n_fft * C and y_stride, and the gaps of y_batch_stride, never are.
 *   - bhw_istft_ola_f32_*: for b < batch, t < samples, c < C, with u = t + pad, over the frames f with 0 <= k = u - f * hop - col0
 *     < L in ASCENDING f, in binary64 from +0.0:
 *         S = sum (double) d_y[b * y_batch_stride + f * y_stride + (u - f * hop) * C + c] * (double) v[k],   E = sum (double) v[k]^2
 *         d_x[b * x_stride + t * C + c] = flags ? (E > 0 ? fl32(S / E) : +0.0) : fl32(S)
 *     bhw_overlap_add_f32_* per signal, with t0 = pad - col0 and count = samples, save that samples may reach past the frames'
 *     extent (outputs no frame reaches are +0.0, as torch.istft zero-pads a long `length`).  pad_mode must be 0.
 *   - Argument checks, all before any HIP call (BHW_ERR_BADARG unless noted): those of the *_f32 calls on (p, length, flags), the
 *     frames call taking flags 0 only; NULL descriptor or pointers, struct_size, channels outside {1, 2}, batch 0, hop 0, n_fft 0 or
 *     above 2^31, shift > 62, col0 + L > n_fft, pad above 2^40, an unknown pad_mode (frames) or a nonzero one (overlap-add);
 *     frames: a frame outside the padded signal ((frames - 1) * hop + n_fft > samples + 2 * pad), samples 0 with frames > 0,
 *     BHW_PAD_REFLECT with pad > samples - 1; overlap-add: frames 0 with samples > 0, pad < col0 (the first outputs would have no
 *     window under them; torch.istft raises there too); strides that make signals or rows overlap (x_stride below samples * C,
 *     y_stride below n_fft * C, y_batch_stride below (frames - 1) * y_stride + n_fft * C), batch * frames * n_fft above 2^34,
 *     d_x and d_y overlapping, the Taylor sources (BHW_ERR_UNSUPPORTED), and (from a table) the key match of the from-table calls.
 *     frames 0 (frames call) or samples 0 (overlap-add) return BHW_OK with the pointers unchecked.
 *   - The library forms compute the coefficients by direct CORDIC: no allocation, no scratch, capturable with no
 *     bhw_prepare_device.  The from-table forms keep the from-table contract: no allocation, no synchronisation, always capturable.
 *   - bhw_describe_stft: one line naming the route, the plan and the kernel of the frames call (inverse 0) or of the overlap-add
 *     (inverse 1, flags 0 or BHW_OLA_NORMALIZE).  t may be NULL (the library call).  Host arithmetic only. */
#define BHW_PAD_CONSTANT 0u
#define BHW_PAD_REFLECT 1u
typedef struct bhw_stft {
    uint32_t struct_size;     /* sizeof(bhw_stft) = 96                                              */
    uint32_t channels;        /* 1 (float32) or 2 (interleaved pairs: complex64)                    */
    uint64_t batch;           /* B >= 1 signals                                                      */
    uint64_t samples;         /* T: time indices per signal (read by the frames, written by the OLA) */
    uint64_t x_stride;        /* float elements between signal starts; 0 = T * C                     */
    uint64_t frames;          /* frames per signal                                                   */
    uint64_t hop;             /* >= 1                                                                */
    uint64_t n_fft;           /* columns of a frame row                                              */
    uint64_t col0;            /* first window column; torch: (n_fft - L) / 2                         */
    uint64_t pad;             /* padding in front of the signal: center n_fft / 2, else 0            */
    uint64_t y_stride;        /* float elements between rows; 0 = n_fft * C                          */
    uint64_t y_batch_stride;  /* float elements between the first rows of two signals; 0 = frames * y_stride */
    uint32_t pad_mode;        /* frames: BHW_PAD_CONSTANT or BHW_PAD_REFLECT; overlap-add: 0          */
    uint32_t shift;           /* 0..62                                                               */
} bhw_stft;
int bhw_stft_frames_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s,
                               const float *d_x, float *d_y);
int bhw_stft_frames_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s,
                                   const float *d_x, float *d_y);
int bhw_istft_ola_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                             const float *d_y, float *d_x);
int bhw_istft_ola_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s,
                                 uint32_t flags, const float *d_y, float *d_x);
int bhw_describe_stft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, int inverse, uint32_t flags, char *buf,
                      uint64_t len);

/* Welch's method around the FFT (scipy.signal.welch's defaults as the model): the window sums every spectrum scaling needs, the
 * detrended windowed segments in front of the FFT, and the averaged periodogram behind it.  The FFT itself is the caller's (hipFFT,
 * torch.fft).  L is the window length `length` (1..2^phi_width), w[k] the int32 coefficient of the length-L phase map (the *_len
 * calls; the power-of-two window at L = 2^phi_width) and v[k] = fl32(w[k]) * 2^-shift the float coefficient of the *_f32 calls.
 *
 * 1. Window sums.  Exact integer sums of the window, computed on the device without storing it:
 *        s1 = sum over k < L of u[k]   (int64),        s2 = sum over k < L of u[k]^2   (below 2^92)
 *    with u[k] = w[k], or under BHW_SUMS_F32 u[k] = (int64) fl32(w[k]), the integer the float calls multiply by (it differs from
 *    w[k] only for |w[k]| >= 2^24; |u| <= 2^31 either way).  d_sums receives four 64-bit words:
 *        d_sums[0] = s1 (two's complement)          d_sums[1] = sum of the low 32 bits of u[k]^2
 *        d_sums[2] = sum of u[k]^2 >> 32            d_sums[3] = L (the number of coefficients summed)
 *    so that s2 = d_sums[1] + d_sums[2] * 2^32, joined by the host in 128 bits (L <= 2^30 keeps each word below 2^62 and |s1| <= 2^61).
 *    The sums are integers: the result does not depend on the order of the reduction, which uses 64-bit integer atomics.
 *    The caller zeroes nothing: the call first clears the four words with a memset on the stream (a memset node under capture), then
 *    launches the reduction -- asynchronous, no synchronisation, capturable.  The library form computes the coefficients by the direct
 *    CORDIC chains (no scratch, no bhw_prepare_device); the from-table form gathers them and keeps the from-table contract.
 *    Checks before any HIP call: those of the *_len calls on (p, length) (the Taylor sources: BHW_ERR_UNSUPPORTED), flags outside
 *    {0, BHW_SUMS_F32}, d_sums NULL or not 8-byte aligned (BHW_ERR_BADARG), and (from a table) the key match.
 *
 * 2. Welch segments.  scipy.signal.welch cuts frames = (T - noverlap) / (L - noverlap) segments at hop = L - noverlap with no padding,
 *    detrends each, multiplies by the window and zero-pads at the END to n_fft.  The descriptor is bhw_stft with pad 0, col0 0,
 *    pad_mode 0 and n_fft >= L (batch, strides, one or two channels as there), plus a flags word:
 *    A segment reads its L window columns only, so the extent rule is (frames - 1) * hop + L <= samples (scipy's segment count), not
 *    the n_fft one of bhw_stft_frames_f32_*: the columns L..n_fft of a row are written, never read.
 *      flags 0:  exactly bhw_stft_frames_f32_* of the same descriptor (the same kernel).  No workspace is needed or read.
 *      BHW_WELCH_DETREND_CONSTANT:  for each row (b, f) and channel c, with x_j = X_b(f * hop + j, c) for j < L:
 *            S = sum over j < L of (double) x_j, in the FIXED order below, binary64 from +0.0
 *            m = fl32(S / (double) L)                                   (a correctly rounded binary64 division, then one rounding)
 *            d_y[b * y_batch_stride + f * y_stride + j * C + c] = j < L ? fl32(fl32(x_j - m) * v[j]) : +0.0      (no fused operation)
 *        Binary64 addition of float32 values is not exact, so the ORDER of S is part of the contract.  It is a function of L alone --
 *        not of the plan, the batch, the lane layout, or library versus table:
 *            P[i] = sum of x_j over j = i, i + 64, i + 128, ... < L, in ascending j, binary64 from +0.0         (i = 0..63)
 *            for s = 32, 16, 8, 4, 2, 1:  P[i] = P[i] + P[i + s]  for every i < s (all i of a step read before any is written)
 *            S = P[0]
 *        IEEE special values propagate: a NaN or an infinity in a segment poisons that row (and channel) and no other.
 *        The means go through a caller workspace of bhw_welch_workspace_bytes bytes (batch * frames * C floats, row (b, f) at
 *        (b * frames + f) * C + c): a first launch computes them, one wave per row, a second one is the stft frames loop with one more
 *        load and a subtraction per row.  No call allocates.
 *    Checks before any HIP call (BHW_ERR_BADARG unless noted): those of bhw_stft_frames_f32_* (with the extent rule above), plus pad != 0,
 *    col0 != 0, pad_mode != 0,
 *    flags outside {0, BHW_WELCH_DETREND_CONSTANT}, and with detrending and frames > 0 a NULL, misaligned (4 bytes) or short workspace
 *    (short: BHW_ERR_WORKSPACE) or one that overlaps d_x or d_y.
 *
 * 3. Averaged periodogram.  d_Y: complex64 (B, F, K) as interleaved float pairs, 8-byte aligned, row (b, f) at
 *    (b * y_batch_stride + f * y_stride) complex elements, bins contiguous; d_P: float32, row b at b * p_stride floats.
 *        q_f   = (double) re * (double) re + (double) im * (double) im      (both squares are exact in binary64: one rounding, and a
 *                                                                            fused multiply-add gives the same value)
 *        A_blk = sum of q_f over the frames of one block, in ascending f, binary64 from +0.0
 *        A     = sum of A_blk over the blocks, in ascending order, binary64 from +0.0
 *        d_P[b * p_stride + k] = fl32(A * s_k),    s_k = scale * (doubled(k) ? 2 : 1)          (binary64 products, one final rounding)
 *    A block is BHW_WELCH_BLOCK consecutive frames (the last one shorter), so every F <= BHW_WELCH_BLOCK is one plain ascending sum.
 *    Under BHW_PSD_ONESIDED doubled(k) is true for every k except 0 and, for even n_fft, K - 1 (scipy's rule); otherwise never.
 *    With more than one block the block sums go through a caller workspace of bhw_welch_psd_workspace_bytes bytes
 *    (B * ceil(F / BLOCK) * K doubles; 0 for one block) and a second launch adds them in block order: no float atomics.  Only the
 *    K floats of each output row are written.  Y is read exactly once, with nontemporal loads.
 *    Checks before any HIP call (BHW_ERR_BADARG unless noted): NULL descriptor or pointers, struct_size, reserved != 0, unknown flags,
 *    batch, frames or bins 0, n_fft 0, bins above n_fft, BHW_PSD_ONESIDED with bins != n_fft / 2 + 1, a scale that is not finite,
 *    strides that make rows overlap (y_stride < K, y_batch_stride < (F - 1) * y_stride + K, p_stride < K), B * F * K above 2^34,
 *    B * ceil(F / BLOCK) * ceil(K / 64) above 2^31 - 1, d_Y not 8-byte aligned, d_P overlapping d_Y, a missing or misaligned
 *    workspace when one is needed, a short one (BHW_ERR_WORKSPACE).
 *
 *  - bhw_describe_welch: one line naming the route, the plan and the kernels.  s non-NULL: the segments call (flags: its flags);
 *    d non-NULL: the periodogram (p, length may then be NULL / 0); both NULL: the window sums (flags: BHW_SUMS_F32 or 0).  t may be NULL
 *    (the library call).  Host arithmetic only. */
#define BHW_SUMS_F32 1u
#define BHW_WELCH_DETREND_CONSTANT 1u
#define BHW_PSD_ONESIDED 1u
#define BHW_WELCH_BLOCK 256u
typedef struct bhw_psd {
    uint32_t struct_size;     /* sizeof(bhw_psd) = 72                                            */
    uint32_t flags;           /* 0 or BHW_PSD_ONESIDED                                            */
    uint64_t batch;           /* B >= 1                                                           */
    uint64_t frames;          /* F >= 1: the rows averaged                                        */
    uint64_t bins;            /* K >= 1: n_fft / 2 + 1 (rfft) or n_fft (fft)                      */
    uint64_t n_fft;           /* for doubled(k)                                                   */
    uint64_t y_stride;        /* complex elements between frames; 0 = K                           */
    uint64_t y_batch_stride;  /* complex elements between signals; 0 = frames * y_stride          */
    uint64_t p_stride;        /* float elements between output rows; 0 = K                        */
    double   scale;           /* density: 1 / (fs * sum v^2 * F); spectrum: 1 / ((sum v)^2 * F)   */
} bhw_psd;
int bhw_window_sums_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, uint32_t flags, uint64_t *d_sums);
int bhw_window_sums_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, uint32_t flags, uint64_t *d_sums);
uint64_t bhw_welch_workspace_bytes(const bhw_stft *s, uint32_t flags);
int bhw_welch_frames_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                const float *d_x, float *d_y, void *workspace, uint64_t workspace_bytes);
int bhw_welch_frames_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s,
                                    uint32_t flags, const float *d_x, float *d_y, void *workspace, uint64_t workspace_bytes);
uint64_t bhw_welch_psd_workspace_bytes(const bhw_psd *d);
int bhw_welch_psd_f32(int device, void *hip_stream, const bhw_psd *d, const float *d_Y, float *d_P, void *workspace,
                      uint64_t workspace_bytes);
int bhw_describe_welch(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_psd *d,
                       char *buf, uint64_t len);

/* Welch cross spectra (scipy.signal.csd / coherence as the model): the pass behind the FFT for TWO signals.  d_X, d_Y: complex64
 * (B, F, K) as interleaved float pairs, 8-byte aligned, the FFTs of the segments of x and of y (bhw_welch_frames_f32_* of each);
 * same B, F, K, each with its own frame and batch strides in complex elements (0 = packed).  X and Y are each read exactly once, with
 * nontemporal loads, and every requested output comes from the same four binary64 sums.  Per signal b and bin k, over the frames f,
 * with (xr, xi) = X[b, f, k] and (yr, yi) = Y[b, f, k] converted to binary64:
 *        xx_f = xr * xr + xi * xi          yy_f = yr * yr + yi * yi                (the q_f of the periodogram, for X and for Y)
 *        re_f = xr * yr + xi * yi          im_f = xr * yi - xi * yr                (conj(X) * Y: scipy's convention)
 *    Every product of two float32 values is exact in binary64, so each of the four is ONE rounding, and a fused multiply-add gives
 *    the same value.  Each of the four is summed exactly as the periodogram sums q_f: ascending f inside blocks of BHW_WELCH_BLOCK
 *    frames from +0.0, then the block sums in ascending block order from +0.0.  Call the sums S_xx, S_yy, C_re, C_im, and let
 *    s_k = scale * (doubled(k) ? 2 : 1) with the periodogram's doubled(k) under BHW_CSD_ONESIDED.  rn() is one binary64 rounding:
 *        BHW_CSD_PXY         d_Pxy, complex64 (B, K):  (fl32(C_re * s_k), fl32(C_im * s_k))
 *        BHW_CSD_PXX / PYY   d_Pxx / d_Pyy, float32 (B, K):  fl32(S_xx * s_k) / fl32(S_yy * s_k) -- bit for bit what bhw_welch_psd_f32
 *                            gives for X (for Y) with the same descriptor fields
 *        BHW_CSD_COHERENCE   d_Cxy, float32 (B, K):  n = rn(C_re * C_re), m = rn(C_im * C_im), num = rn(n + m), den = rn(S_xx * S_yy),
 *                            fl32(rn(num / den)): a correctly rounded division and NO fused operation (n + m is never contracted into
 *                            a multiply-add); the scale cancels and is not applied
 *        BHW_CSD_H1          d_H1, complex64 (B, K):  (fl32(rn(C_re / S_xx)), fl32(rn(C_im / S_xx))): the H1 estimate P_xy / P_xx
 *    IEEE throughout, no special cases: an all-zero bin gives the coherence 0 / 0 = NaN (as scipy does), a NaN or an infinity in a frame
 *    poisons that (signal, bin) and no other.  For finite float32 spectra den neither overflows nor underflows to zero (every q_f is
 *    below 2^257, a sum of at most 2^34 of them below 2^291, the product below 2^582; a non-zero sum is at least 2^-298), so a NaN
 *    coherence means a zero or a non-finite bin.
 *    Any non-empty subset of the five outputs may be asked for in one call; a pointer whose flag is not set is neither read nor written.
 *    Output row b is at b * o_stride elements of the output's own type (one stride for all outputs); only the K elements of a row are
 *    written.  BHW_CSD_BROADCAST_X: X holds ONE signal (F, K), paired with each of Y's B signals (one excitation, many responses); the
 *    X side of every output is then the same in every row and is still written per row.  X is only read.
 *    With more than one block the block sums go through a caller workspace of bhw_welch_csd_workspace_bytes bytes
 *    (B * ceil(F / BLOCK) * K * chains doubles, chains = 2 when BHW_CSD_PXY is the only output and 4 otherwise; 0 for one block) and a
 *    second launch adds them in block order: no float atomics.  The call allocates nothing, neither synchronises nor reads back, and can
 *    be captured.
 *    Checks before any HIP call (BHW_ERR_BADARG unless noted): for X and for Y everything bhw_welch_psd_f32 checks for its operand
 *    (descriptor, struct_size, reserved, sizes, BHW_CSD_ONESIDED with bins != n_fft / 2 + 1, scale, strides that make rows overlap,
 *    B * F * K above 2^34, the workgroup bound, alignment), plus: unknown flags, an empty output mask, a NULL or misaligned pointer of
 *    a requested output (8 bytes for the complex ones, 4 for the others), o_stride < K, an output that overlaps an input, another
 *    requested output or the workspace, x_batch_stride != 0 under BHW_CSD_BROADCAST_X, a missing or misaligned workspace when one is
 *    needed, a short one (BHW_ERR_WORKSPACE).
 *  - bhw_describe_csd: one line naming the form, the plan and the kernels.  Host arithmetic only. */
#define BHW_CSD_ONESIDED 1u
#define BHW_CSD_BROADCAST_X 2u
#define BHW_CSD_PXY 0x10u
#define BHW_CSD_PXX 0x20u
#define BHW_CSD_PYY 0x40u
#define BHW_CSD_COHERENCE 0x80u
#define BHW_CSD_H1 0x100u
typedef struct bhw_csd {
    uint32_t struct_size;     /* sizeof(bhw_csd) = 96                                             */
    uint32_t flags;           /* BHW_CSD_ONESIDED, BHW_CSD_BROADCAST_X, and the output mask       */
    uint64_t batch;           /* B >= 1: the signals of Y (and of X without BHW_CSD_BROADCAST_X)  */
    uint64_t frames;          /* F >= 1: the rows averaged                                        */
    uint64_t bins;            /* K >= 1: n_fft / 2 + 1 (rfft) or n_fft (fft)                      */
    uint64_t n_fft;           /* for doubled(k)                                                   */
    uint64_t x_stride;        /* complex elements between frames of X; 0 = K                      */
    uint64_t x_batch_stride;  /* between signals of X; 0 = frames * x_stride (broadcast: must be 0) */
    uint64_t y_stride;        /* complex elements between frames of Y; 0 = K                      */
    uint64_t y_batch_stride;  /* between signals of Y; 0 = frames * y_stride                      */
    uint64_t o_stride;        /* elements between the rows of every output; 0 = K                 */
    double   scale;           /* as bhw_psd.scale                                                 */
    uint64_t reserved;        /* 0                                                                */
} bhw_csd;
uint64_t bhw_welch_csd_workspace_bytes(const bhw_csd *d);
int bhw_welch_csd_f32(int device, void *hip_stream, const bhw_csd *d, const float *d_X, const float *d_Y, float *d_Pxy, float *d_Pxx,
                      float *d_Pyy, float *d_Cxy, float *d_H1, void *workspace, uint64_t workspace_bytes);
int bhw_describe_csd(const bhw_csd *d, char *buf, uint64_t len);

/* Fused window and real FFT: the rows of bhw_stft_frames_f32_* (flags 0) or of bhw_welch_frames_f32_* (BHW_WELCH_DETREND_CONSTANT)
 * formed, transformed and written as their one-sided spectrum by ONE launch.  A workgroup owns whole rows: it reads the samples of a
 * row once, removes the mean (with the flag), applies the window, runs a float32 FFT of n_fft points in LDS and writes only the
 * K = n_fft / 2 + 1 bins.  Neither the windowed rows nor the means ever reach memory, so the call takes no workspace.
 *   - The row.  The n_fft values the transform sees are bit for bit the row (b, f) those calls would have written for the same
 *     descriptor: flags 0: col0 <= j < col0 + L ? fl32(X_b(t, 0) * v[j - col0]) : +0.0 with the padding of bhw_stft_frames_f32_*;
 *     BHW_WELCH_DETREND_CONSTANT: j < L ? fl32(fl32(x_j - m) * v[j]) : +0.0 with m = fl32(S / L) and S summed in the FIXED order of
 *     bhw_welch_frames_f32_* (64 binary64 partial sums by j mod 64 in ascending j, then the butterfly 32 ... 1), no fused operation.
 *     A row reads its L window columns only, so the extent rule is the Welch one, (frames - 1) * hop + L <= samples, whenever pad,
 *     col0 and pad_mode are all 0, and that of bhw_stft_frames_f32_* otherwise.
 *   - The transform.  d_Y[b * y_batch_stride + f * y_stride + 2 * k + {0, 1}] = (re, im) of sum over j of row[j] * exp(-2 pi i j k / n_fft)
 *     for k < K: the sign convention of torch.fft.rfft, no scaling; complex64 as interleaved float pairs.  The FFT is NOT pinned bit
 *     for bit: it is a float32 Stockham transform of n_fft / 2 complex points (the row taken as pairs) in radix-4 passes, one radix-2
 *     pass at the end when log2(n_fft / 2) is odd, and a split pass; every twiddle factor is the float32 rounding of a binary64
 *     cosine or sine.  Its error against an exact transform of the float32 row is that of a float32 FFT (relative l2 error of a row
 *     of the order of 2^-24 * log2(n_fft) at most); the tests hold it to twice the error of rocFFT on the same rows.
 *   - Supported: channels 1 and n_fft a power of two in 16..4096.  Everything else -- complex input, other lengths -- is
 *     BHW_ERR_UNSUPPORTED.  The inverse is bhw_istft_fft_f32_* below.  Complex input has calls of its own: bhw_stft_cfft_f32_*; so
 *     has an even n_fft = 2^a 3^b 5^c that is no power of two (400, 480, 960, 1000, ...): bhw_stft_mfft_f32_*.
 *   - Descriptor: bhw_stft, where for these calls y_stride and y_batch_stride count FLOAT elements between spectrum rows and between
 *     signals; 0 means 2 * K and frames * y_stride.  Both must be even (rows of complex64 stay 8-byte aligned).  flags: 0 or
 *     BHW_WELCH_DETREND_CONSTANT; with the flag pad, col0 and pad_mode must be 0, as for the segments call.
 *   - Determinism: the bits of spectrum row (b, f) depend only on the window, n_fft, flags and that row's samples -- not on the
 *     batch, the plan, the row's place in a workgroup, the strides, or library versus table.
 *   - Purely real bins: the imaginary parts of bin 0 and of bin n_fft / 2 are written as +0.0.
 *   - IEEE: a NaN or an infinity in x reaches only the rows whose window covers it; every other row keeps its bits.
 *   - Only the 2 * K floats of each row are written: the elements between 2 * K and y_stride and the gaps of y_batch_stride never are.
 *   - Checks before any HIP call (BHW_ERR_BADARG unless noted): everything the frames call (flags 0) or the segments call (with the
 *     flag) checks for the descriptor with packed output strides, unknown flags, the unsupported n_fft or channels
 *     (BHW_ERR_UNSUPPORTED), y_stride below 2 * K or odd, y_batch_stride below (frames - 1) * y_stride + 2 * K or odd,
 *     batch * frames * K above 2^34, NULL pointers, d_Y not 8-byte aligned, d_x not 4-byte aligned, d_Y overlapping d_x, and (from a
 *     table) the key match.  frames 0 returns BHW_OK with the pointers unchecked.
 *   - The library form computes the coefficients by direct CORDIC and the twiddle factors in the kernel: no allocation, no scratch,
 *     capturable with no bhw_prepare_device.  The from-table form keeps the from-table contract: no allocation, no synchronisation,
 *     capturable on its first call.
 *   - bhw_describe_stft_fft: one line naming the route, the plan (lanes per row, rows side by side in a workgroup, radix schedule,
 *     LDS bytes, grid) and the kernel.  t may be NULL (the library call).  Host arithmetic only. */
int bhw_stft_fft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                            const float *d_x, float *d_Y);
int bhw_stft_fft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                const float *d_x, float *d_Y);
int bhw_describe_stft_fft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len);

/* Fused inverse real FFT, window and overlap-add: torch.fft.irfft in front of bhw_istft_ola_f32_*, by ONE launch.  A group of lanes
 * owns a span of a signal's time axis, reads the K = n_fft / 2 + 1 bins of every frame that reaches it, transforms them in LDS, and
 * adds the windowed row into binary64 accumulators that it stores once.  The time rows never reach memory, so the call takes no
 * workspace.
 *   - The row.  For b < batch, f < frames, r[j], j < n_fft, is the float32 inverse real transform of the bins
 *     Y[k] = d_Y[b * y_batch_stride + f * y_stride + 2 * k + {0, 1}]: r[j] ~ (1 / n_fft) * sum over k' < n_fft of Y[k'] exp(+2 pi i j k' /
 *     n_fft) over the Hermitian extension Y[n_fft - k] = conj Y[k]: the convention and the scaling of torch.fft.irfft(Y, n=n_fft).  The
 *     1 / n_fft is one exact power-of-two scaling of the float32 result.  The imaginary parts of bins 0 and n_fft / 2 never enter the
 *     arithmetic.  The transform is NOT pinned bit for bit: it mirrors the forward's structure, a pre-split pass and an inverse float32
 *     Stockham transform of n_fft / 2 complex points in radix-4 passes with one radix-2 pass at the end when log2(n_fft / 2) is odd;
 *     every twiddle factor is the float32 rounding of a binary64 cosine or sine.  The bits of a row depend on its K bins and n_fft
 *     only -- not on its place in a workgroup, the span that reads it, the grid, the strides or the route.
 *   - The sum.  Given those rows every output is exactly what bhw_istft_ola_f32_* defines on them: for t < samples, u = t + pad, over
 *     the frames f with 0 <= k = u - f * hop - col0 < L in ASCENDING f, in binary64 from +0.0:
 *         S = sum (double) r_f[u - f * hop] * (double) v[k],   E = sum (double) v[k]^2
 *         d_x[b * x_stride + t] = flags ? (E > 0 ? fl32(S / E) : +0.0) : fl32(S)
 *     Outputs no frame reaches are +0.0: samples past the frames' extent, and the gaps when hop > L.
 *   - Supported: channels 1 and n_fft a power of two in 16..4096; everything else -- complex output, other lengths -- is
 *     BHW_ERR_UNSUPPORTED.  An even n_fft = 2^a 3^b 5^c that is no power of two (400, 480, 960, ...) has calls of its own:
 *     bhw_istft_mfft_f32_*.
 *   - Descriptor: bhw_stft, where (as for bhw_stft_fft_f32_*) y_stride and y_batch_stride count FLOAT elements between spectrum rows
 *     and between signals; 0 means 2 * K and frames * y_stride; both must be even.  x_stride: floats between output signals.  flags:
 *     0 or BHW_OLA_NORMALIZE.  pad_mode must be 0, as for bhw_istft_ola_f32_*.
 *   - Determinism: the bits of output (b, t) depend only on the window, n_fft, hop, col0, pad, flags and the spectrum rows whose
 *     window covers t -- not on the batch, the plan, how a signal is cut into spans, the strides, or library versus table.
 *   - IEEE: a NaN or an infinity in spectrum row (b, f) makes exactly the outputs under that row's window non-finite; every other
 *     output keeps its bits.
 *   - Only the `samples` floats of each signal are written: the gaps of x_stride never are.
 *   - Checks before any HIP call (BHW_ERR_BADARG unless noted): everything bhw_istft_ola_f32_* checks for the descriptor with packed
 *     row strides (unknown flags, pad < col0, frames 0 with samples > 0, col0 + L > n_fft, shift, a nonzero pad_mode, the Taylor sources
 *     (BHW_ERR_UNSUPPORTED), ...), the unsupported n_fft or channels (BHW_ERR_UNSUPPORTED), y_stride below 2 * K or odd, y_batch_stride
 *     below (frames - 1) * y_stride + 2 * K or odd, batch * frames * n_fft above 2^34 (the overlap-add's cap, which keeps
 *     batch * frames * K below it), NULL pointers, d_Y not 8-byte aligned, d_x not 4-byte aligned, d_Y overlapping d_x, and (from a
 *     table) the key match.  samples 0 returns BHW_OK with the pointers unchecked.
 *   - The library form computes the coefficients by direct CORDIC and the twiddle factors in the kernel: no allocation, no scratch,
 *     capturable with no bhw_prepare_device.  The from-table form keeps the from-table contract: no allocation, no synchronisation,
 *     capturable on its first call.
 *   - bhw_describe_istft_fft: one line naming the route, the kernel and the plan: the radix schedule, the lanes per row, the spans a
 *     workgroup runs side by side, the span length S in frames, the halo (frames before a span that it transforms again), the share
 *     of transforms that are such repeats, the grid and the LDS bytes; under heavy overlap with little work (the halo sets S and few
 *     workgroups run) it says so.  t may be NULL (the library call).  Host arithmetic only. */
int bhw_istft_fft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                             const float *d_Y, float *d_x);
int bhw_istft_fft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                 const float *d_Y, float *d_x);
int bhw_describe_istft_fft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len);

/* Fused power and filter-bank spectrogram: the rows of bhw_stft_fft_f32_* formed and transformed by the same kernel body, and
 * written as |Y|^2 per bin or as those powers folded through a sparse filter bank (a mel bank, say), by ONE launch.  The spectrum
 * never reaches memory, so the call takes no workspace.
 *   - Row and transform: exactly those of bhw_stft_fft_f32_* for the same (p, length, s, flags); flags is 0 or
 *     BHW_WELCH_DETREND_CONSTANT.  Let (re, im) be the float32 pair that call writes for bin k of row (b, f), bit for bit.
 *   - Power, fb == NULL, W = K = n_fft / 2 + 1:
 *         d_P[b * y_batch_stride + f * y_stride + k] = fl32((double) re * (double) re + (double) im * (double) im)
 *     Both squares are exact in binary64 and the sum is one rounding (a fused multiply-add gives the same value), then one rounding
 *     to float32: the periodogram's q_f, rounded.
 *   - Filter bank, fb != NULL, W = filters.  With c_m = offset[m + 1] - offset[m] and P the float32 power above:
 *         d_P[... + m] = fl32(sum over i < c_m of (double) P[first[m] + i] * (double) weight[offset[m] + i])
 *     in ASCENDING i, in binary64, from +0.0 (each product is exact, so a fused multiply-add gives the same value).  c_m = 0 gives +0.0.
 *   - Strides: y_stride and y_batch_stride count FLOATS between output rows and between signals; 0 means W and frames * y_stride.
 *     No evenness rule applies; d_P is 4-byte aligned.  Only the W floats of each row are written.
 *   - Determinism: the bits of an output row depend on the window, n_fft, flags, the bank and that row's samples only -- not on the
 *     batch, the plan, the slot, the strides, or library versus table.
 *   - IEEE: a NaN or an infinity in x reaches only the rows whose window covers it.
 *   - Memory safety of the bank: the host cannot read the device arrays, so the kernel is safe whatever they hold: offset[m] and
 *     offset[m + 1] are clamped to [0, weights] with end >= begin, and a band stops at bin K.  A wrong bank gives wrong numbers and
 *     never an access outside d_weight or the power row.  (d_first holds `filters` and d_offset `filters + 1` readable entries.)
 *   - Checks before any HIP call (BHW_ERR_BADARG unless noted): everything bhw_stft_fft_f32_* checks on the input side (channels 2
 *     and an unsupported n_fft stay BHW_ERR_UNSUPPORTED), its output-stride and overlap rules with W in place of 2 * K (and no
 *     evenness), batch * frames * W above 2^34, and for fb: struct_size, reserved != 0, filters outside 1..4096, bins != K, weights
 *     above 2^24, a NULL d_first or d_offset, a NULL d_weight with weights > 0, any of the three not 4-byte aligned or overlapping
 *     d_P; and (from a table) the key match.  frames 0 returns BHW_OK with the pointers unchecked.
 *   - Capture: as bhw_stft_fft_f32_*.  The library form makes no allocation, uses no scratch and is capturable with no
 *     bhw_prepare_device; the from-table form is capturable on its first call.
 *   - Not built: magnitude (power 1); a complex output next to the power (the log of these rows is bhw_logspec_f32_* below);
 *     accumulating over frames in the kernel (Welch: bhw_welch_fft_f32_* is that call); complex input (bhw_stft_cfft_f32_* with
 *     BHW_CFFT_POWER is its power form).
 *     Other n_fft: bhw_stft_mfft_f32_* with BHW_MFFT_POWER writes these rows for an even n_fft = 2^a 3^b 5^c that is no power of two.
 *   - bhw_describe_spectrogram: the plan fields of bhw_describe_stft_fft's line in the same words, plus the mode, W, and for a bank
 *     filters, weights and filters per lane.  t may be NULL (the library call).  Host arithmetic only. */
typedef struct bhw_fbank {
    uint32_t struct_size;      /* sizeof(bhw_fbank) = 48                                                              */
    uint32_t filters;          /* 1..4096 output columns                                                              */
    uint32_t bins;             /* must equal n_fft / 2 + 1 of the call                                                */
    uint32_t weights;          /* total weights, <= 2^24: the value d_offset[filters] must hold                       */
    const uint32_t *d_first;   /* device, filters entries: first bin of filter m                                      */
    const uint32_t *d_offset;  /* device, filters + 1 entries, ascending from 0: filter m owns d_weight[offset[m] .. offset[m+1]) */
    const float *d_weight;     /* device, `weights` floats                                                            */
    uint64_t reserved;         /* 0                                                                                   */
} bhw_fbank;
int bhw_spectrogram_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                               const bhw_fbank *fb, const float *d_x, float *d_P);
int bhw_spectrogram_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                   const bhw_fbank *fb, const float *d_x, float *d_P);
int bhw_describe_spectrogram(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                             char *buf, uint64_t len);

/* Mixed-radix fused window and real FFT: the calls above for the row lengths speech and audio code uses and a power-of-two transform
 * refuses -- n_fft 400 (25 ms at 16 kHz), 480 and 960 (10 and 20 ms at 48 kHz), 1000, 1200, 1920 -- by ONE launch, in the three
 * output forms of bhw_stft_fft_f32_* and bhw_spectrogram_f32_*.  These are entry points of their own: bhw_stft_fft_f32_* and
 * bhw_spectrogram_f32_* keep refusing such n_fft, and these refuse a power of two, so there is one transform per n_fft and the bits of
 * a row never depend on which entry point was used.
 *   - Supported: channels 1 and n_fft EVEN, of the form 2^a 3^b 5^c, 16 <= n_fft < 4096, and not a power of two.  A power of two is
 *     BHW_ERR_UNSUPPORTED with a message that names bhw_stft_fft_f32_*; an odd n_fft, another prime factor, a value out of range and
 *     channels 2 are BHW_ERR_UNSUPPORTED.
 *   - flags: any combination of BHW_WELCH_DETREND_CONSTANT and BHW_MFFT_POWER.  fb non-NULL requires BHW_MFFT_POWER.  With the detrend
 *     flag pad, col0 and pad_mode must be 0, as for the segments call.
 *   - The row is pinned bit for bit: the float32 row bhw_stft_frames_f32_* (no detrend flag) or bhw_welch_frames_f32_* (with it) writes
 *     for the same descriptor -- those calls take any n_fft -- under the whole row contract of bhw_stft_fft_f32_*: the padding modes,
 *     col0, +0.0 around a window with L < n_fft, the mean in the header's fixed order, fl32(fl32(x - m) * v) unfused, and the Welch
 *     extent rule (frames - 1) * hop + L <= samples whenever pad, col0 and pad_mode are all 0.
 *   - The transform is NOT pinned bit for bit.  Sign and scaling of torch.fft.rfft.  A float32 Stockham transform of M = n_fft / 2
 *     complex points (the row taken as pairs): the radix-5 passes of M, then its radix-3 passes, then floor(a' / 2) radix-4 passes for
 *     M = 2^a' ..., then one radix-2 pass when a' is odd, the first pass without twiddles, and a split pass.  The schedule is a
 *     function of n_fft alone.  Every twiddle factor is an entry (or the negative of an entry) of ONE table W[k] = exp(-2 pi i k /
 *     n_fft), k < n_fft / 2, each component the float32 rounding of a binary64 value, read at an exact index and never a product;
 *     the radix-3 and radix-5 butterfly constants are float32 roundings of binary64 values.  Its error is that of a float32 FFT
 *     (relative l2 error of a row of the order of 2^-24 * log2(n_fft) at most); the tests hold it to twice the error of rocFFT on the
 *     same rows.
 *   - Spectrum form (no BHW_MFFT_POWER): rows of K = n_fft / 2 + 1 complex64 values as interleaved float pairs; y_stride and
 *     y_batch_stride count FLOATS, must be even, 0 means 2 * K and frames * y_stride; d_out is 8-byte aligned.  The imaginary parts
 *     of bins 0 and n_fft / 2 are written as +0.0.
 *   - Power form (BHW_MFFT_POWER, fb NULL): rows of W = K floats, fl32((double) re * (double) re + (double) im * (double) im) of the
 *     very pair the spectrum form writes; the strides count floats, 0 means W and frames * y_stride, no evenness rule applies and
 *     d_out is 4-byte aligned.
 *   - Bank form (BHW_MFFT_POWER, fb non-NULL): rows of W = filters floats, the powers folded through fb exactly as
 *     bhw_spectrogram_f32_* does: fb->bins = K, a binary64 fma sum in ascending bin order from +0.0 rounded once, and the same
 *     clamping (offsets into [0, weights] with end >= begin, a band stops at bin K), so a wrong bank never reads outside its arrays.
 *   - Determinism: the bits of an output row depend only on the window, n_fft, flags, the bank and that row's samples -- not on the
 *     batch, the slot, the group, the grid, the strides, or library versus table.
 *   - IEEE: a NaN or an infinity in x reaches only the rows whose window covers it.  Only the W floats of each row are written.
 *   - Checks before any HIP call (BHW_ERR_BADARG unless noted): unknown flag bits, fb without BHW_MFFT_POWER, everything the frames
 *     call or the segments call checks for the descriptor with packed output strides, the unsupported channels or n_fft
 *     (BHW_ERR_UNSUPPORTED), the fields of fb as bhw_spectrogram_f32_* checks them; frames 0 returns BHW_OK here with the pointers
 *     unchecked; the stride rules of the output form, batch * frames * K (spectrum) or batch * frames * W above 2^34, NULL pointers,
 *     alignment, d_out overlapping d_x or an array of fb; and (from a table) the key match.
 *   - Capture: the library form computes the coefficients by direct CORDIC and the twiddle factors in the kernel: no allocation, no
 *     scratch, capturable with no bhw_prepare_device.  The from-table form allocates nothing, never synchronises and is capturable
 *     on its first call.
 *   - The inverse at these lengths is bhw_istft_mfft_f32_* below.  Not built: I/Q input at these lengths; odd n_fft and prime factors
 *     of 7 and above.
 *   - bhw_describe_stft_mfft: bhw_describe_stft_fft's line in the same words, plus the output form and, for a bank, its filters,
 *     weights and filters per lane.  t may be NULL (the library call).  Host arithmetic only. */
#define BHW_MFFT_POWER 2u
int bhw_stft_mfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                             const bhw_fbank *fb, const float *d_x, float *d_out);
int bhw_stft_mfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                 const bhw_fbank *fb, const float *d_x, float *d_out);
int bhw_describe_stft_mfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                           char *buf, uint64_t len);

/* Fused log spectrogram, log-mel spectrogram and MFCC: the power or bank rows of bhw_spectrogram_f32_* (bhw_logspec_f32_*: n_fft a
 * power of two in 16..4096) or of bhw_stft_mfft_f32_* under BHW_MFFT_POWER (bhw_logspec_mfft_f32_*: its even 2^a 3^b 5^c sizes) taken
 * through a log and, optionally, a dense DCT matrix before they leave the kernel, by ONE launch.  Neither the powers nor the bank
 * rows nor the log rows reach memory.  No existing call changes.
 *   - Row, transform, power and bank: exactly those of the parent call for the same (p, length, s, flags, fb); flags is 0 or
 *     BHW_WELCH_DETREND_CONSTANT (BHW_MFFT_POWER is not a flag here: power is implied).  Let q be the float32 word the parent writes
 *     for column m of row (b, f): the power of bin m when fb is NULL, the bank value otherwise.
 *   - Log stage.  BHW_LOG_CLAMP: t = (q < floor) ? floor : (double) q; a NaN passes through, as torch.clamp(min=) passes it.
 *     BHW_LOG_ADD: t = (double) q + floor.  g_m = fl32(mult * log(t)): a binary64 natural log, one binary64 multiply, one rounding to
 *     float32.  mult is 1 for ln, 1 / ln 10 for log10, 10 / ln 10 for the dB of a power.  With coeffs == 0 the output row is g,
 *     W = K = n_fft / 2 + 1 or fb->filters.  The device's binary64 log is not correctly rounded, so the contract of this stage is
 *     "within one float32 ulp of fl32(mult * log(t)) evaluated in IEEE binary64".
 *   - DCT stage, coeffs > 0 (needs fb, dct_rows == fb->filters and filters <= n_fft: the log row waits in n_fft floats of LDS):
 *         c_j = fl32(sum over m < filters of (double) g_m * (double) d_dct[m * coeffs + j])
 *     a binary64 fma chain in ASCENDING m from +0.0, rounded once -- the arithmetic of the bank sum.  The output row is c,
 *     W = coeffs.  Given the g that was produced, this stage is exact.
 *   - Strides, determinism, IEEE and capture: as the parent, with this W.  d_out is 4-byte aligned; only the W floats of a row are
 *     written.
 *   - Memory safety: the kernel reads d_dct only at m < filters, j < coeffs, and its reads of the bank stay clamped as in
 *     bhw_spectrogram_f32_*.  A wrong bank or matrix gives wrong numbers, never a stray access.
 *   - Checks before any HIP call, in this order (BHW_ERR_BADARG unless noted): flag bits other than BHW_WELCH_DETREND_CONSTANT; everything
 *     the parent checks on the input side and on the fields of fb, in the parent's words (channels 2 is BHW_ERR_UNSUPPORTED with the
 *     words "real input"; an n_fft of the other family is BHW_ERR_UNSUPPORTED with a message that names the other family's call); ls
 *     NULL, its struct_size, reserved != 0, an unknown mode; floor not finite or <= 0; mult not finite or 0; coeffs above 4096;
 *     coeffs > 0 without fb; dct_rows != fb->filters; filters > n_fft with coeffs > 0; dct_rows * coeffs above 2^24.  frames 0
 *     returns BHW_OK here with the pointers unchecked.  Then the parent's output-stride, extent and overlap rules with this W, the
 *     pointers and the arrays of fb as the parent checks them, and d_dct: NULL, not 4-byte aligned, overlapping d_out or an array
 *     of fb; and (from a table) the key match.
 *   - Not built: top_db and Whisper's "max - 8" clamp (both need a per-signal maximum of the result: the caller applies it to the
 *     small output); magnitude (power 1); liftering and deltas; complex input (I/Q); a DCT without a bank.
 *   - bhw_describe_logspec / bhw_describe_logspec_mfft: the plan fields of the parent's line in the same words, plus the log stage
 *     and W.  t may be NULL (the library call).  Host arithmetic only. */
#define BHW_LOG_CLAMP 0u
#define BHW_LOG_ADD 1u
typedef struct bhw_logspec {
    uint32_t struct_size;      /* sizeof(bhw_logspec) = 48                                                            */
    uint32_t mode;             /* BHW_LOG_CLAMP or BHW_LOG_ADD                                                        */
    double floor;              /* the clamp floor or the added epsilon: finite and > 0                                */
    double mult;               /* finite and non-zero: the multiplier of the natural log                              */
    uint32_t coeffs;           /* 0: the log rows; 1..4096: DCT rows of `coeffs` columns                              */
    uint32_t dct_rows;         /* must equal fb->filters when coeffs > 0                                              */
    const float *d_dct;        /* device, dct_rows * coeffs floats (<= 2^24), row-major [m * coeffs + j]; coeffs > 0 */
    uint64_t reserved;         /* 0                                                                                   */
} bhw_logspec;
int bhw_logspec_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                           const bhw_fbank *fb, const bhw_logspec *ls, const float *d_x, float *d_out);
int bhw_logspec_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                               const bhw_fbank *fb, const bhw_logspec *ls, const float *d_x, float *d_out);
int bhw_describe_logspec(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                         const bhw_logspec *ls, char *buf, uint64_t len);
int bhw_logspec_mfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                const bhw_fbank *fb, const bhw_logspec *ls, const float *d_x, float *d_out);
int bhw_logspec_mfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                    const bhw_fbank *fb, const bhw_logspec *ls, const float *d_x, float *d_out);
int bhw_describe_logspec_mfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                              const bhw_logspec *ls, char *buf, uint64_t len);

/* Fused inverse mixed-radix real FFT, window and overlap-add: bhw_istft_fft_f32_* for the row lengths of bhw_stft_mfft_f32_* --
 * torch.fft.irfft(Y, n=n_fft) in front of bhw_istft_ola_f32_*, by ONE launch, for n_fft 400, 480, 960, 1000, 1200, 1920, ...  The time
 * rows never reach memory, so the call takes no workspace.  These are entry points of their own: bhw_istft_fft_f32_* keeps refusing
 * such n_fft, and these refuse a power of two, so there is one transform per n_fft.
 *   - Supported: channels 1 and exactly the n_fft bhw_stft_mfft_f32_* take: EVEN, of the form 2^a 3^b 5^c, 16 <= n_fft < 4096, and not a
 *     power of two.  A power of two is BHW_ERR_UNSUPPORTED with a message that names bhw_istft_fft_f32_*; an odd n_fft, another prime
 *     factor, a value out of range and channels 2 are BHW_ERR_UNSUPPORTED.
 *   - The row.  For b < batch, f < frames, r[j], j < n_fft, is the float32 inverse real transform of the K = n_fft / 2 + 1 bins
 *     Y[k] = d_Y[b * y_batch_stride + f * y_stride + 2 * k + {0, 1}], with the convention and the scaling of
 *     torch.fft.irfft(Y, n=n_fft).  1 / n_fft is no power of two here: the scaling is ONE float32 multiply of the transform's float32
 *     result by c = (float)(1.0 / (double) n_fft) -- a multiply, not a division, so that a plain C replay reproduces it on any IEEE
 *     machine whatever its division flags.  This is one rounding more than bhw_istft_fft_f32_* makes, whose scaling is exact.  The
 *     imaginary parts of bins 0 and n_fft / 2 never enter the arithmetic.  The transform is NOT pinned bit for bit.  The bits of a row
 *     depend on its K bins and n_fft only -- not on its place in a workgroup, the span that reads it, the grid, the strides or the
 *     route.
 *   - The transform.  A pre-split pass, then an inverse float32 Stockham transform of M = n_fft / 2 complex points in the schedule of
 *     bhw_stft_mfft_f32_*: the radix-5 passes of M, then its radix-3 passes, then the radix-4 passes, then one radix-2 pass when
 *     needed (5x5x4x2 at 400).  Every twiddle factor is an entry, or the negative of an entry, of ONE table W[k] = exp(+2 pi i k /
 *     n_fft), k < M, each component the float32 rounding of a binary64 sincospi, read at the exact index q * k * (n_fft / (r * Ns));
 *     indices >= M fold by a compare (W[i + M] = -W[i]), never a mask and never a product.  The radix-3 and radix-5 constants are the
 *     forward's float32 roundings of binary64 values; the butterflies are the forward's, conjugated.  Its error is that of a float32
 *     FFT (relative l2 error of a row of the order of 2^-24 * log2(n_fft) at most).
 *   - The sum.  Given those rows every output is exactly what bhw_istft_ola_f32_* defines on them: for t < samples, u = t + pad, over
 *     the frames f with 0 <= k = u - f * hop - col0 < L in ASCENDING f, in binary64 from +0.0:
 *         S = sum (double) r_f[u - f * hop] * (double) v[k],   E = sum (double) v[k]^2
 *         d_x[b * x_stride + t] = flags ? (E > 0 ? fl32(S / E) : +0.0) : fl32(S)
 *     Outputs no frame reaches are +0.0: samples past the frames' extent, and the gaps when hop > L.
 *   - Descriptor: bhw_stft, where y_stride and y_batch_stride count FLOAT elements between spectrum rows and between signals; 0 means
 *     2 * K and frames * y_stride; both must be even.  x_stride: floats between output signals.  flags: 0 or BHW_OLA_NORMALIZE.
 *     pad_mode must be 0, as for bhw_istft_ola_f32_*.
 *   - Determinism: the bits of output (b, t) depend only on the window, n_fft, hop, col0, pad, flags and the spectrum rows whose
 *     window covers t -- not on the batch, the plan, how a signal is cut into spans, the strides, or library versus table.
 *   - IEEE: a NaN or an infinity in spectrum row (b, f) makes exactly the outputs under that row's window non-finite; every other
 *     output keeps its bits.
 *   - Only the `samples` floats of each signal are written: the gaps of x_stride never are.
 *   - Checks before any HIP call (BHW_ERR_BADARG unless noted): everything bhw_istft_ola_f32_* checks for the descriptor with packed
 *     row strides (unknown flags, pad < col0, frames 0 with samples > 0, col0 + L > n_fft, shift, a nonzero pad_mode, the Taylor sources
 *     (BHW_ERR_UNSUPPORTED), ...), channels other than 1 and the unsupported n_fft (BHW_ERR_UNSUPPORTED), y_stride below 2 * K or odd,
 *     y_batch_stride below (frames - 1) * y_stride + 2 * K or odd, NULL pointers, d_Y not 8-byte aligned, d_x not 4-byte aligned, d_Y
 *     overlapping d_x, and (from a table) the key match.  samples 0 returns BHW_OK with the pointers unchecked.
 *   - The library form computes the coefficients by direct CORDIC and the twiddle factors in the kernel: no allocation, no scratch,
 *     capturable with no bhw_prepare_device.  The from-table form keeps the from-table contract: no allocation, no synchronisation,
 *     capturable on its first call.
 *   - Not built: I/Q output at these lengths; odd n_fft and prime factors of 7 and above; a fast path for heavy overlap.
 *   - bhw_describe_istft_mfft: bhw_describe_istft_fft's line in the same words and fields, with the mixed-radix schedule ("5x5x4x2").
 *     t may be NULL (the library call).  Host arithmetic only. */
int bhw_istft_mfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                              const float *d_Y, float *d_x);
int bhw_istft_mfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                  const float *d_Y, float *d_x);
int bhw_describe_istft_mfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len);

/* Fused window and complex FFT for interleaved I/Q input: the two-channel rows of bhw_stft_frames_f32_* (no detrend flag) or of
 * bhw_welch_frames_f32_* (BHW_WELCH_DETREND_CONSTANT) formed, transformed and written as their two-sided spectrum, or as its powers,
 * by ONE launch.  These are entry points of their own: bhw_stft_fft_f32_*, bhw_istft_fft_f32_* and bhw_spectrogram_f32_* keep
 * refusing channels 2.  Neither the windowed rows nor the means reach memory, so the call takes no workspace.
 *   - Supported: channels 2 (channels 1 is BHW_ERR_UNSUPPORTED: real input goes to bhw_stft_fft_f32_*) and n_fft a power of two in
 *     16..2048; everything else is BHW_ERR_UNSUPPORTED.  n_fft 4096 is out: a workgroup would need 80 KiB of dynamic LDS and 16
 *     complex columns (32 sample registers) per lane.  x is read exactly as bhw_stft_frames_f32_* / bhw_welch_frames_f32_* read it
 *     for channels 2: interleaved (re, im) float pairs, x_stride in floats (0 = 2 * samples), 4-byte aligned.
 *   - flags: any combination of BHW_WELCH_DETREND_CONSTANT, BHW_CFFT_POWER and BHW_CFFT_SHIFT.  With the detrend flag pad, col0 and
 *     pad_mode must be 0, as for the segments call.
 *   - The row is pinned bit for bit: n_fft complex points, the interleaved float pairs those calls would have written for the same
 *     descriptor -- the padding rule, col0, +0.0 around a window with L < n_fft, ONE coefficient v[k] for both parts of a pair.  With
 *     the detrend flag each channel has its own mean m_c = fl32(S_c / L), S_c summed in the FIXED order of bhw_welch_frames_f32_* (64
 *     binary64 partial sums by j mod 64 in ascending j, then the butterfly 32 ... 1), and the product is fl32(fl32(x - m_c) * v),
 *     unfused.  A row reads its L window columns only, so without padding (pad, col0 and pad_mode all 0) the extent rule is the
 *     segments' one, (frames - 1) * hop + L <= samples, with or without the detrend flag.
 *   - The transform is NOT pinned bit for bit.  Y[k] = sum over j of row[j] * exp(-2 pi i j k / n_fft) for k < n_fft: the sign of
 *     torch.fft.fft, no scaling.  It is a float32 Stockham transform of n_fft complex points in radix-4 passes (the first without
 *     twiddles) and one radix-2 pass at the end when log2(n_fft) is odd -- the passes bhw_stft_fft_f32_* runs for 2 * n_fft real
 *     points, without the split pass; every twiddle factor is the float32 rounding of a binary64 cosine or sine, read from one table
 *     and never a product.  Its error is that of a float32 FFT (relative l2 error of a row of the order of 2^-24 * log2(n_fft) at
 *     most); the tests hold it to twice the error of rocFFT on the same rows.
 *   - Outputs.  No BHW_CFFT_POWER: d_Y[b * y_batch_stride + f * y_stride + 2 * j + {0, 1}] = (re, im) of the bin of column j,
 *     complex64 as interleaved float pairs; y_stride and y_batch_stride count FLOATS, 0 means 2 * n_fft and frames * y_stride, both
 *     must be even and d_Y 8-byte aligned.  BHW_CFFT_POWER: float32 rows of n_fft values,
 *         d_Y[b * y_batch_stride + f * y_stride + j] = fl32((double) re * (double) re + (double) im * (double) im)
 *     of the very pair the spectrum form writes (the power contract of bhw_spectrogram_f32_*); the strides count floats, 0 means n_fft
 *     and frames * y_stride, no evenness rule applies and d_Y is 4-byte aligned.  Column j holds bin j, or with BHW_CFFT_SHIFT bin
 *     (j + n_fft / 2) mod n_fft (torch.fft.fftshift along the bins: the same values, permuted), in both forms.
 *   - Determinism: the bits of an output row depend only on the window, n_fft, the flags and the row's samples -- not on the batch,
 *     the slot, the group, the grid, the strides, or library versus table.
 *   - IEEE: a NaN or an infinity in x reaches only the rows whose window covers it; every other row keeps its bits.
 *   - Only the row's floats are written: the elements up to y_stride and the gaps of y_batch_stride never are.
 *   - Checks before any HIP call, in this order (BHW_ERR_BADARG unless noted): everything the frames call (no detrend flag) or the
 *     segments call (with it) checks for the descriptor with packed output strides; unknown flag bits; the unsupported n_fft or
 *     channels (BHW_ERR_UNSUPPORTED); frames 0 returns BHW_OK here with the pointers unchecked; the stride rules of the output form,
 *     batch * frames * n_fft above 2^34, NULL pointers, alignment, d_Y overlapping d_x; and (from a table) the key match.
 *   - Capture: as bhw_stft_fft_f32_*.  The library form makes no allocation, uses no scratch and is capturable with no
 *     bhw_prepare_device; the from-table form allocates nothing, never synchronises and is capturable on its first call.
 *   - Not built: n_fft 4096 and other lengths; a filter bank on the I/Q power rows; accumulating over frames in the kernel.  The
 *     inverse is bhw_istft_cfft_f32_* below.
 *   - bhw_describe_stft_cfft: bhw_describe_stft_fft's line in the same words for the complex transform (no split), the output form,
 *     whether the bins are shifted, and the kernel.  t may be NULL (the library call).  Host arithmetic only. */
#define BHW_CFFT_POWER 2u
#define BHW_CFFT_SHIFT 4u
int bhw_stft_cfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                             const void *d_x, void *d_Y);
int bhw_stft_cfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                 const void *d_x, void *d_Y);
int bhw_describe_stft_cfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len);

/* Mixed-radix fused window and complex FFT for interleaved I/Q input: bhw_stft_cfft_f32_* at n_fft = 2^a 3^b 5^c that is NOT a power
 * of two, 16 <= n_fft <= 2047, odd lengths included (91 sizes: 18, 20, 24, 25, 27, ... 2000, 2025).  The arguments, the flags
 * (BHW_WELCH_DETREND_CONSTANT | BHW_CFFT_POWER | BHW_CFFT_SHIFT), the row contract, the output forms, the strides, determinism, the
 * IEEE rule, capture and the order of the checks are those of bhw_stft_cfft_f32_* word for word; what differs:
 *   - Supported: channels 2 and the n_fft above.  Three refusals are BHW_ERR_UNSUPPORTED and each names the route that takes the
 *     call: a power of two (bhw_stft_cfft_f32_*: one transform per n_fft), channels 1 (bhw_stft_mfft_f32_*), any other n_fft (the
 *     set).  The upper end is the I/Q kernel's: 8 complex columns per lane on 256 lanes.
 *   - The transform is NOT pinned bit for bit.  Y[k] = sum over j of row[j] * exp(-2 pi i j k / n_fft), k < n_fft.  It is a float32
 *     Stockham transform of n_fft complex points in the passes of bhw_stft_mfft_f32_* applied to n_fft itself (radix 5, then 3, then
 *     4, then one radix-2 pass; seven passes at most), without a split pass; every twiddle factor is the float32 rounding of a
 *     binary64 cosine or sine, read from one table at an exact index and never a product.  Its error is that of a float32 FFT
 *     (relative l2 error of a row of the order of 2^-24 * log2(n_fft) at most); the tests hold it to twice the error of rocFFT on
 *     the same rows.
 *   - BHW_CFFT_SHIFT: column j holds bin (j + n_fft - n_fft / 2) mod n_fft, that is bin k goes to column (k + n_fft / 2) mod n_fft
 *     with integer division: torch.fft.fftshift along the bins, for an odd n_fft too.
 *   - Not built: accumulating over frames in the kernel (Welch) at these lengths; a filter bank on the I/Q power rows; prime
 *     factors of 7 and above; n_fft >= 2048.  The inverse is bhw_istft_cmfft_f32_* below.
 *   - bhw_describe_stft_cmfft: bhw_describe_stft_cfft's line in the same words ("stft cmfft ..."), with the mixed-radix schedule
 *     ("5x5x4x4") and the entries of the twiddle table (n_fft / 2 for an even n_fft, n_fft for an odd one).  t may be NULL (the
 *     library call).  Host arithmetic only. */
int bhw_stft_cmfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                              const void *d_x, void *d_Y);
int bhw_stft_cmfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                  const void *d_x, void *d_Y);
int bhw_describe_stft_cmfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len);

/* Fused inverse complex FFT, window and overlap-add for I/Q output: torch.fft.ifft in front of bhw_istft_ola_f32_* with channels 2,
 * by ONE launch -- the inverse of bhw_stft_cfft_f32_*.  A group of lanes owns a span of a signal's time axis, reads the n_fft bins of
 * every frame that reaches it, transforms them in LDS, and adds the windowed row into binary64 accumulators that it stores once.
 * The time rows never reach memory, so the call takes no workspace.  These are entry points of their own: bhw_istft_fft_f32_* keeps
 * refusing channels 2.
 *   - The row.  For b < batch, f < frames, r[j], j < n_fft, is the float32 inverse transform of the n_fft bins
 *     Y[k] = d_Y[b * y_batch_stride + f * y_stride + 2 * k + {0, 1}]: r[j] ~ (1 / n_fft) * sum over k < n_fft of Y[k] exp(+2 pi i j k /
 *     n_fft), complex: the sign and the scaling of torch.fft.ifft.  The 1 / n_fft is one exact power-of-two scaling of the float32
 *     result.  The transform is NOT pinned bit for bit: it is an inverse float32 Stockham transform of n_fft complex points with the
 *     passes of bhw_stft_cfft_f32_* (radix 4, the first without twiddles, one radix-2 pass at the end when log2(n_fft) is odd); every
 *     twiddle factor is the float32 rounding of a binary64 cosine or sine, conjugated, read from one table and never a product; the
 *     butterflies use +i.  The bits of a row depend on its bins, n_fft and the shift flag only -- not on its place in a workgroup, the
 *     span that reads it, the grid, the strides or the route.
 *   - The sum.  Given those rows every output is exactly what bhw_istft_ola_f32_* defines on them for channels 2: for t < samples,
 *     u = t + pad, over the frames f with 0 <= k = u - f * hop - col0 < L in ASCENDING f, in binary64 from +0.0, per part c of {0, 1}:
 *         S_c = sum (double) r_f[u - f * hop].c * (double) v[k],   E = sum (double) v[k]^2   (one E for both parts)
 *         d_x[b * x_stride + 2 * t + c] = BHW_OLA_NORMALIZE ? (E > 0 ? fl32(S_c / E) : +0.0) : fl32(S_c)
 *     Outputs no frame reaches are +0.0 in both parts: samples past the frames' extent, and the gaps when hop > L.
 *   - flags: any combination of BHW_OLA_NORMALIZE and BHW_CFFT_SHIFT.  With BHW_CFFT_SHIFT column j of a spectrum row holds bin
 *     (j + n_fft / 2) mod n_fft -- what bhw_stft_cfft_f32_* writes under the same flag; the kernel changes its load index and runs
 *     no extra pass.
 *   - Supported: channels 2 and n_fft a power of two in 16..2048.  channels 1 is BHW_ERR_UNSUPPORTED (real output goes to
 *     bhw_istft_fft_f32_*); n_fft 4096 and every other length is BHW_ERR_UNSUPPORTED.
 *   - Descriptor: bhw_stft, where y_stride and y_batch_stride count FLOAT elements between spectrum rows and between signals; 0
 *     means 2 * n_fft and frames * y_stride; both must be even and d_Y 8-byte aligned.  x_stride: floats between output signals, 0
 *     means 2 * samples, any value from 2 * samples; d_x is 4-byte aligned (a sample is stored as one 8-byte word where d_x and
 *     x_stride are on the 8-byte grid, as two 4-byte words otherwise: the same bits).  pad_mode must be 0.
 *   - Determinism: the bits of output (b, t) depend only on the window, n_fft, hop, col0, pad, flags and the spectrum rows whose
 *     window covers t -- not on the batch, the plan, how a signal is cut into spans, the strides, or library versus table.
 *   - IEEE: a bin of row (b, f) that is NaN in both parts makes both parts of exactly the outputs under that row's window
 *     non-finite; every other output keeps its bits.
 *   - Only the 2 * samples floats of each signal are written: the gaps of x_stride never are.
 *   - Checks before any HIP call, in this order (BHW_ERR_BADARG unless noted): everything bhw_istft_ola_f32_* checks for the
 *     descriptor with packed row strides (pad < col0, frames 0 with samples > 0, col0 + L > n_fft, shift, a nonzero pad_mode, x_stride
 *     below 2 * samples, batch * frames * n_fft above 2^34, the Taylor sources (BHW_ERR_UNSUPPORTED), ...); unknown flag bits; the
 *     unsupported channels, then the unsupported n_fft (BHW_ERR_UNSUPPORTED); samples 0 returns BHW_OK here with the strides and the
 *     pointers unchecked; y_stride below 2 * n_fft or odd, y_batch_stride below (frames - 1) * y_stride + 2 * n_fft or odd; NULL
 *     pointers, d_Y not 8-byte aligned, d_x not 4-byte aligned, d_Y overlapping d_x; and (from a table) the key match.
 *   - The library form computes the coefficients by direct CORDIC and the twiddle factors in the kernel: no allocation, no scratch,
 *     capturable with no warm call and no bhw_prepare_device.  The from-table form keeps the from-table contract: no allocation, no
 *     synchronisation, capturable on its first call.
 *   - Not built: n_fft 4096 and other lengths; a fast path under heavy overlap (the halo sets S and few workgroups run); complex
 *     data through the real entry points.
 *   - bhw_describe_istft_cfft: bhw_describe_istft_fft's line in the same words for the complex transform (no split), whether the bins
 *     are shifted, and the kernel.  t may be NULL (the library call).  Host arithmetic only. */
int bhw_istft_cfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                              const float *d_Y, float *d_x);
int bhw_istft_cfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                  const float *d_Y, float *d_x);
int bhw_describe_istft_cfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len);

/* Fused inverse mixed-radix complex FFT, window and overlap-add for I/Q output: bhw_istft_cfft_f32_* at the n_fft of
 * bhw_stft_cmfft_f32_* -- the inverse of that call, by ONE launch.  The arguments, the two flags (BHW_OLA_NORMALIZE |
 * BHW_CFFT_SHIFT; any other bit is BHW_ERR_BADARG), the sum (ascending f, binary64 from +0.0, S_c per part and one E, fl32(S_c / E)
 * where E > 0 under normalisation, +0.0 where no frame reaches), the descriptor and stride rules (y_stride in floats, even, default
 * 2 * n_fft; any x_stride from 2 * samples, odd ones included; d_x 4-byte aligned), determinism, the IEEE rule, the order of the
 * checks and the capture statement (no allocation, no workspace, no bhw_prepare_device; both forms capturable on their first call)
 * are those of bhw_istft_cfft_f32_* word for word; what differs:
 *   - Supported: channels 2 and exactly the n_fft of bhw_stft_cmfft_f32_*: 2^a 3^b 5^c in 16..2047 that is NOT a power of two (91
 *     sizes, 18 of them odd).  One transform per n_fft.  Three refusals are BHW_ERR_UNSUPPORTED and each names the route that takes
 *     the call: channels 1 (bhw_istft_mfft_f32_*), a power of two (bhw_istft_cfft_f32_*), any other n_fft (the set).
 *   - The row.  r[j], j < n_fft, is the float32 inverse transform of the n_fft bins of (b, f) with the sign and the scaling of
 *     torch.fft.ifft.  1 / n_fft is no power of two here: as in bhw_istft_mfft_f32_* the scaling is ONE float32 multiply of the
 *     transform's float32 result by c = (float)(1.0 / (double) n_fft), applied to each part -- one rounding more than
 *     bhw_istft_cfft_f32_*.  The transform is NOT pinned bit for bit: it is the forward float32 Stockham transform of
 *     bhw_stft_cmfft_f32_* (radix 5, then 3, then 4, then one radix-2 pass; every twiddle factor the float32 rounding of a binary64
 *     cosine or sine, read from one table at an exact index) applied to the bins with their parts swapped, and its result read with
 *     the parts swapped again: n_fft * IDFT(Y) = swap(DFT(swap(Y))).  The bits of a row depend on its bins, n_fft and the shift flag
 *     only.
 *   - BHW_CFFT_SHIFT: bin k is read from column (k + n_fft / 2) mod n_fft with integer division, that is column j holds bin
 *     (j + n_fft - n_fft / 2) mod n_fft -- what bhw_stft_cmfft_f32_* writes under the same flag (torch.fft.fftshift along the bins),
 *     for an odd n_fft too.  A load index (a compare and a subtract), not a pass.
 *   - Not built: n_fft >= 2048; prime factors of 7 and above; a fast path under heavy overlap; rerouting by n_fft inside
 *     bhw_istft_cfft_f32_*.
 *   - bhw_describe_istft_cmfft: bhw_describe_istft_cfft's line in the same words ("istft cmfft ..."), with the mixed-radix schedule
 *     and the entries of the twiddle table.  t may be NULL (the library call).  Host arithmetic only. */
int bhw_istft_cmfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                               const float *d_Y, float *d_x);
int bhw_istft_cmfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                   const float *d_Y, float *d_x);
int bhw_describe_istft_cmfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len);

/* Fused Welch PSD: window, real FFT and the average over the frames by ONE kernel and a small join.  The rows of bhw_stft_fft_f32_*
 * are formed and transformed by the same kernel body, and |Y|^2 is accumulated over the frames where the transform ends, so the
 * (B, F, K) spectrum that bhw_stft_fft_f32_* + bhw_welch_psd_f32 write and read back never exists.
 *   - Inputs: (p, length, s, flags) exactly as bhw_stft_fft_f32_* takes them (flags 0 or BHW_WELCH_DETREND_CONSTANT; the padding
 *     fields of s as that call accepts them, so the time average of a centred spectrogram comes free), except that s->y_stride and
 *     s->y_batch_stride must be 0: no spectrum is written.  scale and psd_flags (0 or BHW_PSD_ONESIDED) are bhw_psd's; d_P is float32
 *     (B, K), K = n_fft / 2 + 1, row b at b * p_stride floats (0 = K).
 *   - Row and transform: those of bhw_stft_fft_f32_* for the same (p, length, s, flags).  Let (re, im) be the float32 pair that call
 *     writes for bin k of row (b, f): the same words, from the same row function and the same split expression.
 *   - The sums, with q_f = (double) re * (double) re + (double) im * (double) im (both squares exact, one rounding: the q_f of
 *     bhw_welch_psd_f32):
 *        A_chunk = sum of q_f over the frames of one chunk, in ascending f, binary64 from +0.0
 *        A_blk   = sum of A_chunk over the chunks of one block, ascending, binary64 from +0.0
 *        A       = sum of A_blk over the blocks, ascending, binary64 from +0.0
 *        d_P[b * p_stride + k] = fl32(A * s_k),    s_k = scale * (doubled(k) ? 2 : 1)      (doubled: bhw_welch_psd_f32's rule)
 *     A chunk is BHW_WELCH_FFT_CHUNK = 16 consecutive frames (the last may be shorter), a block BHW_WELCH_BLOCK = 256 frames = 16
 *     chunks.  Both constants belong to this header and not to a plan: they ARE the order.
 *   - Consequences: the bits of P depend on the window, n_fft, the flags, scale and the signal's samples only -- not on B, the grid,
 *     or library versus table.  For F <= 16 the order is bhw_welch_psd_f32's plain ascending sum, so P equals bhw_welch_psd_f32 of
 *     bhw_stft_fft_f32_*'s rows bit for bit.  For larger F the two orders associate differently and P may differ from that route by
 *     at most one float32 ulp: both are roundings of binary64 sums of non-negative terms whose relative difference is below
 *     2 F * 2^-53.
 *   - Workspace: caller-provided, 8-byte aligned, bhw_welch_fft_workspace_bytes(s) bytes: the chunk sums, B * ceil(F / 16) * K
 *     doubles, followed, when F > 256, by the block sums, B * ceil(F / 256) * K doubles.  A short one is BHW_ERR_WORKSPACE.  No call
 *     allocates, and there are no float atomics: every chunk sum is stored plainly once and two small kernels join them in order.
 *   - Supported: exactly the set of bhw_stft_fft_f32_* (real input, channels 1, n_fft a power of two in 16..4096) with the same codes
 *     and words for refusals.
 *   - IEEE: a NaN or an infinity in x reaches only the bins of its own signal.  Zeros in give +0.0 out (for a scale >= 0).
 *   - Checks before any HIP call, in this order (BHW_ERR_BADARG unless noted): everything bhw_stft_fft_f32_* checks on the descriptor
 *     (with the y strides taken as packed), non-zero y strides, unknown psd_flags, a scale that is not finite; frames 0 returns BHW_OK
 *     here with the pointers unchecked; p_stride below K, B * ceil(F / 16) * K above 2^34; NULL d_x or d_P, either not 4-byte aligned,
 *     a NULL or misaligned workspace, a short one (BHW_ERR_WORKSPACE), d_P or the workspace overlapping d_x or each other; and (from a
 *     table) the key match.
 *   - Capture: as bhw_stft_fft_f32_*.  The library form needs no bhw_prepare_device; the from-table form is capturable on its first
 *     call.
 *   - Not built: max-hold or median averaging; a filter bank on the averaged powers.  (I/Q input and the mixed-radix n_fft have this
 *     epilogue, bhw_welch_cfft_f32_* and bhw_welch_mfft_f32_* below; cross spectra have it for two signals side by side,
 *     bhw_csd_fft_f32_* below.  Max-hold and min-hold traces exist for I/Q input: bhw_hold_cfft_f32_* and bhw_hold_cmfft_f32_* below.)
 *     Max-hold and min-hold traces of these rows: bhw_hold_fft_f32_* below.
 *   - bhw_describe_welch_fft: bhw_describe_stft_fft's line in the same words, plus the chunk, the runs, the groups per run, the
 *     accumulators per lane and the workspace bytes.  t may be NULL (the library call).  Host arithmetic only. */
/* Why 16: the frames of ONE signal are the only parallelism a long record has.  16 381 frames of one signal (2^24 samples, n_fft 4096,
 * hop 1024) are 1 024 independent chunk chains; chains of BHW_WELCH_BLOCK frames would be 64 on 256 compute units.  16 is also the
 * largest run that needs no carried sum for n_fft <= 128, where a workgroup holds 16 or more frames side by side. */
#define BHW_WELCH_FFT_CHUNK 16u
uint64_t bhw_welch_fft_workspace_bytes(const bhw_stft *s);
int bhw_welch_fft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                             double scale, uint32_t psd_flags, const float *d_x, float *d_P, uint64_t p_stride, void *workspace,
                             uint64_t workspace_bytes);
int bhw_welch_fft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                 double scale, uint32_t psd_flags, const float *d_x, float *d_P, uint64_t p_stride, void *workspace,
                                 uint64_t workspace_bytes);
int bhw_describe_welch_fft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len);

/* Fused Welch PSD for complex (I/Q) input: window, complex FFT and the average over the frames by ONE kernel and the join of
 * bhw_welch_fft_f32_*.  The rows of bhw_stft_cfft_f32_* are formed and transformed by the same kernel body, and |Y|^2 is accumulated
 * over the frames where the transform ends, so the (B, F, n_fft) spectrum that bhw_stft_cfft_f32_* + bhw_welch_psd_f32 write and read
 * back never exists.  The estimate is two-sided: n_fft bins, nothing is doubled, and there is no psd_flags.
 *   - Inputs: (p, length, s, flags) exactly as bhw_stft_cfft_f32_* takes them (channels 2, interleaved I/Q; the padding fields of s
 *     as that call accepts them), except that flags is any combination of BHW_WELCH_DETREND_CONSTANT and BHW_CFFT_SHIFT --
 *     BHW_CFFT_POWER is refused -- and s->y_stride and s->y_batch_stride must be 0: no spectrum is written.  scale is bhw_psd's; d_P
 *     is float32 (B, n_fft), row b at b * p_stride floats (0 = n_fft).
 *   - Row and transform: those of bhw_stft_cfft_f32_* for the same (p, length, s) and the detrend flag.  Let (re, im) be the float32
 *     pair that call writes for bin k of row (b, f), bit for bit: the same words, from the same row function.
 *   - The sums, with q_f = (double) re * (double) re + (double) im * (double) im, are those of bhw_welch_fft_f32_* above:
 *        A_chunk = sum of q_f over the frames of one chunk of BHW_WELCH_FFT_CHUNK = 16, in ascending f, binary64 from +0.0
 *        A_blk   = sum of A_chunk over the 16 chunks of one block of BHW_WELCH_BLOCK = 256 frames, ascending, binary64 from +0.0
 *        A       = sum of A_blk over the blocks, ascending, binary64 from +0.0
 *        d_P[b * p_stride + j] = fl32(A * scale)
 *     (the last chunk and the last block may be shorter).  Column j holds bin j, or with BHW_CFFT_SHIFT bin (j + n_fft / 2) mod
 *     n_fft, the column rule of bhw_stft_cfft_f32_*.
 *   - Consequences: the bits of P depend on the window, n_fft, the flags, scale and the signal's samples only -- not on B, the grid,
 *     or library versus table.  For F <= 16 P equals bhw_welch_psd_f32 (flags 0) of bhw_stft_cfft_f32_*'s rows bit for bit; beyond 16
 *     frames it lies within one float32 ulp of that route, by the argument given for bhw_welch_fft_f32_*.  There are no float
 *     atomics: every chunk sum is stored plainly once.
 *   - Workspace: caller-provided, 8-byte aligned, bhw_welch_cfft_workspace_bytes(s) bytes: the chunk sums, B * ceil(F / 16) * n_fft
 *     doubles, followed, when F > 256, by the block sums, B * ceil(F / 256) * n_fft doubles.  A short one is BHW_ERR_WORKSPACE.  No
 *     call allocates.
 *   - Supported: exactly the set of bhw_stft_cfft_f32_* (channels 2, n_fft a power of two in 16..2048); channels 1 and every other
 *     n_fft are BHW_ERR_UNSUPPORTED with that call's words.
 *   - IEEE: a NaN or an infinity in x reaches only the bins of its own signal.  Zeros in give +0.0 out (for a scale >= 0).
 *   - Checks before any HIP call, in this order (BHW_ERR_BADARG unless noted): everything bhw_stft_cfft_f32_* checks on the
 *     descriptor (with the y strides taken as packed); BHW_CFFT_POWER set, non-zero y strides, a scale that is not finite; frames 0
 *     returns BHW_OK here with the pointers unchecked; p_stride below n_fft, B * ceil(F / 16) * n_fft above 2^34; NULL d_x or d_P,
 *     either not 4-byte aligned; a NULL or misaligned workspace, a short one (BHW_ERR_WORKSPACE); d_P or the workspace overlapping
 *     d_x or each other; and (from a table) the key match.
 *   - Capture: as bhw_stft_cfft_f32_*.  The library form needs no bhw_prepare_device; the from-table form is capturable on its first
 *     call.
 *   - Not built: max-hold or median traces; n_fft 4096; I/Q cross spectra accumulated in the kernel (real input:
 *     bhw_csd_fft_f32_*); a filter bank on the averaged powers.  (I/Q input at the mixed-radix lengths: bhw_welch_cmfft_f32_* below.)
 *     (Max-hold and min-hold traces of the same rows: bhw_hold_cfft_f32_* below; a median is not built.)
 *   - bhw_describe_welch_cfft: bhw_describe_stft_cfft's line in the same words (without the output form), plus the fields
 *     bhw_describe_welch_fft adds.  t may be NULL (the library call).  Host arithmetic only. */
uint64_t bhw_welch_cfft_workspace_bytes(const bhw_stft *s);
int bhw_welch_cfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                              double scale, const float *d_x, float *d_P, uint64_t p_stride, void *workspace, uint64_t workspace_bytes);
int bhw_welch_cfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                  double scale, const float *d_x, float *d_P, uint64_t p_stride, void *workspace, uint64_t workspace_bytes);
int bhw_describe_welch_cfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len);

/* Fused Welch PSD at a mixed-radix n_fft (400, 480, 1000, 4000 ...): window, mixed-radix real FFT and the average over the frames by
 * ONE kernel and the join of bhw_welch_fft_f32_*.  The rows of bhw_stft_mfft_f32_* are formed and transformed by the same kernel body,
 * and |Y|^2 is accumulated over the frames where the transform ends, so the (B, F, K) spectrum that bhw_stft_mfft_f32_* +
 * bhw_welch_psd_f32 write and read back never exists.  The argument list is bhw_welch_fft_f32_*'s, word for word; the estimate is
 * one-sided, so psd_flags and the doubling rule are that call's.
 *   - Inputs: (p, length, s, flags) exactly as bhw_stft_mfft_f32_* takes them (channels 1; the padding fields of s as that call
 *     accepts them), except that flags is 0 or BHW_WELCH_DETREND_CONSTANT -- BHW_MFFT_POWER is refused, and there is no filter-bank
 *     argument -- and s->y_stride and s->y_batch_stride must be 0: no spectrum is written.  scale and psd_flags (0 or
 *     BHW_PSD_ONESIDED) are bhw_psd's; d_P is float32 (B, K), K = n_fft / 2 + 1, row b at b * p_stride floats (0 = K).
 *   - Row and transform: those of bhw_stft_mfft_f32_* for the same (p, length, s) and the detrend flag.  Let (re, im) be the float32
 *     pair that call writes for bin k <= M = n_fft / 2 of row (b, f), bit for bit: the same words, from the same row function and
 *     the same split expression.
 *   - The sums, with q_f = (double) re * (double) re + (double) im * (double) im, are those of bhw_welch_fft_f32_* above:
 *        A_chunk = sum of q_f over the frames of one chunk of BHW_WELCH_FFT_CHUNK = 16, in ascending f, binary64 from +0.0
 *        A_blk   = sum of A_chunk over the 16 chunks of one block of BHW_WELCH_BLOCK = 256 frames, ascending, binary64 from +0.0
 *        A       = sum of A_blk over the blocks, ascending, binary64 from +0.0
 *        d_P[b * p_stride + k] = fl32(A * s_k),    s_k = scale * (doubled(k) ? 2 : 1)      (doubled: bhw_welch_psd_f32's rule)
 *     (the last chunk and the last block may be shorter).
 *   - Consequences: the bits of P depend on the window, n_fft, the flags, scale and the signal's samples only -- not on B, the grid,
 *     or library versus table.  For F <= 16 P equals bhw_welch_psd_f32 of bhw_stft_mfft_f32_*'s rows bit for bit; beyond 16 frames it
 *     lies within one float32 ulp of that route, by the argument given for bhw_welch_fft_f32_*.  There are no float atomics: every
 *     chunk sum is stored plainly once.
 *   - Workspace: caller-provided, 8-byte aligned, bhw_welch_mfft_workspace_bytes(s) bytes: the chunk sums, B * ceil(F / 16) * K
 *     doubles, followed, when F > 256, by the block sums, B * ceil(F / 256) * K doubles.  A short one is BHW_ERR_WORKSPACE.  No call
 *     allocates.
 *   - Supported: exactly the set of bhw_stft_mfft_f32_* (channels 1, n_fft an even 2^a 3^b 5^c in 16..4095 that is no power of two);
 *     channels 2, a power of two and every other n_fft are BHW_ERR_UNSUPPORTED with that call's words.
 *   - IEEE: a NaN or an infinity in x reaches only the bins of its own signal.  Zeros in give +0.0 out (for a scale >= 0).
 *   - Checks before any HIP call, in this order (BHW_ERR_BADARG unless noted): everything bhw_stft_mfft_f32_* checks on the
 *     descriptor (with the y strides taken as packed and no bank), an unknown flag among them, with that call's code and words;
 *     BHW_MFFT_POWER set, non-zero y strides, unknown psd_flags, a scale that is not finite; frames 0 returns BHW_OK here with the
 *     pointers unchecked; p_stride below K; B * ceil(F / 16) * K above 2^34; NULL d_x or d_P, either not 4-byte aligned, a NULL or
 *     misaligned workspace; a short one (BHW_ERR_WORKSPACE); d_P or the workspace overlapping d_x or each other; and (from a table)
 *     the key match.
 *   - Capture: as bhw_stft_mfft_f32_*.  The library form needs no bhw_prepare_device; the from-table form is capturable on its first
 *     call.
 *   - Not built: odd n_fft and factors >= 7; cross spectra at these lengths in one kernel; max-hold or median traces.  (I/Q input
 *     at these lengths, odd ones included: bhw_welch_cmfft_f32_* below.  Max-hold and min-hold traces exist for I/Q input only:
 *     bhw_hold_cmfft_f32_* below.)  Max-hold and min-hold traces of these rows have since been built: bhw_hold_mfft_f32_* below.
 *   - bhw_describe_welch_mfft: bhw_describe_stft_mfft's line in the same words (without the output form), plus the fields
 *     bhw_describe_welch_fft adds.  t may be NULL (the library call).  Host arithmetic only. */
uint64_t bhw_welch_mfft_workspace_bytes(const bhw_stft *s);
int bhw_welch_mfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                              double scale, uint32_t psd_flags, const float *d_x, float *d_P, uint64_t p_stride, void *workspace,
                              uint64_t workspace_bytes);
int bhw_welch_mfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                  double scale, uint32_t psd_flags, const float *d_x, float *d_P, uint64_t p_stride, void *workspace,
                                  uint64_t workspace_bytes);
int bhw_describe_welch_mfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len);

/* Fused Welch PSD for complex (I/Q) input at a mixed-radix n_fft (400, 1000, 1200, 1536, odd lengths included): window, mixed-radix
 * complex FFT and the average over the frames by ONE kernel and the join of bhw_welch_fft_f32_*.  The rows of bhw_stft_cmfft_f32_* are
 * formed and transformed by the same kernel body, and |Y|^2 is accumulated over the frames where the transform ends, so the
 * (B, F, n_fft) spectrum that bhw_stft_cmfft_f32_* + bhw_welch_psd_f32 write and read back never exists.  The argument list is
 * bhw_welch_cfft_f32_*'s, word for word: the estimate is two-sided, n_fft bins, nothing is doubled, and there is no psd_flags.
 *   - Inputs: (p, length, s, flags) exactly as bhw_stft_cmfft_f32_* takes them (channels 2, interleaved I/Q; the padding fields of s
 *     as that call accepts them), except that flags is any combination of BHW_WELCH_DETREND_CONSTANT and BHW_CFFT_SHIFT --
 *     BHW_CFFT_POWER is refused -- and s->y_stride and s->y_batch_stride must be 0: no spectrum is written.  scale is bhw_psd's; d_P
 *     is float32 (B, n_fft), row b at b * p_stride floats (0 = n_fft).
 *   - Row and transform: those of bhw_stft_cmfft_f32_* for the same (p, length, s) and the detrend flag.  Let (re, im) be the float32
 *     pair that call writes for bin k of row (b, f), bit for bit: the same words, from the same row function.
 *   - The sums, with q_f = (double) re * (double) re + (double) im * (double) im, are those of bhw_welch_fft_f32_* above:
 *        A_chunk = sum of q_f over the frames of one chunk of BHW_WELCH_FFT_CHUNK = 16, in ascending f, binary64 from +0.0
 *        A_blk   = sum of A_chunk over the 16 chunks of one block of BHW_WELCH_BLOCK = 256 frames, ascending, binary64 from +0.0
 *        A       = sum of A_blk over the blocks, ascending, binary64 from +0.0
 *        d_P[b * p_stride + j] = fl32(A * scale)
 *     (the last chunk and the last block may be shorter).  Column j holds bin j, or with BHW_CFFT_SHIFT bin (j + n_fft - n_fft / 2)
 *     mod n_fft: bin k goes to column (k + n_fft / 2) mod n_fft, the column rule of bhw_stft_cmfft_f32_*.  n_fft / 2 is integer
 *     division, so for an odd n_fft the row is torch.fft.fftshift of the unshifted one (bin (n_fft + 1) / 2 comes first).
 *   - Consequences: the bits of P depend on the window, n_fft, the flags, scale and the signal's samples only -- not on B, the grid,
 *     or library versus table.  For F <= 16 P equals bhw_welch_psd_f32 (flags 0) of bhw_stft_cmfft_f32_*'s rows bit for bit; beyond
 *     16 frames it lies within one float32 ulp of that route, by the argument given for bhw_welch_fft_f32_*.  There are no float
 *     atomics: every chunk sum is stored plainly once.
 *   - Workspace: caller-provided, 8-byte aligned, bhw_welch_cmfft_workspace_bytes(s) bytes: the chunk sums, B * ceil(F / 16) * n_fft
 *     doubles, followed, when F > 256, by the block sums, B * ceil(F / 256) * n_fft doubles.  A short one is BHW_ERR_WORKSPACE.  No
 *     call allocates.
 *   - Supported: exactly the set of bhw_stft_cmfft_f32_* (channels 2, n_fft = 2^a 3^b 5^c in 16..2047 that is no power of two: 91
 *     sizes, 18 of them odd); channels 1, a power of two and every other n_fft are BHW_ERR_UNSUPPORTED with that call's words, which
 *     name the call that takes them.
 *   - IEEE: a NaN or an infinity in x reaches only the bins of its own signal.  Zeros in give +0.0 out (for a scale >= 0).
 *   - Checks before any HIP call, in this order (BHW_ERR_BADARG unless noted):
 *       1. everything bhw_stft_cmfft_f32_* checks on the descriptor (with the y strides taken as packed), with that call's codes and
 *          words: the descriptor and an unknown flag, channels 1, a power of two, an unsupported n_fft (BHW_ERR_UNSUPPORTED);
 *       2. BHW_CFFT_POWER set, then non-zero y strides, then a scale that is not finite;
 *       3. frames 0 returns BHW_OK here with the pointers unchecked;
 *       4. p_stride below n_fft, B * ceil(F / 16) * n_fft above 2^34;
 *       5. NULL d_x or d_P, either not 4-byte aligned;
 *       6. a NULL or misaligned workspace, a short one (BHW_ERR_WORKSPACE);
 *       7. d_P or the workspace overlapping d_x or each other;
 *       8. (from a table) the key match.
 *     Steps 2 to 7 are those of bhw_welch_cfft_f32_*, in its words.
 *   - Capture: as bhw_stft_cmfft_f32_*.  The library form needs no bhw_prepare_device; the from-table form is capturable on its
 *     first call.
 *   - Not built: n_fft >= 2048; factors of 7 and above; I/Q cross spectra accumulated in the kernel; max-hold or median traces.
 *     (Max-hold and min-hold traces of the same rows: bhw_hold_cmfft_f32_* below; a median is not built.)
 *   - bhw_describe_welch_cmfft: bhw_describe_stft_cmfft's line in the same words ("welch cmfft ...", without the output form), plus
 *     the fields bhw_describe_welch_fft adds.  t may be NULL (the library call).  Host arithmetic only. */
uint64_t bhw_welch_cmfft_workspace_bytes(const bhw_stft *s);
int bhw_welch_cmfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                               double scale, const float *d_x, float *d_P, uint64_t p_stride, void *workspace, uint64_t workspace_bytes);
int bhw_welch_cmfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                   double scale, const float *d_x, float *d_P, uint64_t p_stride, void *workspace, uint64_t workspace_bytes);
int bhw_describe_welch_cmfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len);

/* Fused max-hold and min-hold traces for complex (I/Q) input: window, complex FFT and the maximum and the minimum of |Y|^2 over the
 * frames by ONE kernel and a small join -- the two traces a spectrum analyser keeps beside the average, for occupancy, intermittent
 * emitters and the noise floor.  The rows of bhw_stft_cfft_f32_* are formed and transformed by the same kernel body, and the powers
 * are reduced over the frames where the transform ends, so the (B, F, n_fft) powers that bhw_stft_cfft_f32_* with BHW_CFFT_POWER
 * writes for an amax / amin to read back never exist.
 *   - Inputs: (p, length, s, flags) exactly as bhw_welch_cfft_f32_* takes them: channels 2, any combination of
 *     BHW_WELCH_DETREND_CONSTANT and BHW_CFFT_SHIFT -- BHW_CFFT_POWER is refused -- s->y_stride and s->y_batch_stride 0, and a
 *     finite scale.
 *   - Outputs: d_max and d_min are float32 (B, n_fft), row b at b * p_stride floats (0 = n_fft).  Either may be NULL: that trace is
 *     not written.  Both NULL is BHW_ERR_BADARG.  Both traces are always computed; the pointers only select what is stored, so there
 *     is one kernel family, not one per trace.  The alignment, p_stride and overlap rules are d_P's of bhw_welch_cfft_f32_*, applied
 *     to each output and between the two.
 *   - Values: let h_f be the float32 word that bhw_stft_cfft_f32_* with BHW_CFFT_POWER writes for bin k of row (b, f): fl32(re^2 +
 *     im^2), the binary64 sum of the two exact products rounded to float32, from the same row function.  Then
 *        d_max[b * p_stride + j] = fl32((double) max_f h_f * scale)         d_min[b * p_stride + j] = fl32((double) min_f h_f * scale)
 *     over the live frames f < F only.  Column j holds bin j, or with BHW_CFFT_SHIFT bin (j + n_fft / 2) mod n_fft, the column rule
 *     of bhw_stft_cfft_f32_* (integer division, a compare and a subtract).
 *   - NaN: if any h_f of a bin is a NaN, both traces of that bin are NaN (some quiet NaN), as an amax / amin over the frames gives.
 *     h_f is never negative, so the kernels reduce the float32 WORDS as unsigned integers: they order as the values do, and a NaN's
 *     word lies above +inf's and is carried up where a float maximum would drop it.  Infinities behave as IEEE says; an infinite
 *     maximum times a zero scale is a NaN.  A NaN or an infinity in x reaches only the bins of its own signal.  Zeros in give +0.0
 *     out (for a scale >= 0).
 *   - Consequences: the bits of both traces depend on the window, n_fft, the flags, scale and the signal's samples only -- not on B,
 *     the grid, the order of the reduction (a maximum has none), or library versus table.  At EVERY F the result equals the
 *     reduction of bhw_stft_cfft_f32_*'s power rows bit for bit; there is no ulp clause.
 *   - Workspace: caller-provided, 8-byte aligned, bhw_hold_cfft_workspace_bytes(s) = bhw_welch_cfft_workspace_bytes(s) bytes: a
 *     (max, min) pair of words is the 8 bytes of a chunk sum, per chunk of BHW_WELCH_FFT_CHUNK = 16 frames and, when F > 256, per
 *     block of BHW_WELCH_BLOCK frames.  The layout inside is not part of the contract.  Partial results are stored plainly, once
 *     each, and joined by small kernels: there are no float atomics.  A short workspace is BHW_ERR_WORKSPACE.  No call allocates.
 *   - Supported: exactly the set of bhw_welch_cfft_f32_* (channels 2, n_fft a power of two in 16..2048), with that call's codes and
 *     words for every refusal on the input side: both calls run the same check function.
 *   - Checks before any HIP call, in this order (BHW_ERR_BADARG unless noted):
 *       1. to 4. those of bhw_welch_cfft_f32_*, in its words (frames 0 returns BHW_OK at 3. with the pointers unchecked);
 *       5. NULL d_x; d_max and d_min both NULL; d_max, d_min or d_x not 4-byte aligned;
 *       6. a NULL or misaligned workspace, a short one (BHW_ERR_WORKSPACE);
 *       7. d_max or d_min overlapping d_x, d_max overlapping d_min, the workspace overlapping d_x, d_max or d_min;
 *       8. (from a table) the key match.
 *   - Capture: as bhw_welch_cfft_f32_*.  The library form needs no bhw_prepare_device; the from-table form is capturable on its
 *     first call.
 *   - Not built: median or percentile traces; the mean in the same launch (call bhw_welch_cfft_f32_* beside this one); real input;
 *     n_fft >= 2048 for I/Q input (2048 itself is taken here, 4096 is not).  Real input has calls of its own: bhw_hold_fft_f32_*
 *     and bhw_hold_mfft_f32_* below.
 *   - bhw_describe_hold_cfft: bhw_describe_welch_cfft's line field for field ("hold cfft ...", its own kernels and k_hold_join),
 *     plus the traces asked for: traces is a non-empty subset of BHW_HOLD_MAX | BHW_HOLD_MIN.  t may be NULL (the library call).
 *     Host arithmetic only. */
#define BHW_HOLD_MAX 1u
#define BHW_HOLD_MIN 2u
uint64_t bhw_hold_cfft_workspace_bytes(const bhw_stft *s);
int bhw_hold_cfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                             double scale, const float *d_x, float *d_max, float *d_min, uint64_t p_stride,
                             void *workspace, uint64_t workspace_bytes);
int bhw_hold_cfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                 double scale, const float *d_x, float *d_max, float *d_min, uint64_t p_stride,
                                 void *workspace, uint64_t workspace_bytes);
int bhw_describe_hold_cfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint32_t traces,
                           char *buf, uint64_t len);

/* The same traces at a mixed-radix n_fft (400, 1000, 1200, 1536, odd lengths included): the rows of bhw_stft_cmfft_f32_* under the
 * same epilogue.  The argument list is bhw_hold_cfft_f32_*'s, word for word, and so is the contract, with bhw_stft_cmfft_f32_* and
 * bhw_welch_cmfft_f32_* read for bhw_stft_cfft_f32_* and bhw_welch_cfft_f32_*:
 *   - Inputs, and every refusal on the input side, are bhw_welch_cmfft_f32_*'s (the same check function): channels 2, the 91 n_fft =
 *     2^a 3^b 5^c in 18..2025 that are no power of two, 18 of them odd; a power of two, real input and every other n_fft are
 *     BHW_ERR_UNSUPPORTED in that call's words.
 *   - Values: h_f is the float32 word bhw_stft_cmfft_f32_* writes under BHW_CFFT_POWER; the traces, the NaN rule, the consequences
 *     (bit for bit at every F) and the checks 5. to 8. are those above.  With BHW_CFFT_SHIFT bin k goes to column (k + n_fft / 2) mod
 *     n_fft, integer division: an odd n_fft follows torch.fft.fftshift.
 *   - Workspace: bhw_hold_cmfft_workspace_bytes(s) = bhw_welch_cmfft_workspace_bytes(s) bytes.
 *   - Not built: as above; factors of 7 and above. */
uint64_t bhw_hold_cmfft_workspace_bytes(const bhw_stft *s);
int bhw_hold_cmfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                              double scale, const float *d_x, float *d_max, float *d_min, uint64_t p_stride,
                              void *workspace, uint64_t workspace_bytes);
int bhw_hold_cmfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                  double scale, const float *d_x, float *d_max, float *d_min, uint64_t p_stride,
                                  void *workspace, uint64_t workspace_bytes);
int bhw_describe_hold_cmfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint32_t traces,
                            char *buf, uint64_t len);

/* Fused max-hold and min-hold traces for real input: window, real FFT and the maximum and the minimum of |Y|^2 over the frames by ONE
 * kernel and the join of bhw_hold_cfft_f32_* -- the two analyser traces beside the average of bhw_welch_fft_f32_*, for audio, vibration
 * and speech frames.  The rows of bhw_stft_fft_f32_* are formed and transformed by the same kernel body, and the powers are reduced over
 * the frames where the transform ends, so the (B, F, K) powers that bhw_spectrogram_f32_* writes for an amax / amin to read back never
 * exist.  The argument list is bhw_welch_fft_f32_*'s with the two outputs in d_P's place.
 *   - Inputs: (p, length, s, flags, scale, psd_flags) exactly as bhw_welch_fft_f32_* takes them: channels 1, flags 0 or
 *     BHW_WELCH_DETREND_CONSTANT, s->y_stride and s->y_batch_stride 0, a finite scale, psd_flags 0 or BHW_PSD_ONESIDED.
 *   - Outputs: d_max and d_min are float32 (B, K), K = n_fft / 2 + 1, row b at b * p_stride floats (0 = K).  Either may be NULL: that
 *     trace is not written.  Both NULL is BHW_ERR_BADARG.  Both traces are always computed; the pointers only select what is stored.
 *     The alignment, p_stride and overlap rules are those of bhw_hold_cfft_f32_*, with K columns and T floats of a signal.
 *   - Values: let h_f be the float32 word that bhw_spectrogram_f32_* stores for bin k of row (b, f): fl32((double) re * re +
 *     (double) im * im) of the split bin, the binary64 sum of the two exact products rounded to float32, from the same row function
 *     and the same split expression.  Then, over the live frames f < F only,
 *        d_max[b * p_stride + k] = fl32((double) max_f h_f * s_k)           d_min[b * p_stride + k] = fl32((double) min_f h_f * s_k)
 *        s_k = scale * 2.0 where bhw_welch_psd_f32's rule doubles bin k (psd_flags, k, K, n_fft), else scale
 *     s_k is the very factor of bhw_welch_fft_f32_*, so the traces are in that call's units and bracket its P for the same scale
 *     times F.
 *   - NaN: if any h_f of a bin is a NaN, both traces of that bin are NaN, as an amax / amin over the frames gives; the words are
 *     reduced as unsigned integers, as bhw_hold_cfft_f32_* explains.  Infinities behave as IEEE says.  A NaN or an infinity in x
 *     reaches only the bins of its own signal.  Zeros in give +0.0 out (for a scale >= 0).
 *   - Consequences: the bits of both traces depend on the window, n_fft, the flags, scale, psd_flags and the signal's samples only --
 *     not on B, the grid, the order of the reduction (a maximum has none), or library versus table.  At EVERY F the result equals the
 *     reduction of bhw_spectrogram_f32_*'s power rows bit for bit; there is no ulp clause.
 *   - Workspace: caller-provided, 8-byte aligned, bhw_hold_fft_workspace_bytes(s) = bhw_welch_fft_workspace_bytes(s) bytes: a
 *     (max, min) pair of words is the 8 bytes of a chunk sum.  The layout inside is not part of the contract.  Partial results are
 *     stored plainly, once each: there are no float atomics.  A short workspace is BHW_ERR_WORKSPACE.  No call allocates.
 *   - Supported: exactly the set of bhw_welch_fft_f32_* (channels 1, n_fft a power of two in 16..4096), with that call's codes and
 *     words for every refusal on the input side: both calls run the same check function.
 *   - Checks before any HIP call, in this order (BHW_ERR_BADARG unless noted): everything bhw_welch_fft_f32_* checks before its
 *     pointers, in its words (frames 0 returns BHW_OK there with the pointers unchecked); then the steps 5. to 8. of
 *     bhw_hold_cfft_f32_*.
 *   - Capture: as bhw_welch_fft_f32_*.  The library form needs no bhw_prepare_device; the from-table form is capturable on its first
 *     call.
 *   - Not built: median or percentile traces; the mean in the same launch (call bhw_welch_fft_f32_* beside this one); a filter bank
 *     on the traces; odd n_fft.
 *   - bhw_describe_hold_fft: bhw_describe_welch_fft's line field for field ("hold fft ...", its own kernels and k_hold_join), plus
 *     the traces asked for: traces is a non-empty subset of BHW_HOLD_MAX | BHW_HOLD_MIN.  t may be NULL (the library call).  Host
 *     arithmetic only. */
uint64_t bhw_hold_fft_workspace_bytes(const bhw_stft *s);
int bhw_hold_fft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                            double scale, uint32_t psd_flags, const float *d_x, float *d_max, float *d_min, uint64_t p_stride,
                            void *workspace, uint64_t workspace_bytes);
int bhw_hold_fft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                double scale, uint32_t psd_flags, const float *d_x, float *d_max, float *d_min, uint64_t p_stride,
                                void *workspace, uint64_t workspace_bytes);
int bhw_describe_hold_fft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint32_t traces,
                          char *buf, uint64_t len);

/* The same traces at a mixed-radix n_fft (400, 1000, 1200, 1536): the rows of bhw_stft_mfft_f32_* under the same epilogue.  The argument
 * list is bhw_hold_fft_f32_*'s, word for word, and so is the contract, with bhw_stft_mfft_f32_* and bhw_welch_mfft_f32_* read for
 * bhw_stft_fft_f32_* and bhw_welch_fft_f32_*:
 *   - Inputs, and every refusal on the input side, are bhw_welch_mfft_f32_*'s (the same check function): channels 1, the 95 even
 *     n_fft = 2^a 3^b 5^c in 16..4095 that are no power of two, flags 0 or BHW_WELCH_DETREND_CONSTANT (BHW_MFFT_POWER is refused); a
 *     power of two, I/Q input and every other n_fft are BHW_ERR_UNSUPPORTED in that call's words.
 *   - Values: h_f is the float32 word bhw_stft_mfft_f32_* writes under BHW_MFFT_POWER; the traces, s_k, the NaN rule, the
 *     consequences (bit for bit at every F) and the pointer checks are those above.
 *   - Workspace: bhw_hold_mfft_workspace_bytes(s) = bhw_welch_mfft_workspace_bytes(s) bytes.
 *   - Not built: as above; factors of 7 and above. */
uint64_t bhw_hold_mfft_workspace_bytes(const bhw_stft *s);
int bhw_hold_mfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                             double scale, uint32_t psd_flags, const float *d_x, float *d_max, float *d_min, uint64_t p_stride,
                             void *workspace, uint64_t workspace_bytes);
int bhw_hold_mfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                 double scale, uint32_t psd_flags, const float *d_x, float *d_max, float *d_min, uint64_t p_stride,
                                 void *workspace, uint64_t workspace_bytes);
int bhw_describe_hold_mfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint32_t traces,
                           char *buf, uint64_t len);

/* Fused Welch cross spectra: window, real FFT of TWO signals and the four averages over the frames by ONE kernel and a small join.  The
 * rows of bhw_stft_fft_f32_* of x and of y are formed and transformed side by side by the same kernel body, and the terms of
 * bhw_welch_csd_f32 are accumulated where the transforms end, so the two (B, F, K) spectra that 2 x bhw_stft_fft_f32_* +
 * bhw_welch_csd_f32 write and read back never exist.
 *   - Inputs: (p, length, s, flags, scale) as bhw_welch_fft_f32_* takes them; ONE bhw_stft describes both operands (the same samples,
 *     frames, hop, n_fft, padding and batch stride), and its y strides must be 0.  csd_flags is bhw_csd.flags: BHW_CSD_ONESIDED,
 *     BHW_CSD_BROADCAST_X and the output mask BHW_CSD_PXY ... BHW_CSD_H1 (any non-empty subset).  d_x and d_y are float32 signals,
 *     signal b at b * x_stride floats; under BHW_CSD_BROADCAST_X d_x holds ONE signal, paired with each of the B signals of d_y.  The
 *     five output pointers and o_stride are bhw_welch_csd_f32's (d_Pxy and d_H1 complex64, the others float32, row b at b * o_stride
 *     elements, 0 = K = n_fft / 2 + 1); a pointer is read only where its bit is set.
 *   - Rows and transforms: those of bhw_stft_fft_f32_* for the same (p, length, s, flags).  Let (xr, xi) and (yr, yi) be the float32
 *     pairs that call writes for bin k of row (b, f) of x and of y: the same words, from the same row function and split expression.
 *   - The terms, in binary64 from the float32 parts, each one rounding (the products are exact), as bhw_welch_csd_f32 forms them:
 *        xx = xr^2 + xi^2,  yy = yr^2 + yi^2,  re = xr * yr + xi * yi,  im = xr * yi - xi * yr
 *   - The sums S_xx, S_yy, C_re, C_im, each in the order of bhw_welch_fft_f32_*:
 *        chunk sums over the frames of a chunk of BHW_WELCH_FFT_CHUNK = 16, ascending f, binary64 from +0.0;
 *        block sums over the 16 chunks of a block of BHW_WELCH_BLOCK = 256 frames, ascending, from +0.0; then the blocks, ascending.
 *   - The outputs: from the four sums by the output formulas of bhw_welch_csd_f32, the unfused coherence expression and IEEE
 *     0 / 0 = NaN included.
 *   - Consequences: the bits depend on the window, n_fft, the flags, scale and the samples only -- not on B, the grid, or library
 *     versus table.  P_xx is bit for bit bhw_welch_fft_f32_* of x and P_yy that of y, at any F (the same term, order and scale).  For
 *     F <= 16 every output equals bhw_welch_csd_f32 of bhw_stft_fft_f32_*'s rows bit for bit.  Beyond 16 frames the cross terms are
 *     signed, so the one-ulp statement of bhw_welch_fft_f32_* does not carry over: both orders add F products that are exact in
 *     binary64, so C_re (and C_im) of the two routes differ by at most 2 F * 2^-53 * sum |term| <= 2 F * 2^-53 * sqrt(S_xx * S_yy)
 *     (Cauchy-Schwarz), and each part of P_xy by that times s_k plus one float32 ulp of the larger result.
 *   - Workspace: caller-provided, 8-byte aligned, bhw_csd_fft_workspace_bytes(s) = 4 * bhw_welch_fft_workspace_bytes(s) bytes: the
 *     chunk sums of the four chains, [(b * chunks + c) * 4 K + chain * K + k], then, when F > 256, the block sums in the same layout.
 *     A short one is BHW_ERR_WORKSPACE.  No call allocates, and there are no float atomics.
 *   - Supported: real input (channels 1), n_fft a power of two in 16..2048.  n_fft 4096 is BHW_ERR_UNSUPPORTED (the two operands side
 *     by side would need 80 KB of LDS): use bhw_stft_fft_f32_* + bhw_welch_csd_f32.  A mixed-radix n_fft and complex input are
 *     BHW_ERR_UNSUPPORTED naming bhw_stft_mfft_f32_* / bhw_stft_cfft_f32_* + bhw_welch_csd_f32.
 *   - IEEE: a NaN or an infinity in x or y reaches only the bins of its own pair.  Zeros in give P_xy = +0.0 and coherence NaN.
 *   - Checks before any HIP call, in this order (BHW_ERR_BADARG unless noted): everything bhw_welch_fft_f32_* checks on the descriptor,
 *     with the refusals named above and n_fft above 2048 (BHW_ERR_UNSUPPORTED); non-zero y strides; unknown csd_flags, an empty output
 *     mask, a scale that is not finite; frames 0 returns BHW_OK here with the pointers unchecked; o_stride below K; B * ceil(F / 16) *
 *     4 K above 2^34; NULL d_x or d_y, either not 4-byte aligned; a requested output that is NULL or misaligned (bhw_welch_csd_f32's
 *     rules); a NULL or misaligned workspace, a short one (BHW_ERR_WORKSPACE); any output or the workspace overlapping anything else
 *     (d_x and d_y may coincide: both are only read); and (from a table) the key match.
 *   - Capture: as bhw_welch_fft_f32_*.
 *   - Not built: n_fft 4096; mixed-radix and I/Q cross spectra; a two-chain kernel family for P_xy alone (four chains always run).
 *   - bhw_describe_csd_fft: bhw_describe_welch_fft's line in the same words for the pair plan (lanes per row is min(128, ...): n_fft
 *     2048 runs two butterflies per lane), plus the pairs per group and the outputs.  Host arithmetic only. */
uint64_t bhw_csd_fft_workspace_bytes(const bhw_stft *s);
int bhw_csd_fft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                           double scale, uint32_t csd_flags, const float *d_x, const float *d_y, float *d_Pxy, float *d_Pxx, float *d_Pyy,
                           float *d_Cxy, float *d_H1, uint64_t o_stride, void *workspace, uint64_t workspace_bytes);
int bhw_csd_fft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                               double scale, uint32_t csd_flags, const float *d_x, const float *d_y, float *d_Pxy, float *d_Pxx,
                               float *d_Pyy, float *d_Cxy, float *d_H1, uint64_t o_stride, void *workspace, uint64_t workspace_bytes);
int bhw_describe_csd_fft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint32_t csd_flags,
                         char *buf, uint64_t len);

/* Fused STFT, spectral mask and inverse STFT: bhw_stft_fft_f32_*, a real gain per bin, and bhw_istft_fft_f32_* by ONE launch -- the
 * analysis - modify - synthesis chain of a time-frequency mask (speech enhancement, source separation, spectral gating, a per-bin
 * equaliser).  The span kernel of bhw_istft_fft_f32_* forms every frame it needs in LDS from the signal: the window, the forward
 * transform, the gains, the inverse transform, the window again and the overlap-add.  Neither spectrum reaches memory, so the call
 * takes no workspace.
 *   - sa, the analysis descriptor: exactly what bhw_stft_fft_f32_* takes for d_x -- samples = T, pad, pad_mode BHW_PAD_REFLECT or
 *     BHW_PAD_CONSTANT, col0, x_stride (floats between input signals).  ss, the synthesis descriptor: exactly what bhw_istft_fft_f32_*
 *     takes for d_out -- samples = the output length, pad (with col0: the first output), pad_mode 0, x_stride = floats between output
 *     signals.  The y strides of both must be 0: there are no spectrum rows.  The two must agree on batch, frames, hop, n_fft, col0,
 *     shift and channels (1); a disagreement is BHW_ERR_BADARG naming the field.  flags: 0 or BHW_OLA_NORMALIZE (no detrending).
 *   - d_g: the real gain of bin k < K = n_fft / 2 + 1 of frame f of signal b is d_g[b * g_batch_stride + f * g_stride + k].  Either
 *     stride may be 0: one row for every frame, the same gains for every signal.  A nonzero g_stride is at least K, a nonzero
 *     g_batch_stride at least (frames - 1) * g_stride + K.  Floats between the rows are never read.
 *   - The rows, in terms of the two contracts above.  Y[b, f, k] = (re, im) is the float32 pair bhw_stft_fft_f32_* writes for
 *     (sa, d_x, flags 0); the masked bin is (fl32(re * g), fl32(im * g)), one float32 rounding per part; d_out is exactly what
 *     bhw_istft_fft_f32_* writes for (ss, flags) from those masked rows.  The three-call route and this call agree WORD FOR WORD.
 *   - Determinism: the bits of an output depend on the window, the descriptors' geometry, the flags, the samples and the gains under
 *     its frames only -- not on the batch, the plan, the spans, the strides, or library versus table.
 *   - IEEE: a NaN or an infinity in gain row (b, f), or in the samples of that frame, makes exactly the outputs under that frame's
 *     window non-finite; every other output keeps its bits.
 *   - Only the ss->samples floats of each output signal are written.  d_out may not overlap d_x or d_g: a span reads the samples under
 *     its halo frames again, so the call is not in place.
 *   - Supported: channels 1, n_fft a power of two in 16..2048 (the kernel keeps a forward and an inverse twiddle table in LDS, and at
 *     4096 the inverse kernel alone fills 64 KiB).  BHW_ERR_UNSUPPORTED naming the route that takes the input: 4096 names
 *     bhw_stft_fft_f32_* + bhw_istft_fft_f32_*, a mixed-radix n_fft bhw_stft_mfft_f32_* + bhw_istft_mfft_f32_*, channels 2
 *     bhw_stft_cfft_f32_* + bhw_istft_cfft_f32_*.
 *   - Checks before any HIP call, in this order (BHW_ERR_BADARG unless noted): the params and unknown flags; the three refusals above;
 *     everything bhw_stft_fft_f32_* checks on sa and everything bhw_istft_fft_f32_* checks on ss, both with packed row strides and in
 *     those calls' own words; nonzero y strides; the fields that must agree; ss->samples 0 returns BHW_OK here with the pointers
 *     unchecked; the gain strides; NULL pointers, any not 4-byte aligned, an extent beyond 2^60 elements; d_out overlapping d_x or d_g;
 *     and (from a table) the key match.
 *   - No workspace, no allocation, no float atomics.  The library form computes the coefficients by direct CORDIC and both twiddle
 *     tables in the kernel: capturable with no bhw_prepare_device.  The from-table form is capturable on its first call.
 *   - Not built: complex gains (bhw_cmask_fft_f32_* below take them); I/Q input (bhw_mask_cfft_f32_* below takes it); 4096; a gain computed in the kernel; a second output
 *     with the masked spectrum.  (A mixed-radix n_fft from 18 to 2000 has calls of its own: bhw_mask_mfft_f32_* below.)
 *   - bhw_describe_mask_fft: the plan fields of bhw_describe_istft_fft's line for ss in the same words (the plan IS that call's, but
 *     for the LDS bytes), with the kernel, "forward + inverse FFT", the analysis padding and the gain strides.  It takes the gain
 *     strides because its line and its checks need them.  t may be NULL (the library call).  Host arithmetic only. */
int bhw_mask_fft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                            uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out);
int bhw_mask_fft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                                uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride,
                                float *d_out);
int bhw_describe_mask_fft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                          uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);

/* Fused STFT, spectral mask and inverse STFT at a mixed-radix n_fft: bhw_stft_mfft_f32_*, a real gain per bin, and
 * bhw_istft_mfft_f32_* by ONE launch -- bhw_mask_fft_f32_* for the frame sizes speech and audio callers use (320, 400, 480, 960, 1000,
 * 1200, 1920).  The arguments are those of bhw_mask_fft_f32_device, _from_table and bhw_describe_mask_fft, word for word, and so is the
 * contract, stated by the two mixed-radix parents:
 *   - Y[b, f, k] = (re, im) is the float32 pair bhw_stft_mfft_f32_* writes for (sa, d_x, flags 0); the masked bin is
 *     (fl32(re * g), fl32(im * g)), one float32 rounding per part; d_out is exactly what bhw_istft_mfft_f32_* writes for (ss, flags)
 *     from those masked rows.  The three-call route and this call agree WORD FOR WORD.  K = n_fft / 2 + 1.
 *   - The descriptors, the gain strides (0: one row for every frame / the same gains for every signal), ss->samples 0 -> BHW_OK, the
 *     determinism and IEEE statements and the overlap rules are bhw_mask_fft_f32_*'s.
 *   - Supported: channels 1, n_fft even, 2^a 3^b 5^c, no power of two, from 18 to 2000: 73 of the 95 lengths bhw_stft_mfft_f32_* takes
 *     (a lane keeps at most 8 ring columns and the two twiddle tables fit 40 000 bytes of LDS; the 22 lengths from 2160 to 4050 need
 *     16 columns and up to 81 000 bytes).  BHW_ERR_UNSUPPORTED naming the route that takes the input: channels 2 names
 *     bhw_stft_cmfft_f32_* + bhw_istft_cmfft_f32_*, a power of two in 16..2048 bhw_mask_fft_f32_*, 4096 bhw_stft_fft_f32_* +
 *     bhw_istft_fft_f32_*, a mixed-radix length above 2047 bhw_stft_mfft_f32_* + bhw_istft_mfft_f32_*.
 *   - Checks before any HIP call, in this order (BHW_ERR_BADARG unless noted): the params and unknown flags; the four refusals above;
 *     everything bhw_stft_mfft_f32_* checks on sa and everything bhw_istft_mfft_f32_* checks on ss, both with packed row strides and
 *     in those calls' own words; then what bhw_mask_fft_f32_* checks after its parents, in its words and its order.
 *   - No workspace, no allocation, no float atomics; both forms are capturable as bhw_mask_fft_f32_*'s are.
 *   - Not built: complex gains (bhw_cmask_mfft_f32_* below take them); I/Q input (bhw_mask_cmfft_f32_* below takes it); n_fft >= 2048; a gain computed in the kernel; a second
 *     output with the masked spectrum.
 *   - bhw_describe_mask_mfft: the plan fields of bhw_describe_istft_mfft's line for ss in the same words (the plan IS that call's, but
 *     for the LDS bytes), with the kernel, "forward + inverse FFT", the analysis padding and the gain strides. */
int bhw_mask_mfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                             uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out);
int bhw_mask_mfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                                 uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride,
                                 float *d_out);
int bhw_describe_mask_mfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                           uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);

/* Fused STFT, COMPLEX spectral gain and inverse STFT: bhw_mask_fft_f32_* and bhw_mask_mfft_f32_* with a complex gain per bin -- a
 * complex ratio mask (phase as well as magnitude), a frequency response H[k] as one (K,) row, a fractional delay
 * exp(-2 pi i k d / n_fft), one channel's beamforming weight per bin.  Still ONE launch and no spectrum in memory.  The arguments are
 * those of the real-gain calls of the same family, word for word, with one difference:
 *   - d_g points to interleaved float32 pairs (gr, gi), and g_stride / g_batch_stride count PAIRS.  The gain of bin k < K =
 *     n_fft / 2 + 1 of frame f of signal b is the pair at d_g + 2 * (b * g_batch_stride + f * g_stride + k).  Either stride may be 0; a
 *     nonzero g_stride is at least K, a nonzero g_batch_stride at least (frames - 1) * g_stride + K.  Pairs between the rows are never
 *     read.  d_g must be 8-byte aligned (a message of its own), and its extent, the 2^60 bound, the wrap and the overlap with d_out
 *     are computed in 8-byte elements.
 *   - The rows.  Y[b, f, k] = (re, im) is the float32 pair bhw_stft_fft_f32_* (bhw_stft_mfft_f32_*) writes for (sa, d_x, flags 0).
 *     The masked bin is
 *         re' = fl32( fl32(re * gr) - fl32(im * gi) )
 *         im' = fl32( fl32(re * gi) + fl32(im * gr) )
 *     -- each of the four products rounded on its own, none fused into the subtraction or the addition.  d_out is exactly what
 *     bhw_istft_fft_f32_* (bhw_istft_mfft_f32_*) writes for (ss, flags) from those masked rows: WORD FOR WORD, with no tolerance.
 *     This is what separate float32 operations on the real and imaginary planes give; it is NOT promised to equal a library's complex
 *     multiply Y * G bit for bit (such a multiply may fuse a product into the sum), only to within that multiply's rounding.
 *   - Bins 0 and n_fft / 2: the forward parents store im = 0 there and the inverse parents read only the real parts, so gi enters
 *     through re' = fl32(re * gr) - fl32(0 * gi) alone: a finite gi changes nothing, a NaN or an infinity there is one in the row.
 *   - The descriptors, ss->samples 0 -> BHW_OK, the determinism and IEEE statements (a non-finite part of a gain pair counts as a
 *     non-finite gain), the rule that d_out overlaps neither d_x nor d_g, capture, workspace (none) and the order of the checks are
 *     the real-gain calls'.
 *   - Supported: what the real-gain call of the family takes -- bhw_cmask_fft_f32_*: a power of two in 16..2048;
 *     bhw_cmask_mfft_f32_*: even 2^a 3^b 5^c in 18..2000, no power of two (73 sizes).  BHW_ERR_UNSUPPORTED in the real-gain calls'
 *     sentences, about "the fused complex-gain mask": channels 2 names the I/Q transforms, 4096 and the mixed-radix lengths above 2047
 *     the pairs of transforms, and the other family's sizes name bhw_cmask_mfft_f32_* / bhw_cmask_fft_f32_*.
 *   - Not built: n_fft >= 2048 (mixed) / 4096; a gain computed in the kernel; a second output with the masked spectrum.  (I/Q input:
 *     bhw_cmask_cfft_f32_* and bhw_cmask_cmfft_f32_* below.)
 *   - bhw_describe_cmask_fft / _mfft: bhw_describe_mask_fft's / _mfft's line -- the plan IS that call's for the same arguments: lanes,
 *     spans, columns per lane and LDS bytes; the gains live in registers -- beginning "cmask", naming k_cmask_*_direct / _table and
 *     saying "complex gains" before the strides (in pairs). */
int bhw_cmask_fft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                             uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out);
int bhw_cmask_fft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                                 uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride,
                                 float *d_out);
int bhw_describe_cmask_fft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                           uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);
int bhw_cmask_mfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                              uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out);
int bhw_cmask_mfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                                  uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride,
                                  float *d_out);
int bhw_describe_cmask_mfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                            uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);

/* Fused STFT, a REAL OR COMPLEX gain per bin and inverse STFT for I/Q INPUT: the four calls above for complex baseband -- excision
 * and blanking masks, an equaliser or channeliser response H[k] as one (K,) row, a fractional delay, per-channel beamforming weights.
 * ONE launch, no spectrum in memory, no workspace.  bhw_mask_cfft_f32_* / bhw_cmask_cfft_f32_*: n_fft a power of two in 16..2048;
 * bhw_mask_cmfft_f32_* / bhw_cmask_cmfft_f32_*: the 91 sizes 2^a 3^b 5^c in 18..2025 that are no power of two, odd ones included.
 * The arguments are those of bhw_mask_fft_f32_device / _from_table / bhw_describe_mask_fft, word for word, with these differences:
 *   - d_x and d_out hold interleaved I/Q (two floats a sample; x_stride counts floats, 0 = 2 * samples) and both descriptors carry
 *     channels = 2.  sa is checked exactly as bhw_stft_cfft_f32_* (bhw_stft_cmfft_f32_*) checks it with flags 0 and ss as
 *     bhw_istft_cfft_f32_* (bhw_istft_cmfft_f32_*) checks it with `flags`, in those calls' words and with packed row strides.
 *   - K = n_fft: every bin takes a gain, at an odd n_fft too.  bhw_mask_*: d_g holds floats; bhw_cmask_*: interleaved pairs (gr, gi),
 *     8-byte aligned, the strides in pairs.  The gain of column j of frame f of signal b is at b * g_batch_stride + f * g_stride + j;
 *     either stride may be 0, a nonzero g_stride is at least K, a nonzero g_batch_stride at least (frames - 1) * g_stride + K.
 *   - flags: BHW_OLA_NORMALIZE and BHW_CFFT_SHIFT.  With BHW_CFFT_SHIFT the gain of bin k is read from column (k + n_fft / 2) mod
 *     n_fft (integer division at an odd n_fft too) -- the column bhw_stft_c[m]fft_f32_* writes bin k to and bhw_istft_c[m]fft_f32_*
 *     reads it from under the same flag, torch.fft.fftshift along the bins: a mask designed on a centred frequency axis is passed as
 *     it is.  (At an even n_fft column j then holds the gain of bin (j + n_fft / 2) mod n_fft; at an odd one of bin
 *     (j + n_fft / 2 + 1) mod n_fft.)  The shift is a load index in the kernel, never a pass over the data, and it does not touch d_x
 *     or d_out.  Detrending has no inverse and is refused with the other unknown flag bits.
 *   - NO BIN IS SPECIAL (unlike bhw_cmask_fft_f32_* above): bins 0 and n_fft / 2 of a complex signal carry an imaginary part, and gi
 *     acts on them as on every other bin.
 *   - The rows, exact and without tolerance.  Y[b, f, k] = (re, im) is the pair bhw_stft_cfft_f32_* (bhw_stft_cmfft_f32_*) writes for
 *     (sa, d_x, flags 0).  The masked bin under a real gain g is (fl32(re * g), fl32(im * g)); under a pair
 *         re' = fl32( fl32(re * gr) - fl32(im * gi) )
 *         im' = fl32( fl32(re * gi) + fl32(im * gr) )
 *     with nothing contracted.  d_out is what bhw_istft_cfft_f32_* (bhw_istft_cmfft_f32_*) writes for (ss, flags & BHW_OLA_NORMALIZE)
 *     from those rows, WORD FOR WORD.  Equality with a library's complex multiply is not promised.
 *   - Determinism: an output's bits depend only on the window, the geometry, the flags, the samples and the gains under its frames.
 *     IEEE: a NaN or infinity in one gain (or one part of it), or in either part of one sample, reaches exactly the outputs under
 *     those frames' windows.  ss->samples 0 -> BHW_OK.  d_out overlaps neither d_x nor d_g (extents in floats of two per sample, and
 *     in gain elements).  No workspace, no allocation, no float atomics; both forms can be captured in a HIP graph.
 *   - BHW_ERR_UNSUPPORTED names the route that takes the input: channels 1 the real-signal mask call of the same gain type and
 *     family; a size of the other family the sibling among these four; 4096 and the mixed-radix lengths above 2047, which no fused
 *     I/Q transform takes either, the pair of I/Q transforms whose range this call shares.
 *   - bhw_describe_[c]mask_c[m]fft: the line of bhw_describe_istft_c[m]fft for (ss, flags) with the kernel name, "forward + inverse
 *     FFT", the analysis padding, the gain strides ("complex gains:" for pairs), "gain columns shifted" / "in order" and the LDS
 *     bytes of this call. */
int bhw_mask_cfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                             uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out);
int bhw_mask_cfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                                 uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride,
                                 float *d_out);
int bhw_describe_mask_cfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                           uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);
int bhw_cmask_cfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                              uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out);
int bhw_cmask_cfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                                  uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride,
                                  float *d_out);
int bhw_describe_cmask_cfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                            uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);
int bhw_mask_cmfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                              uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out);
int bhw_mask_cmfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                                  uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride,
                                  float *d_out);
int bhw_describe_mask_cmfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                            uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);
int bhw_cmask_cmfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                               uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out);
int bhw_cmask_cmfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                                   uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride,
                                   float *d_out);
int bhw_describe_cmask_cmfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                             uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len);

/* Fused multichannel FILTER-AND-SUM: STFT of every channel, a complex weight per channel and bin, the sum over the channels in the
 * frequency domain and ONE inverse STFT -- a delay-and-sum, MVDR, GEV or any other filter-and-sum beamformer over n_ch microphone
 * channels, in one launch.  Per output frame: n_ch forward transforms and one inverse; no spectrum reaches memory and there is no
 * workspace.  bhw_beam_fft_f32_*: n_fft a power of two in 16..2048; bhw_beam_mfft_f32_*: even 2^a 3^b 5^c in 18..2000, no power of
 * two (73 sizes).  The arguments are those of bhw_cmask_fft_f32_* (bhw_cmask_mfft_f32_*), word for word, with these additions:
 *   - n_ch: the channels of one signal, 1..BHW_BEAM_MAX_CH.  sa->batch == ss->batch == B counts OUTPUT signals: d_out is (B, T_out),
 *     one signal per group of n_ch channels.
 *   - x_ch_stride: floats between the channels of one signal; 0 = sa->samples, otherwise at least that.  Channel c of signal b starts
 *     at d_x + b * sa->x_stride + c * x_ch_stride.  sa->x_stride 0 = n_ch channel strides, otherwise at least
 *     (n_ch - 1) * x_ch_stride + samples.  Floats between the channels and between the signals are never read.
 *   - g_ch_stride: PAIRS between the gain rows of the channels, as g_stride and g_batch_stride count pairs.  The gain row of frame f
 *     of channel c of signal b starts at d_g + 2 * (b * g_batch_stride + c * g_ch_stride + f * g_stride).  g_stride and
 *     g_batch_stride may be 0 (one row for every frame; the same weights for every signal).  g_ch_stride is at least
 *     (frames - 1) * g_stride + K and may not be 0 when n_ch > 1: equal weights on every channel are a sum of the channels of x in
 *     front of bhw_cmask_*, and the refusal says so.  A nonzero g_batch_stride is at least (n_ch - 1) * g_ch_stride +
 *     (frames - 1) * g_stride + K.  Pairs between the rows are never read.
 *   - The rows, exact and without tolerance.  With Y_c[b, f, k] = (re, im) the pair bhw_stft_fft_f32_* (bhw_stft_mfft_f32_*) writes
 *     for channel c of signal b under (sa, flags 0) and (gr, gi) that channel's gain of the bin,
 *         P_c.re = fl32( fl32(re * gr) - fl32(im * gi) )
 *         P_c.im = fl32( fl32(re * gi) + fl32(im * gr) )
 *     as in bhw_cmask_*, and the sum runs per part in float32 in ascending channel order: Z = P_0, then Z = fl32(Z + P_c) for
 *     c = 1 .. n_ch - 1.  Nothing is contracted.  d_out is exactly what bhw_istft_fft_f32_* (bhw_istft_mfft_f32_*) writes for
 *     (ss, flags) from the rows Z: WORD FOR WORD.  This is what eager float32 operations on the two planes give in a loop over the
 *     channels.  The weights are applied as given: a caller with w^H x passes conj(w).
 *   - Bins 0 and n_fft / 2 behave per channel as in bhw_cmask_*: the forward parents store im = 0 there and the inverse parents read
 *     only the real part of the sum.  With n_ch == 1 the call equals bhw_cmask_fft_f32_* (bhw_cmask_mfft_f32_*) bit for bit.
 *   - Determinism: an output's bits depend only on the window, the geometry, the flags, the samples of the channels and the gains
 *     under its frames, never on the batch, the grid, or library versus table.  IEEE: a NaN or infinity in one sample of one channel,
 *     or in one part of one gain pair, reaches exactly the outputs under the frames concerned.  ss->samples 0 -> BHW_OK.  d_out
 *     overlaps neither any channel of d_x nor d_g.  No workspace, no allocation, no float atomics; both forms can be captured in a
 *     HIP graph.  The checks go in the order of bhw_cmask_*: n_ch behind the fields the descriptors share, the channel strides with
 *     the gain strides, the extents (up to 2^60 elements, the channel axis included) and the overlaps last.
 *   - BHW_ERR_UNSUPPORTED in the sentences of bhw_cmask_*, about "the fused beamformer": channels 2 names the I/Q transforms, 4096
 *     and the mixed-radix lengths above 2047 the pairs of transforms, the other family's sizes bhw_beam_mfft_f32_* /
 *     bhw_beam_fft_f32_*.
 *   - Not built: I/Q input (bhw_cmask_cfft_f32_* per channel and a sum take it); real gains; more than one output beam a launch;
 *     weights computed in the kernel.
 *   - bhw_describe_beam_fft / _mfft: bhw_describe_cmask_fft's / _mfft's line -- the plan IS that call's for B signals: the sums live
 *     in registers -- beginning "beam", naming k_beam_*_direct / _table and saying "channels C" and the three gain strides. */
#define BHW_BEAM_MAX_CH 64u
int bhw_beam_fft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                            uint32_t flags, const float *d_x, uint32_t n_ch, uint64_t x_ch_stride, const float *d_g, uint64_t g_stride,
                            uint64_t g_ch_stride, uint64_t g_batch_stride, float *d_out);
int bhw_beam_fft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                                uint32_t flags, const float *d_x, uint32_t n_ch, uint64_t x_ch_stride, const float *d_g, uint64_t g_stride,
                                uint64_t g_ch_stride, uint64_t g_batch_stride, float *d_out);
int bhw_describe_beam_fft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                          uint32_t n_ch, uint64_t x_ch_stride, uint64_t g_stride, uint64_t g_ch_stride, uint64_t g_batch_stride, char *buf,
                          uint64_t len);
int bhw_beam_mfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                             uint32_t flags, const float *d_x, uint32_t n_ch, uint64_t x_ch_stride, const float *d_g, uint64_t g_stride,
                             uint64_t g_ch_stride, uint64_t g_batch_stride, float *d_out);
int bhw_beam_mfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                                 uint32_t flags, const float *d_x, uint32_t n_ch, uint64_t x_ch_stride, const float *d_g, uint64_t g_stride,
                                 uint64_t g_ch_stride, uint64_t g_batch_stride, float *d_out);
int bhw_describe_beam_mfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                           uint32_t n_ch, uint64_t x_ch_stride, uint64_t g_stride, uint64_t g_ch_stride, uint64_t g_batch_stride, char *buf,
                           uint64_t len);

/* Threading: every entry point may be called from any host thread.  Calls that use the library-owned scratch of one
 * (device, stream) are serialised against each other for the duration of their launches (the table is rebuilt per call);
 * callers that pass their own bhw_exec.workspace must not share one workspace between concurrent calls.  The calling
 * thread's current HIP device is restored before every entry point returns, and no entry point reads or clears the
 * thread's hipGetLastError() state.
 *
 * Releases the library-owned per-device scratch, including the buffers of graphs captured with it: a graph captured with
 * library scratch on `device` must not be replayed after this call. */
int bhw_release_device(int device);

#ifdef __cplusplus
}
#endif
#endif /* BHW_H */
