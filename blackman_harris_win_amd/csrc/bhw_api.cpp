// bhw_api.cpp -- the device side of the C ABI (include/bhw.h): per-device scratch, table-format verification on the device,
// launches.  Everything that is decided from parameters alone -- validation, resolution of a (model, widths) tuple into kernel
// constants, strategy / format / shape choice, ownership segments, scratch sizing, bhw_describe_plan -- lives in the HIP-free
// bhw_plan.cpp (sanitised on the CPU build).  No per-sample arithmetic happens on the host: every compute entry point fails
// with BHW_ERR_HIP when no device is usable.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "bhw_plan.h"

extern "C" void bhw_taylor_rom(uint32_t dat_width, uint32_t lut_size, int32_t *rom_sin_cos);
extern "C" uint32_t bhw_taylor_pi_word(int e);

namespace {

#define fail bhwp_fail

int fail_hip(int hip_code, const char *what)
{
    return fail(BHW_ERR_HIP, "%s: %s (hipError %d)", what, hipGetErrorString((hipError_t)hip_code), hip_code);
}

bool device_ok(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return false;
    return device >= 0 && device < n;
}

// The calling thread's current device is switched for the duration of an entry point and put back afterwards.  status() is the
// entry point's prologue: BHW_ERR_HIP, with bhw_last_error() set, when `device` cannot be made current or -- with `check_device` --
// is no usable device at all (nothing is switched then).  The hooks that report neither do not ask.
struct DeviceGuard {
    int device, prev = -1;
    bool usable, switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev, bool check_device = true) : device(dev), usable(!check_device || device_ok(dev))
    {
        if (!usable) return;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) {
            err = hipSetDevice(device);
            switched = (err == hipSuccess);
        }
    }
    ~DeviceGuard()
    {
        if (switched && prev >= 0) (void)hipSetDevice(prev);
    }
    int status() const
    {
        if (!usable) return fail(BHW_ERR_HIP, "no usable HIP device %d (this library has no CPU path)", device);
        return err != hipSuccess ? fail_hip(err, "hipSetDevice") : BHW_OK;
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

bool stream_is_capturing(void *stream)
{
    if (!stream) return false;                               // the legacy default stream cannot be captured
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &st) != hipSuccess) return false;
    return st != hipStreamCaptureStatusNone;
}

// ---- library-owned scratch, one buffer per (device, stream) ------------------------------------
// The table is rebuilt by every call, so two calls that share a buffer must not interleave their launches
// (A.build, B.build, A.combine would combine A from B's table).  Calls on different streams get different
// buffers; calls on one (device, stream) -- from any number of host threads, the *_to_host helpers on the
// NULL stream included -- hold the slot's mutex from before the build launch until after the last launch,
// and the stream then orders the kernels.  Growing a buffer happens under the same mutex; a buffer only grows.
// Callers that want no allocation in the launch path (graph capture) pass their own workspace through
// bhw_exec, or call bhw_prepare_device first.
struct Slot {
    std::mutex mu;
    void *buf = nullptr;
    uint64_t bytes = 0;
    bool captured = false;              // buf was handed to a capturing stream: a graph may hold its address
    std::vector<void *> retired;        // captured buffers the slot has grown out of, freed by bhw_release_device
    uint64_t retired_bytes = 0;
};
struct DeviceScratch {
    std::map<void *, std::shared_ptr<Slot>> bufs;            // stream -> slot
    std::map<std::pair<uint32_t, uint32_t>, int32_t *> roms;  // Taylor ROM cache keyed by (W, L)
};
std::mutex g_mu;                                              // guards g_scratch's maps (never held across a launch)
std::map<int, DeviceScratch> g_scratch;

std::shared_ptr<Slot> slot_of(int device, void *stream)
{
    std::lock_guard<std::mutex> lk(g_mu);
    auto &sp = g_scratch[device].bufs[stream];
    if (!sp) sp = std::make_shared<Slot>();
    return sp;
}

// slot.mu is held by the caller; the current device is `device`
int ensure_slot_bytes(Slot &slot, void *stream, uint64_t bytes)
{
    if (slot.bytes >= bytes) return BHW_OK;
    if (stream_is_capturing(stream))
        return fail(BHW_ERR_HIP, "library scratch of this stream must grow to %llu bytes during stream capture: call "
                    "bhw_prepare_device first or pass bhw_exec.workspace", (unsigned long long)bytes);
    if (slot.buf && slot.captured) {                          // a graph may still replay with it: kept until bhw_release_device
        slot.retired.push_back(slot.buf);
        slot.retired_bytes += slot.bytes;
    } else if (slot.buf) {
        (void)hipStreamSynchronize((hipStream_t)stream);      // earlier launches on this stream may still read it
        (void)hipFree(slot.buf);
    }
    slot.buf = nullptr;
    slot.bytes = 0;
    slot.captured = false;
    void *b = nullptr;
    const hipError_t e = hipMalloc(&b, bytes);
    if (e != hipSuccess) return fail_hip(e, "hipMalloc(scratch)");
    slot.buf = b;
    slot.bytes = bytes;
    return BHW_OK;
}

int get_taylor_rom(int device, void *stream, uint32_t W, uint32_t L, const int32_t **rom)
{
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceScratch &s = g_scratch[device];
    auto key = std::make_pair(W, L);
    auto it = s.roms.find(key);
    if (it != s.roms.end()) { *rom = it->second; return BHW_OK; }
    if (stream_is_capturing(stream))
        return fail(BHW_ERR_HIP, "the Taylor ROM for dat_width %u / lut_size %u is not on the device yet and the stream is "
                    "capturing: call bhw_prepare_device first", W, L);
    std::vector<int32_t> host(2u << L);
    bhw_taylor_rom(W, L, host.data());
    int32_t *d = nullptr;
    hipError_t e = hipMalloc((void **)&d, host.size() * sizeof(int32_t));
    if (e != hipSuccess) return fail_hip(e, "hipMalloc(rom)");
    e = hipMemcpy(d, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice);   // synchronous: once per (device, W, L)
    if (e != hipSuccess) { (void)hipFree(d); return fail_hip(e, "hipMemcpy(rom)"); }
    s.roms[key] = d;
    *rom = d;
    return BHW_OK;
}

int resolve_taylor(const bhw_params *p, int device, void *stream, BhwTaylorCfg &t)
{
    memset(&t, 0, sizeof t);
    t.phi_width = p->phi_width;
    t.dat_width = p->dat_width;
    t.lut_size = p->lut_size;
    const int d = (int)p->phi_width - (int)p->lut_size;
    t.mode = d < 2 ? 0u : d == 2 ? 1u : 2u;
    t.xshift = 19 + p->lut_size;
    t.pi_word = d > 2 ? bhw_taylor_pi_word(17 - (d - 3)) : 0;          // tay1_order.vhd:133, STAGE = PW-L-3
    t.pad[0] = (d - 1) > 2 ? bhw_taylor_pi_word(17 - (d - 4)) : 0;      // generator at PHASE_WIDTH-1 (harmonics 2, 6)
    t.pad[1] = (d - 2) > 2 ? bhw_taylor_pi_word(17 - (d - 5)) : 0;      // generator at PHASE_WIDTH-2 (harmonic 4)
    return get_taylor_rom(device, stream, p->dat_width, p->lut_size, &t.rom);
}

// Runs [n0, n0+count) as  head | whole periods | tail.  `ragged(w, off, len)` handles an arbitrary sub-range, `period(w, off)`
// one whole period starting at a multiple of N; each gets `w` with the fused apply's input (w.apply_x, if any) advanced to its
// piece.  Without the fused apply only the first period is computed and the others are store-only replicas; with it every
// period has its own x.
template <typename Ragged, typename Period>
int run_split(const BhwLaunch &l, const BhwWinCfg &w, uint64_t n0, uint64_t count, uint64_t N, int32_t *d_out, Ragged ragged, Period period)
{
    BhwWinCfg piece = w;
    auto at = [&](uint64_t off) -> const BhwWinCfg & {
        if (w.apply_x) piece.apply_x = w.apply_x + off;
        return piece;
    };
    const uint64_t head_len = (N - n0 % N) % N;
    int e;
    if (count < head_len + N) {
        e = ragged(at(0), 0, count);
        return e ? fail_hip(e, "launch") : BHW_OK;
    }
    const uint64_t head = head_len, periods = (count - head) / N, tail = count - head - periods * N;
    e = head ? ragged(at(0), 0, head) : 0;
    if (e) return fail_hip(e, "head launch");
    const uint64_t computed = w.apply_x ? periods : 1;
    for (uint64_t f = 0; f < computed; ++f) {
        e = period(at(head + f * N), head + f * N);
        if (e) return fail_hip(e, "whole-period launch");
    }
    if (!w.apply_x && periods > 1) {
        e = bhwk_replicate(l, d_out + head, N, (uint32_t)(periods - 1), d_out + head + N);
        if (e) return fail_hip(e, "replicate launch");
    }
    e = tail ? ragged(at(head + periods * N), head + periods * N, tail) : 0;
    return e ? fail_hip(e, "tail launch") : BHW_OK;
}

// Points `c` at a table in format `dlog` laid out in `buf` (bhwp_table_layout), with the overflow check off.
void point_table(BhwCordicCfg &c, uint32_t dlog, const void *buf)
{
    const BhwTableLayout lay = bhwp_table_layout(bhwp_table_entries(c), dlog);
    c.tab_dlog = dlog;
    c.tab_coarse = dlog ? (const void *)((const char *)buf + lay.coarse_off) : nullptr;
    c.tab_esc = lay.esc_off ? (const void *)((const char *)buf + lay.esc_off) : nullptr;
    c.esc_wg_log = lay.esc_wg_log;
    c.tab_check = nullptr;
}

// Builds the packed table `c` points at in `buf` with the kernels' overflow check on, reads the check word back into *flag
// (non-zero: the format overflowed) and synchronises.  Returns the raw HIP status; `stage` names the step that failed.
int checked_build(const BhwLaunch &l, BhwCordicCfg c, void *buf, uint32_t *flag, const char **stage = nullptr)
{
    c.tab_check = (uint32_t *)((char *)buf + bhwp_table_layout(bhwp_table_entries(c), c.tab_dlog).check_off);
    const char *what = "hipMemsetAsync(check word)";
    int e = hipMemsetAsync(c.tab_check, 0, 8, (hipStream_t)l.stream);
    if (!e) {
        what = "table build launch";
        e = bhwk_table_build(l, c, (int32_t *)buf);
    }
    if (!e) {
        what = "read-back of the table format check";
        e = hipMemcpyAsync(flag, c.tab_check, sizeof *flag, hipMemcpyDeviceToHost, (hipStream_t)l.stream);
    }
    if (!e) e = hipStreamSynchronize((hipStream_t)l.stream);
    if (e && stage) *stage = what;
    return e;
}

// Settles the verdicts of the walk's open formats, narrowest first, up to the first exact one: each is read again first (another
// call may have settled it since the walk), and each still unknown gets a build with the kernels' overflow check on -- into `spare`
// when it holds spare_bytes >= the format's layout, else into a temporary allocation.  It reads the check word back, so never
// during a capture (a capturing walk has no open formats), and it never sizes the library scratch.
int settle_formats(const bhw_params *p, const BhwLaunch &l, BhwCordicCfg c, const BhwFormatWalk &fw, void *spare, uint64_t spare_bytes)
{
    for (int i = 0; i < fw.n_open; ++i) {
        int verdict = bhwp_fmt_verdict(p, fw.open[i]);
        if (verdict == kFmtUnknown) {
            const uint64_t bytes = bhwp_table_layout(bhwp_table_entries(c), fw.open[i]).bytes;
            void *buf = spare;
            if (bytes > spare_bytes) {
                const hipError_t he = hipMalloc(&buf, bytes);
                if (he != hipSuccess) return fail_hip(he, "hipMalloc(trial table)");
            }
            point_table(c, fw.open[i], buf);
            uint32_t flag = 1;
            const char *stage = "";
            const int e = checked_build(l, c, buf, &flag, &stage);
            if (buf != spare) (void)hipFree(buf);
            if (e) return fail_hip(e, stage);
            verdict = flag ? kFmtBad : kFmtOk;
            bhwp_fmt_set_verdict(p, fw.open[i], verdict);
        }
        if (verdict == kFmtOk) break;
    }
    return BHW_OK;
}

// Scratch of a table-strategy call: the caller's workspace when it passed one, else the library-owned buffer of this stream
// (locked until every launch of the call is enqueued), holding at least `need` bytes.  A slot handed to a capturing stream is
// marked `captured`, so that growing it later retires the buffer instead of freeing it.
struct TableScratch {
    void *ws = nullptr;
    std::shared_ptr<Slot> slot;
    std::unique_lock<std::mutex> lock;
};
int acquire_scratch(const bhw_exec *ex, int device, void *stream, uint64_t need, bool capturing, TableScratch &t)
{
    if (ex && ex->workspace) {
        if (ex->workspace_bytes < need)
            return fail(BHW_ERR_WORKSPACE, "workspace %llu < %llu bytes", (unsigned long long)ex->workspace_bytes, (unsigned long long)need);
        t.ws = ex->workspace;
        return BHW_OK;
    }
    t.slot = slot_of(device, stream);
    t.lock = std::unique_lock<std::mutex>(t.slot->mu);
    const int rc = ensure_slot_bytes(*t.slot, stream, need);
    if (rc) return rc;
    if (capturing) t.slot->captured = true;
    t.ws = t.slot->buf;
    return BHW_OK;
}

// The table of a table-strategy call, rebuilt: the open formats settled first (the first call of a configuration without
// bhw_prepare_device; the trials use the call's workspace or the stream's current buffer where either holds them), then scratch
// for the one format kept (acquire_scratch; a slot stays locked in `scratch` until every launch of the call is enqueued), the
// table built into it, then ex->event_after_build recorded.  Whole-period tile tables are stored packed when the widths allow it
// (formats in bhw_device.h): "nibble" = 1 byte per entry, "residual" = 2 bytes + one int4 record per 2^d entries, else "delta16"
// = 4 bytes per entry + one int2 head per 64 entries, else the plain 8 bytes per entry.
int rebuild_table(const bhw_params *p, const BhwLaunch &l, BhwCordicCfg &c, bool tiled, const bhw_exec *ex, TableScratch &scratch)
{
    const uint32_t limit = bhwp_exec_table_format(ex);
    const bool capturing = stream_is_capturing(l.stream);
    BhwFormatWalk fw = bhwp_format_walk(p, c, tiled, limit, capturing);
    int rc;
    if (fw.n_open) {
        if (ex && ex->workspace) {
            rc = settle_formats(p, l, c, fw, ex->workspace, ex->workspace_bytes);
        } else {
            const std::shared_ptr<Slot> slot = slot_of(l.device, l.stream);
            std::lock_guard<std::mutex> lk(slot->mu);
            rc = settle_formats(p, l, c, fw, slot->buf, slot->bytes);
        }
        if (rc) return rc;
        fw = bhwp_format_walk(p, c, tiled, limit, false);
    }
    rc = acquire_scratch(ex, l.device, l.stream, fw.scratch_bytes, capturing, scratch);
    if (!rc) {
        point_table(c, fw.kept, scratch.ws);
        const int e = bhwk_table_build(l, c, (int32_t *)scratch.ws);
        if (e) rc = fail_hip(e, "table build launch");
    }
    if (rc || !ex || !ex->event_after_build) return rc;
    const hipError_t he = hipEventRecord((hipEvent_t)ex->event_after_build, (hipStream_t)l.stream);
    return he != hipSuccess ? fail_hip(he, "hipEventRecord(event_after_build)") : BHW_OK;
}

// A built table: the configuration pointing at it, and whether whole periods take the tile kernel.
struct TableView {
    const BhwCordicCfg &c;
    bool tiled;
    const int32_t *tab;
};
// ragged pieces over a built table: bhwk_table_combine (the rebuilt path) or bhwk_range_combine (resident tables)
using RaggedKernel = int (*)(const BhwLaunch &, const BhwCordicCfg &, const BhwWinCfg &, const int32_t *, uint64_t, uint64_t, int32_t *);

// [n0, n0 + count) over a built table: the tile kernel over an image subset (a contiguous range of whole eighths of one window --
// one device's contiguous shard of a window split over 2, 4 or 8), else head | whole periods | tail with the whole periods on the
// run-length kernel (dropped phase bits: consecutive coefficients repeat table entries) or the tile / fold kernel of the layout.
int table_pieces(const BhwLaunch &l, const TableView &t, const bhw_params *p, const BhwWinCfg &w, uint64_t n0, uint64_t count,
                 int32_t *d_out, RaggedKernel ragged)
{
    const BhwTableCall tc = bhwp_table_call(p, t.c, w, n0, count, w.apply_x != nullptr);
    if (tc.images) {
        const int e = bhwk_table_combine_tile_range(l, t.c, w, t.tab, d_out, 0, 0, tc.img_mask, tc.n0mod);
        return e ? fail_hip(e, "tile launch (image subset)") : BHW_OK;
    }
    auto piece = [&](const BhwWinCfg &wp, uint64_t off, uint64_t len) { return ragged(l, t.c, wp, t.tab, n0 + off, len, d_out + off); };
    auto period = [&](const BhwWinCfg &wp, uint64_t off) {
        if (bhwk_runlength_applicable(t.c, wp, d_out + off)) return bhwk_runlength_window(l, t.c, wp, t.tab, d_out + off);
        return t.tiled ? bhwk_table_combine_tile(l, t.c, wp, t.tab, d_out + off) : bhwk_table_combine_fold(l, t.c, wp, t.tab, d_out + off);
    };
    return run_split(l, w, n0, count, 1ull << p->phi_width, d_out, piece, period);
}

// the tiles [tile0, tile0 + tile_count) of an ownership part over a built table
int part_tiles(const BhwLaunch &l, const TableView &t, const BhwWinCfg &w, uint32_t tile0, uint32_t tile_count, int32_t *d_window)
{
    const int e = bhwk_table_combine_tile_range(l, t.c, w, t.tab, d_window, tile0, tile_count);
    return e ? fail_hip(e, "tile part launch") : BHW_OK;
}

int generate_impl(const bhw_params *p, int device, void *stream, uint64_t n0, uint64_t count, int32_t *d_out,
                  const bhw_exec *ex, const int32_t *apply_x = nullptr, uint32_t apply_shift = 0)
{
    int rc = bhwp_validate(p);
    if (rc) return rc;
    if (count && !d_out) return fail(BHW_ERR_BADARG, "d_out is NULL");
    rc = bhwp_check_exec(ex);
    if (rc) return rc;
    if (!count) return BHW_OK;
    if (count > (1ull << 34)) return fail(BHW_ERR_BADARG, "count %llu > 2^34 per call", (unsigned long long)count);
    DeviceGuard guard(device);
    if ((rc = guard.status())) return rc;
    BhwLaunch l{device, stream};
    BhwWinCfg w;
    bhwp_resolve_window(p, w);
    w.apply_x = apply_x;
    w.apply_shift = apply_shift;
    if (p->sin_type != BHW_SIN_CORDIC) {
        BhwTaylorCfg t;
        rc = resolve_taylor(p, device, stream, t);
        if (rc) return rc;
        auto ragged = [&](const BhwWinCfg &wp, uint64_t off, uint64_t len) { return bhwk_taylor_window(l, t, wp, n0 + off, len, d_out + off); };
        if (p->phi_width < 5) {
            int e = ragged(w, 0, count);
            return e ? fail_hip(e, "taylor window launch") : BHW_OK;
        }
        auto period = [&](const BhwWinCfg &wp, uint64_t off) { return bhwk_taylor_window_fold(l, t, wp, d_out + off); };
        return run_split(l, w, n0, count, 1ull << p->phi_width, d_out, ragged, period);
    }
    BhwCordicCfg c;
    bhwp_resolve_cordic(p, c);
    const uint32_t algo = bhwp_pick_algo(p, c, w, n0, count, ex ? ex->algo : (uint32_t)BHW_ALGO_AUTO);
    if (algo == BHW_ALGO_DIRECT) {
        int e = bhwk_direct(l, c, w, n0, count, d_out);
        return e ? fail_hip(e, "direct launch") : BHW_OK;
    }
    if (algo == BHW_ALGO_FUSED) {
        // head | whole periods | tail: each whole period is one launch of the fused kernel over the full ring, the ragged
        // ends take the direct kernel; nothing is allocated and no table exists
        const BhwFoldRun ring{0u, 1u << (p->phi_width - 3)};
        auto ragged = [&](const BhwWinCfg &wp, uint64_t off, uint64_t len) { return bhwk_direct(l, c, wp, n0 + off, len, d_out + off); };
        auto period = [&](const BhwWinCfg &wp, uint64_t off) { return bhwk_fold_direct(l, c, wp, &ring, 1, d_out + off); };
        return run_split(l, w, n0, count, 1ull << p->phi_width, d_out, ragged, period);
    }
    // the one table built here, then its pieces; the ragged ends take the general gather kernel
    const BhwTableCall tc = bhwp_table_call(p, c, w, n0, count, apply_x != nullptr);
    c.tab_split = (tc.tiled && c.z_shr == 0) ? 1u : 0u;
    TableScratch scratch;
    rc = rebuild_table(p, l, c, tc.tiled, ex, scratch);
    if (rc) return rc;
    return table_pieces(l, TableView{c, tc.tiled, (const int32_t *)scratch.ws}, p, w, n0, count, d_out, bhwk_table_combine);
}

} // namespace

extern "C" {

int bhw_generate_device(const bhw_params *p, int device, void *hip_stream, uint64_t n0, uint64_t count, int32_t *d_out)
{
    return generate_impl(p, device, hip_stream, n0, count, d_out, nullptr);
}

int bhw_generate_device_ex(const bhw_params *p, int device, void *hip_stream, uint64_t n0, uint64_t count,
                           int32_t *d_out, const bhw_exec *ex)
{
    return generate_impl(p, device, hip_stream, n0, count, d_out, ex);
}

int bhw_apply_device(const bhw_params *p, int device, void *hip_stream, uint64_t n0, uint64_t count,
                     const int32_t *d_x, int32_t *d_y, uint32_t shift)
{
    const int rc = bhwp_apply_checks(count, d_x, d_y, shift);
    return rc ? rc : generate_impl(p, device, hip_stream, n0, count, d_y, nullptr, d_x, shift);
}

int bhw_generate_batched_device(const bhw_params *p, int device, void *hip_stream, uint32_t frames, int32_t *d_out)
{
    int rc = bhwp_validate(p);
    if (rc) return rc;
    if (!frames) return BHW_OK;
    if (!d_out) return fail(BHW_ERR_BADARG, "d_out is NULL");
    const uint64_t N = 1ull << p->phi_width;
    if (frames > 1 && p->sin_type == BHW_SIN_CORDIC) {
        // a period the fused kernel takes, up to 2^19 coefficients: ONE launch computes it and writes every frame -- no second kernel
        // reading frame 0 back.  1024 x 2^16 (BASELINE configs[3]) 0.0430 -> 0.0408 ms; 0.0410 - 0.0419 against 0.0427 - 0.0439 for
        // periods of 2^14 .. 2^19; at 2^20 the rows' repeated computation is no longer hidden (0.0468 against 0.0441) and the old
        // path stays (profiles/r04_ab_batched_one_launch.txt)
        BhwCordicCfg c;
        bhwp_resolve_cordic(p, c);
        BhwWinCfg w;
        bhwp_resolve_window(p, w);
        if (p->phi_width <= 19 && bhwp_pick_algo(p, c, w, 0, N, BHW_ALGO_AUTO) == BHW_ALGO_FUSED && bhwp_fold_form(c, w, N >> 3) != BHWP_FOLD_SPLIT) {
            DeviceGuard guard(device);
            if ((rc = guard.status())) return rc;
            BhwLaunch l{device, hip_stream};
            const BhwFoldRun ring{0u, 1u << (p->phi_width - 3)};
            const int e = bhwk_fold_direct(l, c, w, &ring, 1, d_out, frames);
            return e ? fail_hip(e, "fused batched launch") : BHW_OK;
        }
    }
    // frame 0 is generated in place, then replicated into frames 1..frames-1
    rc = generate_impl(p, device, hip_stream, 0, N, d_out, nullptr);
    if (rc || frames == 1) return rc;
    DeviceGuard guard(device, false);
    if ((rc = guard.status())) return rc;
    BhwLaunch l{device, hip_stream};
    int e = bhwk_replicate(l, d_out, N, frames - 1, d_out + N);
    return e ? fail_hip(e, "replicate launch") : BHW_OK;
}

int bhw_sincos_device(const bhw_params *p, int device, void *hip_stream, uint64_t theta0, uint64_t count,
                      int32_t *d_sin, int32_t *d_cos)
{
    int rc = bhwp_validate(p, true);
    if (rc) return rc;
    if (!count) return BHW_OK;
    if (!d_sin && !d_cos) return fail(BHW_ERR_BADARG, "both outputs NULL");
    DeviceGuard guard(device);
    if ((rc = guard.status())) return rc;
    BhwLaunch l{device, hip_stream};
    if (p->sin_type != BHW_SIN_CORDIC) {
        BhwTaylorCfg t;
        rc = resolve_taylor(p, device, hip_stream, t);
        if (rc) return rc;
        int e = bhwk_taylor_sincos(l, t, theta0, count, d_sin, d_cos);
        return e ? fail_hip(e, "taylor sincos launch") : BHW_OK;
    }
    if (p->model > BHW_MODEL_VHDL) {
        BhwPrerotCfg c;
        bhwp_resolve_prerot(p, c);                                                  // cordic_dds48 / cordic_dds_scaled constants
        int e = bhwk_sincos_prerot(l, c, theta0, count, d_sin, d_cos);
        return e ? fail_hip(e, "sincos (pre-rotated) launch") : BHW_OK;
    }
    BhwCordicCfg c;
    bhwp_resolve_cordic(p, c);
    int e = bhwk_sincos(l, c, theta0, count, d_sin, d_cos);
    return e ? fail_hip(e, "sincos launch") : BHW_OK;
}

int bhw_generate_to_host(const bhw_params *p, int device, uint64_t n0, uint64_t count, int32_t *h_out)
{
    int rc = bhwp_validate(p);
    if (rc) return rc;
    if (!count) return BHW_OK;
    if (!h_out) return fail(BHW_ERR_BADARG, "h_out is NULL");
    DeviceGuard guard(device);
    if ((rc = guard.status())) return rc;
    int32_t *d = nullptr;
    hipError_t e = hipMalloc((void **)&d, count * sizeof(int32_t));
    if (e != hipSuccess) return fail_hip(e, "hipMalloc(out)");
    rc = generate_impl(p, device, nullptr, n0, count, d, nullptr);
    if (!rc) {
        e = hipMemcpy(h_out, d, count * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail_hip(e, "hipMemcpy(D2H)");
    }
    (void)hipFree(d);
    return rc;
}

int bhw_sincos_to_host(const bhw_params *p, int device, uint64_t theta0, uint64_t count, int32_t *h_sin, int32_t *h_cos)
{
    int rc = bhwp_validate(p, true);
    if (rc) return rc;
    if (!count) return BHW_OK;
    if (!h_sin && !h_cos) return fail(BHW_ERR_BADARG, "both outputs NULL");
    DeviceGuard guard(device);
    if ((rc = guard.status())) return rc;
    int32_t *d = nullptr;
    hipError_t e = hipMalloc((void **)&d, 2 * count * sizeof(int32_t));
    if (e != hipSuccess) return fail_hip(e, "hipMalloc(out)");
    rc = bhw_sincos_device(p, device, nullptr, theta0, count, d, d + count);
    if (!rc && h_sin) {
        e = hipMemcpy(h_sin, d, count * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail_hip(e, "hipMemcpy(D2H)");
    }
    if (!rc && h_cos) {
        e = hipMemcpy(h_cos, d + count, count * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail_hip(e, "hipMemcpy(D2H)");
    }
    (void)hipFree(d);
    return rc;
}

// Development hooks (not part of the ABI in include/bhw.h): the two passes of the table strategy on their own,
// for overlap experiments (tools/overlap_probe.py).  They use the narrowest table format already verified for the
// configuration (a bhw_generate_device call of the same parameters settles it: the walk's `kept`), plain otherwise.
static void dbg_verified_format(const bhw_params *p, BhwCordicCfg &c, bool tiled, const void *ws)
{
    point_table(c, bhwp_format_walk(p, c, tiled, BHW_TABLE_BEST, false).kept, ws);
}

int bhw_dbg_table_build(const bhw_params *p, int device, void *stream, void *ws)
{
    if (bhwp_validate(p)) return BHW_ERR_BADARG;
    BhwCordicCfg c;
    bhwp_resolve_cordic(p, c);
    BhwWinCfg w;
    bhwp_resolve_window(p, w);
    c.tab_split = (bhwk_tile_applicable(c, w) && c.z_shr == 0) ? 1u : 0u;
    dbg_verified_format(p, c, bhwk_tile_applicable(c, w), ws);
    DeviceGuard guard(device, false);
    BhwLaunch l{device, stream};
    return bhwk_table_build(l, c, (int32_t *)ws);
}

int bhw_dbg_table_combine(const bhw_params *p, int device, void *stream, const void *ws, int32_t *d_out)
{
    if (bhwp_validate(p)) return BHW_ERR_BADARG;
    BhwCordicCfg c;
    bhwp_resolve_cordic(p, c);
    BhwWinCfg w;
    bhwp_resolve_window(p, w);
    DeviceGuard guard(device, false);
    BhwLaunch l{device, stream};
    if (bhwk_tile_applicable(c, w)) {
        c.tab_split = c.z_shr == 0 ? 1u : 0u;
        dbg_verified_format(p, c, true, ws);
        return bhwk_table_combine_tile(l, c, w, (const int32_t *)ws, d_out);
    }
    return bhwk_table_combine_fold(l, c, w, (const int32_t *)ws, d_out);
}

// Builds the table of `p` in the packed format `dlog` (6 delta16, 7..9 residual, 23..25 nibble) with the overflow check on, whether or not
// the format would be chosen for this configuration, and returns the check word.  `ws`: bhw_workspace_bytes(TABLE) bytes.
int bhw_dbg_check_table_format(const bhw_params *p, int device, void *stream, uint32_t dlog, void *ws, uint32_t *flag_out)
{
    if (bhwp_validate(p) || !ws || !flag_out || dlog < 6 || (dlog > 9 && (dlog < 16u + 7u || dlog > 16u + 9u) && (dlog < 48u + 7u || dlog > 48u + 9u))) return BHW_ERR_BADARG;
    BhwCordicCfg c;
    bhwp_resolve_cordic(p, c);
    if (c.z_shr != 0 || c.n_iter < 21 || c.dat_width + c.out_shr > 34 || bhwp_table_entries(c) < (1ull << 20)) return BHW_ERR_UNSUPPORTED;   // packed tables exist for tiled windows (PW >= 22) only
    DeviceGuard guard(device, false);
    c.tab_split = 1u;
    point_table(c, dlog, ws);
    return checked_build(BhwLaunch{device, stream}, c, ws, flag_out) ? BHW_ERR_HIP : BHW_OK;
}

int bhw_atan2_device(const bhw_atan2_params *p, int device, void *hip_stream, uint64_t count,
                     const int32_t *d_x, const int32_t *d_y, int32_t *d_phi)
{
    int rc = bhwp_validate_atan2(p);
    if (rc) return rc;
    if (!count) return BHW_OK;
    if (!d_x || !d_y || !d_phi) return fail(BHW_ERR_BADARG, "d_x / d_y / d_phi is NULL");
    DeviceGuard guard(device);
    if ((rc = guard.status())) return rc;
    BhwAtan2Cfg c;
    bhwp_resolve_atan2(p, c);
    BhwLaunch l{device, hip_stream};
    int e = bhwk_atan2(l, c, count, d_x, d_y, d_phi);
    return e ? fail_hip(e, "atan2 launch") : BHW_OK;
}

int bhw_atan2_to_host(const bhw_atan2_params *p, int device, uint64_t count, const int32_t *h_x, const int32_t *h_y, int32_t *h_phi)
{
    int rc = bhwp_validate_atan2(p);
    if (rc) return rc;
    if (!count) return BHW_OK;
    if (!h_x || !h_y || !h_phi) return fail(BHW_ERR_BADARG, "h_x / h_y / h_phi is NULL");
    DeviceGuard guard(device);
    if ((rc = guard.status())) return rc;
    int32_t *d = nullptr;
    hipError_t e = hipMalloc((void **)&d, 3 * count * sizeof(int32_t));
    if (e != hipSuccess) return fail_hip(e, "hipMalloc(atan2)");
    e = hipMemcpy(d, h_x, count * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + count, h_y, count * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = fail_hip(e, "hipMemcpy(H2D)");
    if (!rc) rc = bhw_atan2_device(p, device, nullptr, count, d, d + count, d + 2 * count);
    if (!rc) {
        e = hipMemcpy(h_phi, d + 2 * count, count * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail_hip(e, "hipMemcpy(D2H)");
    }
    (void)hipFree(d);
    return rc;
}

// ---- interleaved ownership parts (include/bhw.h; bhw_part_segments and the ownership arithmetic: bhw_plan.cpp) ----------------------
int bhw_generate_part_device(const bhw_params *p, int device, void *hip_stream, uint32_t part, uint32_t n_parts,
                             int32_t *d_window, const bhw_exec *ex)
{
    int rc = bhwp_part_checks(p, part, n_parts);
    if (rc) return rc;
    if (!d_window) return fail(BHW_ERR_BADARG, "d_window is NULL");
    rc = bhwp_check_exec(ex);
    if (rc) return rc;
    DeviceGuard guard(device);
    if ((rc = guard.status())) return rc;
    BhwLaunch l{device, hip_stream};
    BhwCordicCfg c;
    bhwp_resolve_cordic(p, c);
    BhwWinCfg w;
    bhwp_resolve_window(p, w);
    BhwFoldRun runs[32];
    uint32_t tile0 = 0, tile_count = 0;
    const int n_runs = bhwk_part_runs(c, w, part, n_parts, runs, &tile0, &tile_count);
    if (n_runs == 0) return BHW_OK;
    const bool fused = bhwp_part_fused(p, c, runs, n_runs, tile_count, ex ? ex->algo : (uint32_t)BHW_ALGO_AUTO, &rc);
    if (rc) return rc;
    if (fused) {
        const int e = bhwk_fold_direct(l, c, w, runs, (uint32_t)n_runs, d_window);
        return e ? fail_hip(e, "fused part launch") : BHW_OK;
    }
    c.tab_split = c.z_shr == 0 ? 1u : 0u;
    TableScratch scratch;
    rc = rebuild_table(p, l, c, true, ex, scratch);
    return rc ? rc : part_tiles(l, TableView{c, true, (const int32_t *)scratch.ws}, w, tile0, tile_count, d_window);
}

int bhw_gather_parts_device(const bhw_params *p, uint32_t n_parts, const int *src_devices, const int32_t *const *d_windows,
                            int dst_device, void *dst_stream, int32_t *d_dst)
{
    int rc = bhwp_part_checks(p, 0, n_parts);
    if (rc) return rc;
    if (!src_devices || !d_windows || !d_dst) return fail(BHW_ERR_BADARG, "src_devices / d_windows / d_dst is NULL");
    DeviceGuard guard(dst_device);
    if (!guard.usable) return guard.status();
    for (uint32_t g = 0; g < n_parts; ++g) {
        if (!d_windows[g]) return fail(BHW_ERR_BADARG, "d_windows[%u] is NULL", g);
        if (!device_ok(src_devices[g])) return fail(BHW_ERR_HIP, "no usable HIP device %d", src_devices[g]);
    }
    if ((rc = guard.status())) return rc;
    std::vector<bhw_segment> segs(256);
    for (uint32_t g = 0; g < n_parts; ++g) {
        if (d_windows[g] == d_dst) continue;                      // this part was generated in place
        uint32_t n = 0;
        rc = bhw_part_segments(p, g, n_parts, segs.data(), (uint32_t)segs.size(), &n);
        if (rc) return rc;
        for (uint32_t i = 0; i < n; ++i) {
            const hipError_t e = hipMemcpyPeerAsync(d_dst + segs[i].n0, dst_device, d_windows[g] + segs[i].n0, src_devices[g],
                                                    segs[i].count * sizeof(int32_t), (hipStream_t)dst_stream);
            if (e != hipSuccess) return fail_hip(e, "hipMemcpyPeerAsync(segment)");
        }
    }
    return BHW_OK;
}

int bhw_release_device(int device)
{
    DeviceScratch taken;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_scratch.find(device);
        if (it == g_scratch.end()) return BHW_OK;
        taken = std::move(it->second);
        g_scratch.erase(it);
    }
    DeviceGuard guard(device, false);
    if (guard.err == hipSuccess) {
        (void)hipDeviceSynchronize();
        for (auto &kv : taken.bufs) {
            std::lock_guard<std::mutex> lk(kv.second->mu);   // a call still enqueueing on this slot finishes first
            if (kv.second->buf) (void)hipFree(kv.second->buf);
            for (void *b : kv.second->retired) (void)hipFree(b);
            kv.second->buf = nullptr;
            kv.second->bytes = 0;
            kv.second->retired.clear();
            kv.second->retired_bytes = 0;
        }
        for (auto &kv : taken.roms) (void)hipFree(kv.second);
    }
    return BHW_OK;
}

int bhw_prepare_device(const bhw_params *p, int device, void *hip_stream)
{
    int rc = bhwp_validate(p, true);
    if (rc) return rc;
    DeviceGuard guard(device);
    if ((rc = guard.status())) return rc;
    if (p->sin_type != BHW_SIN_CORDIC) {
        BhwTaylorCfg t;
        return resolve_taylor(p, device, hip_stream, t);        // uploads the ROM on first use
    }
    if (p->model > BHW_MODEL_VHDL) return BHW_OK;               // variant generators: nothing lazy
    BhwCordicCfg c;
    bhwp_resolve_cordic(p, c);
    BhwWinCfg w;
    bhwp_resolve_window(p, w);
    // Settle the packed-format verdict of EVERY format a later call may name: the chain table_format BEST walks, and each explicit
    // limit -- a captured call with an explicit bhw_exec.table_format must not meet an open verdict (it would fall back to the plain
    // table, which the scratch may not hold).  Then reserve the scratch every later table-strategy call with these widths can need
    // -- also for configurations AUTO sends to the fused kernel as whole periods: a partial range of such a window, or an explicit
    // BHW_ALGO_TABLE, still builds a table, and must not allocate inside a stream capture.  Two shapes: the settled format of
    // whole-period tile calls (16.5 MiB instead of 128 MiB for a 2^26-point window at 32 bits) and the plain table of ranges without
    // a whole period (8 bytes per entry; reserved up to 64 MiB -- beyond that a ragged call after prepare may still grow the scratch
    // once, outside a capture).  The slot only grows: what an earlier prepared configuration needs stays.
    const bool tile = bhwk_tile_applicable(c, w);
    const uint64_t plain = bhwp_table_layout(bhwp_table_entries(c), 0).bytes;
    uint64_t keep = plain <= (64ull << 20) || !tile ? plain : 0;
    auto slot = slot_of(device, hip_stream);
    std::unique_lock<std::mutex> lk(slot->mu);
    if (tile) {
        c.tab_split = c.z_shr == 0 ? 1u : 0u;
        if (!stream_is_capturing(hip_stream)) {
            for (uint32_t limit : {BHW_TABLE_BEST, BHW_TABLE_NIBBLE_ESC, BHW_TABLE_RESIDUAL, BHW_TABLE_DELTA16}) {
                rc = settle_formats(p, BhwLaunch{device, hip_stream}, c, bhwp_format_walk(p, c, true, limit, false), slot->buf, slot->bytes);
                if (rc) return rc;
            }
        }
        const uint64_t settled = bhwp_format_walk(p, c, true, BHW_TABLE_BEST, false).scratch_bytes;
        if (settled > keep) keep = settled;
    }
    rc = ensure_slot_bytes(*slot, hip_stream, keep);
    if (rc) return rc;
    const hipError_t he = hipStreamSynchronize((hipStream_t)hip_stream);
    return he != hipSuccess ? fail_hip(he, "hipStreamSynchronize") : BHW_OK;
}

// ---- resident tables (include/bhw.h: bhw_table_create ...) -------------------------------------------------------------------------
// One first-quadrant table of a configuration's CORDIC generics in one device allocation, immutable after create.  The calls that
// read it take no lock, allocate nothing, neither synchronise nor read anything back and never touch the library scratch, so they
// can be captured into a graph on any stream.  Decisions from parameters alone (key match, layout, format candidates, the kernel of
// each piece) are bhw_plan.cpp's.

} // extern "C"

struct bhw_table_s {
    int device;
    bhw_params key;        // the generics the table was built from (only model / widths / precision matter)
    BhwCordicCfg c;        // resolved, with the format and the pointers of the table's records / escape lists set
    bool tiled;            // whole periods take the tile kernel (split packed layout at z_shr == 0)
    void *buf;
    uint64_t bytes;
    TableView view() const { return TableView{c, tiled, (const int32_t *)buf}; }
};

namespace {

// the prologue of every from-table call: the handle, `p` validated and matched to the table's generics
int table_call_checks(bhw_table t, const bhw_params *p)
{
    if (!t) return fail(BHW_ERR_BADARG, "table is NULL");
    const int rc = bhwp_validate(p);
    return rc ? rc : bhwp_table_key_check(&t->key, p);
}

// head | whole periods | tail as generate_impl splits a table-strategy call, every piece over the one resident table
int from_table(bhw_table t, const bhw_params *p, void *stream, uint64_t n0, uint64_t count, int32_t *d_out,
               const int32_t *apply_x = nullptr, uint32_t apply_shift = 0, RaggedKernel ragged = bhwk_range_combine)
{
    int rc = table_call_checks(t, p);
    if (rc) return rc;
    if (count && !d_out) return fail(BHW_ERR_BADARG, "d_out is NULL");
    if (!count) return BHW_OK;
    if (count > (1ull << 34)) return fail(BHW_ERR_BADARG, "count %llu > 2^34 per call", (unsigned long long)count);
    DeviceGuard guard(t->device, false);
    if ((rc = guard.status())) return rc;
    BhwWinCfg w;
    bhwp_resolve_window(p, w);
    w.apply_x = apply_x;
    w.apply_shift = apply_shift;
    return table_pieces(BhwLaunch{t->device, stream}, t->view(), p, w, n0, count, d_out, ragged);
}

// The launch of a frames / overlap-add / any-length generate call that passed its checks, from table t (on its device) or, with t
// NULL, by the direct CORDIC chains of p on `device` (checked to be a usable device).  length 0: L = 2^phi_width, no phase map.
// launch(l, c, w, d_table, lp) returns the HIP status, reported as `what`.
template <typename Launch>
int run_source(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const char *what, Launch launch)
{
    const int dev = t ? t->device : device;
    DeviceGuard guard(dev, !t);
    if (const int rc = guard.status()) return rc;
    BhwCordicCfg c;
    if (t) c = t->c;
    else   bhwp_resolve_cordic(p, c);
    BhwWinCfg w;
    bhwp_resolve_window(p, w);
    const BhwLenPhase lp = length ? bhw_len_phase(p->phi_width, length) : BhwLenPhase{};
    const int e = launch(BhwLaunch{dev, stream}, c, w, t ? (const int32_t *)t->buf : nullptr, length ? &lp : nullptr);
    return e ? fail_hip(e, what) : BHW_OK;
}

// Every overlapped-frame apply: the frames kernel from table t or by the direct CORDIC chains (t NULL), over the window of length
// `length` (0: 2^phi_width), or one bhw_apply_device per frame where the planner's route rule says so (library calls at
// L = 2^phi_width).  force_route >= 0: the route of an A/B run (bhw_dbg_apply_frames_route).
int frames_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_frames *f, const int32_t *d_x,
               int32_t *d_y, int force_route = -1)
{
    int rc = t ? table_call_checks(t, p) : BHW_OK;
    if (!rc) rc = bhwp_frames_checks(p, f, d_x, d_y, true, length);
    if (rc || !f->frames) return rc;
    const BhwFramesPlan pl = bhwp_frames_plan(p, f, t != nullptr, force_route, length);
    if (pl.route == BHWP_FRAMES_PER_FRAME) {
        for (uint64_t i = 0; i < f->frames; ++i)
            if ((rc = generate_impl(p, device, stream, 0, pl.len, d_y + i * pl.y_stride, nullptr, d_x + i * f->hop, f->shift))) return rc;
        return BHW_OK;
    }
    const char *what = length ? "frames launch (any length)" : t ? "frames launch (resident table)" : "frames launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                               const BhwLenPhase *lp) { return bhwk_frames(l, c, w, pl, f, d_x, d_y, tab, lp); });
}

// Every weighted overlap-add, as frames_run.  force_q / force_rx > 0: the plan shape of a test or A/B run (bhw_dbg_overlap_add_shape).
int ola_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_ola *o, const int32_t *d_y, int32_t *d_x,
            uint32_t force_q = 0, uint32_t force_rx = 0)
{
    int rc = t ? table_call_checks(t, p) : BHW_OK;
    if (!rc) rc = bhwp_ola_checks(p, o, d_y, d_x, true, length);
    if (rc || !o->count) return rc;
    const BhwOlaPlan pl = bhwp_ola_plan(p, o, t != nullptr, force_q, force_rx, length);
    const char *what = length ? "overlap-add launch (any length)" : t ? "overlap-add launch (resident table)" : "overlap-add launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                               const BhwLenPhase *lp) { return bhwk_ola(l, c, w, pl, o, d_y, d_x, tab, lp); });
}

} // namespace

extern "C" {

int bhw_table_create(const bhw_params *p, int device, void *hip_stream, uint32_t table_format, bhw_table *out)
{
    if (!out) return fail(BHW_ERR_BADARG, "out is NULL");
    *out = nullptr;
    int rc = bhwp_table_create_checks(p, table_format);
    if (rc) return rc;
    DeviceGuard guard(device);
    if ((rc = guard.status())) return rc;
    const BhwLaunch l{device, hip_stream};
    BhwCordicCfg c;
    bool tiled;
    bhwp_resident_layout(p, c, &tiled);
    // the narrowest format under `table_format` that is exact for the configuration: the walk's open verdicts settled by trial
    // builds into temporary buffers, then the walk's `kept`
    rc = settle_formats(p, l, c, bhwp_format_walk(p, c, tiled, table_format, false), nullptr, 0);
    if (rc) return rc;
    const uint32_t keep = bhwp_format_walk(p, c, tiled, table_format, false).kept;
    const uint64_t bytes = bhwp_table_layout(bhwp_table_entries(c), keep).bytes;
    void *buf = nullptr;
    hipError_t he = hipMalloc(&buf, bytes);
    if (he != hipSuccess) return fail_hip(he, "hipMalloc(resident table)");
    point_table(c, keep, buf);
    int e = bhwk_table_build(l, c, (int32_t *)buf);
    if (!e) e = hipStreamSynchronize((hipStream_t)hip_stream);
    if (e) {
        (void)hipFree(buf);
        return fail_hip(e, "resident table build");
    }
    bhw_table t = new (std::nothrow) bhw_table_s{device, *p, c, tiled, buf, bytes};
    if (!t) {
        (void)hipFree(buf);
        return fail(BHW_ERR_HIP, "out of host memory");
    }
    *out = t;
    return BHW_OK;
}

int bhw_table_destroy(bhw_table t)
{
    if (!t) return BHW_OK;
    {
        DeviceGuard guard(t->device, false);
        if (guard.err == hipSuccess) {
            (void)hipDeviceSynchronize();                               // launches still reading it finish first
            (void)hipFree(t->buf);
        }
    }
    delete t;
    return BHW_OK;
}

uint64_t bhw_table_bytes(bhw_table t) { return t ? t->bytes : 0; }

int bhw_table_describe(bhw_table t, const bhw_params *p, uint64_t n0, uint64_t count, char *buf, uint64_t len)
{
    const int rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_from_table(p, t->c, t->tiled, n0, count, buf, len);
}

int bhw_generate_from_table(bhw_table t, const bhw_params *p, void *hip_stream, uint64_t n0, uint64_t count, int32_t *d_out)
{
    return from_table(t, p, hip_stream, n0, count, d_out);
}

int bhw_apply_from_table(bhw_table t, const bhw_params *p, void *hip_stream, uint64_t n0, uint64_t count,
                         const int32_t *d_x, int32_t *d_y, uint32_t shift)
{
    const int rc = bhwp_apply_checks(count, d_x, d_y, shift);
    return rc ? rc : from_table(t, p, hip_stream, n0, count, d_y, d_x, shift);
}

int bhw_generate_part_from_table(bhw_table t, const bhw_params *p, void *hip_stream, uint32_t part, uint32_t n_parts, int32_t *d_window)
{
    if (!t) return fail(BHW_ERR_BADARG, "table is NULL");
    int rc = bhwp_part_checks(p, part, n_parts);
    if (!rc) rc = bhwp_table_key_check(&t->key, p);
    if (rc) return rc;
    if (!d_window) return fail(BHW_ERR_BADARG, "d_window is NULL");
    if (!t->tiled)
        return fail(BHW_ERR_UNSUPPORTED, "parts from a table need the tile layout (phi_width >= 22); shorter windows' parts are the fused kernel's");
    BhwWinCfg w;
    bhwp_resolve_window(p, w);
    BhwFoldRun runs[32];
    uint32_t tile0 = 0, tile_count = 0;
    if (bhwk_part_runs(t->c, w, part, n_parts, runs, &tile0, &tile_count) == 0 || tile_count == 0) return BHW_OK;
    DeviceGuard guard(t->device, false);
    if ((rc = guard.status())) return rc;
    return part_tiles(BhwLaunch{t->device, hip_stream}, t->view(), w, tile0, tile_count, d_window);
}

int bhw_apply_frames_device(const bhw_params *p, int device, void *hip_stream, const bhw_frames *f, const int32_t *d_x, int32_t *d_y)
{
    return frames_run(nullptr, p, 0, device, hip_stream, f, d_x, d_y);
}

// Development hook (not part of the ABI in include/bhw.h): bhw_apply_frames_device on a forced route (BHWP_FRAMES_DIRECT or
// BHWP_FRAMES_PER_FRAME; a route the call cannot take is ignored) -- the crossover runs of tools/bench_apply_frames.py and tests.
int bhw_dbg_apply_frames_route(const bhw_params *p, int device, void *hip_stream, const bhw_frames *f, const int32_t *d_x, int32_t *d_y,
                               int route)
{
    return frames_run(nullptr, p, 0, device, hip_stream, f, d_x, d_y, route);
}

int bhw_apply_frames_from_table(bhw_table t, const bhw_params *p, void *hip_stream, const bhw_frames *f, const int32_t *d_x, int32_t *d_y)
{
    return t ? frames_run(t, p, 0, t->device, hip_stream, f, d_x, d_y) : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_apply_frames_describe(bhw_table t, const bhw_params *p, const bhw_frames *f, char *buf, uint64_t len)
{
    int rc = t ? table_call_checks(t, p) : BHW_OK;
    if (!rc) rc = bhwp_frames_checks(p, f, nullptr, nullptr, false);
    return rc ? rc : bhwp_describe_frames(p, t ? &t->c : nullptr, f, buf, len);
}

int bhw_overlap_add_describe(bhw_table t, const bhw_params *p, const bhw_ola *o, char *buf, uint64_t len)
{
    int rc = t ? table_call_checks(t, p) : BHW_OK;
    if (!rc) rc = bhwp_ola_checks(p, o, nullptr, nullptr, false);
    return rc ? rc : bhwp_describe_ola(p, t ? &t->c : nullptr, o, buf, len);
}

// Development hook (not part of the ABI in include/bhw.h): the overlap-add with a forced plan shape -- Q (1..16) and the lanes along
// the residue rx (a power of two <= 256; 0 = the planner's) -- from table t, or with the direct source when t is NULL (on `device`).
// The tests compare the shapes' outputs; tools/bench_overlap_add.py times them.
int bhw_dbg_overlap_add_shape(bhw_table t, const bhw_params *p, int device, void *hip_stream, const bhw_ola *o, const int32_t *d_y,
                              int32_t *d_x, uint32_t force_q, uint32_t force_rx)
{
    return ola_run(t, p, 0, device, hip_stream, o, d_y, d_x, force_q, force_rx);
}

int bhw_overlap_add_device(const bhw_params *p, int device, void *hip_stream, const bhw_ola *o, const int32_t *d_y, int32_t *d_x)
{
    return ola_run(nullptr, p, 0, device, hip_stream, o, d_y, d_x);
}

int bhw_overlap_add_from_table(bhw_table t, const bhw_params *p, void *hip_stream, const bhw_ola *o, const int32_t *d_y, int32_t *d_x)
{
    return t ? ola_run(t, p, 0, t->device, hip_stream, o, d_y, d_x) : fail(BHW_ERR_BADARG, "table is NULL");
}

// Development hook (not part of the ABI in include/bhw.h): bhw_generate_from_table with every ragged piece on the general gather
// kernel k_table_combine (format read at run time) instead of k_range_combine -- the A/B of tools/bench_resident_table.py.
int bhw_dbg_generate_from_table_generic(bhw_table t, const bhw_params *p, void *hip_stream, uint64_t n0, uint64_t count, int32_t *d_out)
{
    return from_table(t, p, hip_stream, n0, count, d_out, nullptr, 0, bhwk_table_combine);
}

// the live (or, with `retired`, the retired) bytes of the library-owned scratch of (device, stream); 0 where it has none
static uint64_t slot_bytes(int device, void *stream, bool retired)
{
    std::shared_ptr<Slot> sp;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_scratch.find(device);
        if (it == g_scratch.end()) return 0;
        auto jt = it->second.bufs.find(stream);
        if (jt == it->second.bufs.end()) return 0;
        sp = jt->second;
    }
    std::lock_guard<std::mutex> lk(sp->mu);
    return retired ? sp->retired_bytes : sp->bytes;
}

// Bytes the library-owned scratch of (device, hip_stream) holds right now (0: none yet) -- what bench.py reports beside the size of
// the workspace it passes itself -- and the bytes of the captured buffers it has grown out of (kept until bhw_release_device).  Not
// part of the ABI in include/bhw.h.
uint64_t bhw_dbg_library_scratch_bytes(int device, void *hip_stream) { return slot_bytes(device, hip_stream, false); }
uint64_t bhw_dbg_library_retired_bytes(int device, void *hip_stream) { return slot_bytes(device, hip_stream, true); }

} // extern "C"

// ---- windows of any length (include/bhw.h: bhw_generate_len_device ...) -------------------------------------------------------------
// At L = 2^phi_width every call takes the existing entry point of its kind, unchanged; otherwise the any-length kernels (bhw_len.hip,
// k_frames_*_len, k_ola_*_len), which allocate nothing and use no scratch.  bhw_dbg_len_force_kernels sends L = 2^phi_width to the
// any-length kernels too (the identity tests).

namespace {

std::atomic<bool> g_len_force{false};

// the length a run function takes after bhwp_len_checks: L on the any-length kernels, 0 on the power-of-two route
uint64_t len_route(const bhw_params *p, uint64_t length) { return bhwp_len_kernels(p, length, g_len_force) ? length : 0; }

// generate [n0, n0 + count) of the window of length L on the any-length kernels, from table t or by the direct chains (t NULL)
int generate_len(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, uint64_t n0, uint64_t count, int32_t *d_out)
{
    int rc = t ? table_call_checks(t, p) : BHW_OK;
    if (rc) return rc;
    if (count && !d_out) return fail(BHW_ERR_BADARG, "d_out is NULL");
    if (count > (1ull << 34)) return fail(BHW_ERR_BADARG, "count %llu > 2^34 per call", (unsigned long long)count);
    if (!count) return BHW_OK;
    const char *what = t ? "generate launch (any length, resident table)" : "generate launch (any length)";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                               const BhwLenPhase *lp) { return bhwk_len_range(l, c, w, tab, *lp, n0, count, d_out); });
}

// Every float32 frame apply, from table t (checked non-NULL by the caller) or by the direct CORDIC chains (t NULL): the checks, then
// the float32 frames kernel (no per-frame route).
int frames_f32_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_frames *f, const float *d_x,
                   float *d_y)
{
    int rc = bhwp_f32_checks(p, length, 0);
    if (!rc && t) rc = table_call_checks(t, p);
    if (!rc) rc = bhwp_frames_checks(p, f, d_x, d_y, true, length);
    if (rc || !f->frames) return rc;
    const uint64_t L = len_route(p, length);
    const BhwFramesPlan pl = bhwp_frames_plan(p, f, t != nullptr, -1, L, true);
    const char *what = t ? "f32 frames launch (resident table)" : "f32 frames launch";
    return run_source(t, p, L, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                         const BhwLenPhase *lp) { return bhwk_frames_f32(l, c, w, pl, f, d_x, d_y, tab, lp); });
}

// Every float32 overlap-add, as frames_f32_run; flags: BHW_OLA_NORMALIZE or 0.
int ola_f32_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_ola *o, uint32_t flags, const float *d_y,
                float *d_x)
{
    int rc = bhwp_f32_checks(p, length, flags);
    if (!rc && t) rc = table_call_checks(t, p);
    if (!rc) rc = bhwp_ola_checks(p, o, d_y, d_x, true, length);
    if (rc || !o->count) return rc;
    const uint64_t L = len_route(p, length);
    const bool norm = (flags & BHW_OLA_NORMALIZE) != 0;
    const BhwOlaPlan pl = bhwp_ola_plan(p, o, t != nullptr, 0, 0, L, norm ? kOlaQMaxNorm : kOlaQMax);
    const char *what = t ? "f32 overlap-add launch (resident table)" : "f32 overlap-add launch";
    return run_source(t, p, L, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                         const BhwLenPhase *lp) { return bhwk_ola_f32(l, c, w, pl, o, norm, d_y, d_x, tab, lp); });
}

// A batched STFT frames call (t NULL: the direct CORDIC chains): the checks, then the frames kernel at the angles of the length-L
// phase map, for every L.
int stft_frames_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, const float *d_x,
                    float *d_y)
{
    int rc = bhwp_f32_checks(p, length, 0);
    if (!rc && t) rc = table_call_checks(t, p);
    if (!rc) rc = bhwp_stft_checks(p, length, s, false, 0, d_x, d_y);
    if (rc || !s->frames) return rc;
    const BhwStftPlan pl = bhwp_stft_plan(p, length, s, t != nullptr);
    const char *what = t ? "stft frames launch (resident table)" : "stft frames launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) { return bhwk_stft_frames_f32(l, c, w, pl, s, d_x, d_y, tab, *lp); });
}

// A batched STFT overlap-add: the float32 overlap-add of every signal in one launch (bhwp_stft_ola maps the descriptor onto it; the
// power-of-two kernels at L = 2^phi_width, the any-length ones otherwise).
int istft_ola_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                  const float *d_y, float *d_x)
{
    int rc = bhwp_f32_checks(p, length, flags);
    if (!rc && t) rc = table_call_checks(t, p);
    if (!rc) rc = bhwp_stft_checks(p, length, s, true, flags, d_x, d_y);
    if (rc || !s->samples) return rc;
    bhw_ola o;
    BhwOlaBatch bt;
    bhwp_stft_ola(s, o, bt);
    const uint64_t L = bhwp_len_kernels(p, length, false) ? length : 0;
    const bool norm = (flags & BHW_OLA_NORMALIZE) != 0;
    const BhwOlaPlan pl = bhwp_ola_plan(p, &o, t != nullptr, 0, 0, L, norm ? kOlaQMaxNorm : kOlaQMax, bt.batch);
    const float *rows = d_y + s->col0 * s->channels;             // the window columns of each row
    const char *what = t ? "istft overlap-add launch (resident table)" : "istft overlap-add launch";
    return run_source(t, p, L, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                         const BhwLenPhase *lp) { return bhwk_ola_f32(l, c, w, pl, &o, norm, rows, d_x, tab, lp, bt); });
}

// The fused window + FFT (t NULL: the direct CORDIC chains): the checks, then the one kernel.
int stft_fft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                 const float *d_x, float *d_Y)
{
    int rc = bhwp_stft_fft_checks(p, length, s, flags, d_x, d_Y);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const BhwStftFftPlan pl = bhwp_stft_fft_plan(p, length, s, flags, t != nullptr);
    const char *what = t ? "stft fft launch (resident table)" : "stft fft launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) { return bhwk_stft_fft_f32(l, c, w, pl, s, d_x, d_Y, tab, *lp); });
}

// The fused window + complex FFT for I/Q input (t NULL: the direct CORDIC chains): the checks, then the one kernel.
int stft_cfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                  const float *d_x, float *d_Y)
{
    int rc = bhwp_stft_cfft_checks(p, length, s, flags, d_x, d_Y);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const BhwStftCfftPlan pl = bhwp_stft_cfft_plan(p, length, s, flags, t != nullptr);
    const char *what = t ? "stft cfft launch (resident table)" : "stft cfft launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) { return bhwk_stft_cfft_f32(l, c, w, pl, s, d_x, d_Y, tab, *lp); });
}

// The mixed-radix fused window + complex FFT for I/Q input (t NULL: the direct CORDIC chains): the checks, then the one kernel.
int stft_cmfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                   const float *d_x, float *d_Y)
{
    int rc = bhwp_stft_cmfft_checks(p, length, s, flags, d_x, d_Y);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const BhwStftCmfftPlan pl = bhwp_stft_cmfft_plan(p, length, s, flags, t != nullptr);
    const char *what = t ? "stft cmfft launch (resident table)" : "stft cmfft launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) { return bhwk_stft_cmfft_f32(l, c, w, pl, s, d_x, d_Y, tab, *lp); });
}

// The fused spectrogram (t NULL: the direct CORDIC chains): the checks, then the one kernel.
int spectrogram_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                    const bhw_fbank *fb, const float *d_x, float *d_P)
{
    int rc = bhwp_spectrogram_checks(p, length, s, flags, fb, d_x, d_P);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const BhwStftFftPlan pl = bhwp_spectrogram_plan(p, length, s, flags, fb, t != nullptr);
    const char *what = t ? "spectrogram launch (resident table)" : "spectrogram launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) { return bhwk_spectrogram_f32(l, c, w, pl, s, fb, d_x, d_P, tab, *lp); });
}

// The fused log spectrogram / MFCC of either radix family (t NULL: the direct CORDIC chains): the checks, then the one kernel.
int logspec_run(bool mixed, bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                const bhw_fbank *fb, const bhw_logspec *ls, const float *d_x, float *d_out)
{
    int rc = bhwp_logspec_checks(mixed, p, length, s, flags, fb, ls, d_x, d_out);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const char *what = t ? "logspec launch (resident table)" : "logspec launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) {
        if (mixed) return bhwk_logspec_mfft_f32(l, c, w, bhwp_logspec_mfft_plan(p, length, s, flags, fb, ls, t != nullptr), s, fb, ls, d_x, d_out, tab, *lp);
        return bhwk_logspec_f32(l, c, w, bhwp_logspec_plan(p, length, s, flags, fb, ls, t != nullptr), s, fb, ls, d_x, d_out, tab, *lp);
    });
}

// The fused Welch PSD (t NULL: the direct CORDIC chains): the checks, then the accumulating kernel and its join.
int welch_fft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                  double scale, uint32_t psd_flags, const float *d_x, float *d_P, uint64_t p_stride, void *workspace, uint64_t workspace_bytes)
{
    int rc = bhwp_welch_fft_checks(p, length, s, flags, scale, psd_flags, p_stride, d_x, d_P, workspace, workspace_bytes);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const BhwWelchFftPlan pl = bhwp_welch_fft_plan(p, length, s, flags, p_stride, t != nullptr);
    const char *what = t ? "welch fft launch (resident table)" : "welch fft launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) {
        return bhwk_welch_fft_f32(l, c, w, pl, s, scale, psd_flags, d_x, d_P, (double *)workspace, tab, *lp);
    });
}

// The fused Welch cross spectra (t NULL: the direct CORDIC chains): the checks, then the accumulating kernel and its join.
int csd_fft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags, double scale,
                uint32_t csd_flags, const float *d_x, const float *d_y, float *const *outs, uint64_t o_stride, void *workspace,
                uint64_t workspace_bytes)
{
    int rc = bhwp_csd_fft_checks(p, length, s, flags, scale, csd_flags, o_stride, d_x, d_y, (const void *const *)outs, workspace,
                                 workspace_bytes);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const BhwCsdFftPlan pl = bhwp_csd_fft_plan(p, length, s, flags, csd_flags, o_stride, t != nullptr);
    const char *what = t ? "csd fft launch (resident table)" : "csd fft launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) {
        return bhwk_csd_fft_f32(l, c, w, pl, s, scale, d_x, d_y, outs, (double *)workspace, tab, *lp);
    });
}

// The fused Welch PSD for I/Q input (t NULL: the direct CORDIC chains): the checks, then the accumulating kernel and the join.
int welch_cfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                   double scale, const float *d_x, float *d_P, uint64_t p_stride, void *workspace, uint64_t workspace_bytes)
{
    int rc = bhwp_welch_cfft_checks(p, length, s, flags, scale, p_stride, d_x, d_P, workspace, workspace_bytes);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const BhwWelchCfftPlan pl = bhwp_welch_cfft_plan(p, length, s, flags, p_stride, t != nullptr);
    const char *what = t ? "welch cfft launch (resident table)" : "welch cfft launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) {
        return bhwk_welch_cfft_f32(l, c, w, pl, s, scale, d_x, d_P, (double *)workspace, tab, *lp);
    });
}

// The fused Welch PSD for I/Q input at a mixed-radix n_fft (t NULL: the direct CORDIC chains): the checks, then the accumulating kernel
// and the join.
int welch_cmfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                    double scale, const float *d_x, float *d_P, uint64_t p_stride, void *workspace, uint64_t workspace_bytes)
{
    int rc = bhwp_welch_cmfft_checks(p, length, s, flags, scale, p_stride, d_x, d_P, workspace, workspace_bytes);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const BhwWelchCmfftPlan pl = bhwp_welch_cmfft_plan(p, length, s, flags, p_stride, t != nullptr);
    const char *what = t ? "welch cmfft launch (resident table)" : "welch cmfft launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) {
        return bhwk_welch_cmfft_f32(l, c, w, pl, s, scale, d_x, d_P, (double *)workspace, tab, *lp);
    });
}

// The fused max-hold / min-hold traces for I/Q input (t NULL: the direct CORDIC chains): the checks, then the reducing kernel and the
// join.  A NULL output is a trace that is not stored.
int hold_cfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                  double scale, const float *d_x, float *d_max, float *d_min, uint64_t p_stride, void *workspace, uint64_t workspace_bytes)
{
    int rc = bhwp_hold_cfft_checks(p, length, s, flags, scale, p_stride, d_x, d_max, d_min, workspace, workspace_bytes);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const uint32_t traces = (d_max ? BHW_HOLD_MAX : 0u) | (d_min ? BHW_HOLD_MIN : 0u);
    const BhwHoldCfftPlan pl = bhwp_hold_cfft_plan(p, length, s, flags, p_stride, traces, t != nullptr);
    const char *what = t ? "hold cfft launch (resident table)" : "hold cfft launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) {
        return bhwk_hold_cfft_f32(l, c, w, pl, s, scale, d_x, d_max, d_min, workspace, tab, *lp);
    });
}

// The same at a mixed-radix n_fft.
int hold_cmfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                   double scale, const float *d_x, float *d_max, float *d_min, uint64_t p_stride, void *workspace, uint64_t workspace_bytes)
{
    int rc = bhwp_hold_cmfft_checks(p, length, s, flags, scale, p_stride, d_x, d_max, d_min, workspace, workspace_bytes);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const uint32_t traces = (d_max ? BHW_HOLD_MAX : 0u) | (d_min ? BHW_HOLD_MIN : 0u);
    const BhwHoldCmfftPlan pl = bhwp_hold_cmfft_plan(p, length, s, flags, p_stride, traces, t != nullptr);
    const char *what = t ? "hold cmfft launch (resident table)" : "hold cmfft launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) {
        return bhwk_hold_cmfft_f32(l, c, w, pl, s, scale, d_x, d_max, d_min, workspace, tab, *lp);
    });
}

// The fused Welch PSD at a mixed-radix n_fft (t NULL: the direct CORDIC chains): the checks, then the accumulating kernel and the join.
int welch_mfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                   double scale, uint32_t psd_flags, const float *d_x, float *d_P, uint64_t p_stride, void *workspace, uint64_t workspace_bytes)
{
    int rc = bhwp_welch_mfft_checks(p, length, s, flags, scale, psd_flags, p_stride, d_x, d_P, workspace, workspace_bytes);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const BhwWelchMfftPlan pl = bhwp_welch_mfft_plan(p, length, s, flags, p_stride, t != nullptr);
    const char *what = t ? "welch mfft launch (resident table)" : "welch mfft launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) {
        return bhwk_welch_mfft_f32(l, c, w, pl, s, scale, psd_flags, d_x, d_P, (double *)workspace, tab, *lp);
    });
}

// The fused max-hold / min-hold traces for real input (t NULL: the direct CORDIC chains): the checks, then the reducing kernel and the
// join.  A NULL output is a trace that is not stored.
int hold_fft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                 double scale, uint32_t psd_flags, const float *d_x, float *d_max, float *d_min, uint64_t p_stride, void *workspace,
                 uint64_t workspace_bytes)
{
    int rc = bhwp_hold_fft_checks(p, length, s, flags, scale, psd_flags, p_stride, d_x, d_max, d_min, workspace, workspace_bytes);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const uint32_t traces = (d_max ? BHW_HOLD_MAX : 0u) | (d_min ? BHW_HOLD_MIN : 0u);
    const BhwHoldFftPlan pl = bhwp_hold_fft_plan(p, length, s, flags, p_stride, traces, t != nullptr);
    const char *what = t ? "hold fft launch (resident table)" : "hold fft launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) {
        return bhwk_hold_fft_f32(l, c, w, pl, s, scale, psd_flags, d_x, d_max, d_min, workspace, tab, *lp);
    });
}

// The same at a mixed-radix n_fft.
int hold_mfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                  double scale, uint32_t psd_flags, const float *d_x, float *d_max, float *d_min, uint64_t p_stride, void *workspace,
                  uint64_t workspace_bytes)
{
    int rc = bhwp_hold_mfft_checks(p, length, s, flags, scale, psd_flags, p_stride, d_x, d_max, d_min, workspace, workspace_bytes);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const uint32_t traces = (d_max ? BHW_HOLD_MAX : 0u) | (d_min ? BHW_HOLD_MIN : 0u);
    const BhwHoldMfftPlan pl = bhwp_hold_mfft_plan(p, length, s, flags, p_stride, traces, t != nullptr);
    const char *what = t ? "hold mfft launch (resident table)" : "hold mfft launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) {
        return bhwk_hold_mfft_f32(l, c, w, pl, s, scale, psd_flags, d_x, d_max, d_min, workspace, tab, *lp);
    });
}

// The mixed-radix fused window + FFT in its three output forms (t NULL: the direct CORDIC chains): the checks, then the one kernel.
int stft_mfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                  const bhw_fbank *fb, const float *d_x, float *d_out)
{
    int rc = bhwp_stft_mfft_checks(p, length, s, flags, fb, d_x, d_out);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const BhwStftMfftPlan pl = bhwp_stft_mfft_plan(p, length, s, flags, fb, t != nullptr);
    const char *what = t ? "stft mfft launch (resident table)" : "stft mfft launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) { return bhwk_stft_mfft_f32(l, c, w, pl, s, fb, d_x, d_out, tab, *lp); });
}

// The fused inverse FFT + overlap-add of a family (t NULL: the direct CORDIC chains): its checks, then its plan and its one kernel.
template <auto Checks, auto Plan, auto Launch>
int istft_run(const char *what, const char *what_table, bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream,
              const bhw_stft *s, uint32_t flags, const float *d_Y, float *d_x)
{
    int rc = Checks(p, length, s, flags, d_Y, d_x, true);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->samples) return rc;
    const auto pl = Plan(p, length, s, flags, t != nullptr);
    return run_source(t, p, length, device, stream, t ? what_table : what,
                      [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab, const BhwLenPhase *lp) {
                          return Launch(l, c, w, pl, s, d_Y, d_x, tab, *lp);
                      });
}

// Real output at a power of two and at a mixed-radix n_fft, I/Q output at a power of two and at a mixed-radix n_fft.
int istft_fft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                  const float *d_Y, float *d_x)
{
    return istft_run<bhwp_istft_fft_checks, bhwp_istft_fft_plan, bhwk_istft_fft_f32>(
        "istft fft launch", "istft fft launch (resident table)", t, p, length, device, stream, s, flags, d_Y, d_x);
}

int istft_mfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                   const float *d_Y, float *d_x)
{
    return istft_run<bhwp_istft_mfft_checks, bhwp_istft_mfft_plan, bhwk_istft_mfft_f32>(
        "istft mfft launch", "istft mfft launch (resident table)", t, p, length, device, stream, s, flags, d_Y, d_x);
}

int istft_cfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                   const float *d_Y, float *d_x)
{
    return istft_run<bhwp_istft_cfft_checks, bhwp_istft_cfft_plan, bhwk_istft_cfft_f32>(
        "istft cfft launch", "istft cfft launch (resident table)", t, p, length, device, stream, s, flags, d_Y, d_x);
}

int istft_cmfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                    const float *d_Y, float *d_x)
{
    return istft_run<bhwp_istft_cmfft_checks, bhwp_istft_cmfft_plan, bhwk_istft_cmfft_f32>(
        "istft cmfft launch", "istft cmfft launch (resident table)", t, p, length, device, stream, s, flags, d_Y, d_x);
}

// The fused STFT, mask and inverse STFT (t NULL: the direct CORDIC chains): its checks, then the inverse plan and the one kernel.  One
// text for the two families and the two gain types: Checks / Plan / Kernel are bhwp_[c]mask_[m]fft_checks, bhwp_mask_[m]fft_plan (the
// complex-gain calls run the real-gain plan, their strides in pairs) and bhwk_[c]mask_[m]fft_f32.
template <auto Checks, auto Plan, auto Kernel>
int mask_run(const char *what, const char *what_table, bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream,
             const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride,
             uint64_t g_batch_stride, float *d_out)
{
    int rc = Checks(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out, true);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !ss->samples) return rc;
    const auto pl = Plan(p, length, sa, ss, flags, g_stride, g_batch_stride, t != nullptr);
    return run_source(t, p, length, device, stream, t ? what_table : what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w,
                                                                               const int32_t *tab, const BhwLenPhase *lp) {
        return Kernel(l, c, w, pl, sa, ss, d_x, d_g, d_out, tab, *lp);
    });
}

int mask_fft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *sa, const bhw_stft *ss,
                 uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out)
{
    return mask_run<bhwp_mask_fft_checks, bhwp_mask_fft_plan, bhwk_mask_fft_f32>(
        "mask fft launch", "mask fft launch (resident table)", t, p, length, device, stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
}

int mask_mfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *sa, const bhw_stft *ss,
                  uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out)
{
    return mask_run<bhwp_mask_mfft_checks, bhwp_mask_mfft_plan, bhwk_mask_mfft_f32>(
        "mask mfft launch", "mask mfft launch (resident table)", t, p, length, device, stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
}

// d_g: interleaved float32 pairs (gr, gi), the strides in pairs
int cmask_fft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *sa, const bhw_stft *ss,
                  uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out)
{
    return mask_run<bhwp_cmask_fft_checks, bhwp_mask_fft_plan, bhwk_cmask_fft_f32>(
        "cmask fft launch", "cmask fft launch (resident table)", t, p, length, device, stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
}

int cmask_mfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *sa, const bhw_stft *ss,
                   uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out)
{
    return mask_run<bhwp_cmask_mfft_checks, bhwp_mask_mfft_plan, bhwk_cmask_mfft_f32>(
        "cmask mfft launch", "cmask mfft launch (resident table)", t, p, length, device, stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
}

// The same for I/Q input (d_x, d_out: interleaved I/Q; K = n_fft gains a row), a real gain or a pair per bin
int mask_cfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *sa, const bhw_stft *ss,
                  uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out)
{
    return mask_run<bhwp_mask_cfft_checks, bhwp_mask_cfft_plan, bhwk_mask_cfft_f32>(
        "mask cfft launch", "mask cfft launch (resident table)", t, p, length, device, stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
}

int cmask_cfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *sa, const bhw_stft *ss,
                   uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out)
{
    return mask_run<bhwp_cmask_cfft_checks, bhwp_mask_cfft_plan, bhwk_cmask_cfft_f32>(
        "cmask cfft launch", "cmask cfft launch (resident table)", t, p, length, device, stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
}

int mask_cmfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *sa, const bhw_stft *ss,
                   uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out)
{
    return mask_run<bhwp_mask_cmfft_checks, bhwp_mask_cmfft_plan, bhwk_mask_cmfft_f32>(
        "mask cmfft launch", "mask cmfft launch (resident table)", t, p, length, device, stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
}

int cmask_cmfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *sa, const bhw_stft *ss,
                    uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out)
{
    return mask_run<bhwp_cmask_cmfft_checks, bhwp_mask_cmfft_plan, bhwk_cmask_cmfft_f32>(
        "cmask cmfft launch", "cmask cmfft launch (resident table)", t, p, length, device, stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
}

// The fused filter-and-sum over ch.n_ch channels: mask_run with the channel axis (Checks / Plan / Kernel: bhwp_beam_[m]fft_checks,
// bhwp_beam_[m]fft_plan, bhwk_beam_[m]fft_f32).
template <auto Checks, auto Plan, auto Kernel>
int beam_run(const char *what, const char *what_table, bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream,
             const bhw_stft *sa, const bhw_stft *ss, uint32_t flags, const float *d_x, const BhwBeamAxis &ch, const float *d_g,
             uint64_t g_stride, uint64_t g_batch_stride, float *d_out)
{
    int rc = Checks(p, length, sa, ss, flags, d_x, ch, d_g, g_stride, g_batch_stride, d_out, true);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !ss->samples) return rc;
    const auto pl = Plan(p, length, sa, ss, flags, ch, g_stride, g_batch_stride, t != nullptr);
    return run_source(t, p, length, device, stream, t ? what_table : what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w,
                                                                               const int32_t *tab, const BhwLenPhase *lp) {
        return Kernel(l, c, w, pl, sa, ss, d_x, d_g, d_out, tab, *lp);
    });
}

int beam_fft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *sa, const bhw_stft *ss,
                 uint32_t flags, const float *d_x, const BhwBeamAxis &ch, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride,
                 float *d_out)
{
    return beam_run<bhwp_beam_fft_checks, bhwp_beam_fft_plan, bhwk_beam_fft_f32>(
        "beam fft launch", "beam fft launch (resident table)", t, p, length, device, stream, sa, ss, flags, d_x, ch, d_g, g_stride, g_batch_stride,
        d_out);
}

int beam_mfft_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *sa, const bhw_stft *ss,
                  uint32_t flags, const float *d_x, const BhwBeamAxis &ch, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride,
                  float *d_out)
{
    return beam_run<bhwp_beam_mfft_checks, bhwp_beam_mfft_plan, bhwk_beam_mfft_f32>(
        "beam mfft launch", "beam mfft launch (resident table)", t, p, length, device, stream, sa, ss, flags, d_x, ch, d_g, g_stride,
        g_batch_stride, d_out);
}

// The window sums (t NULL: the direct CORDIC chains): the checks, then the memset of the four words and the reduction.
int window_sums_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, uint32_t flags, uint64_t *d_sums)
{
    int rc = bhwp_sums_checks(p, length, flags, d_sums);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc) return rc;
    const BhwSumsPlan pl = bhwp_sums_plan(length);
    const char *what = t ? "window sums launch (resident table)" : "window sums launch";
    return run_source(t, p, length, device, stream, what, [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab,
                                                              const BhwLenPhase *lp) { return bhwk_window_sums(l, c, w, pl, flags, tab, *lp, d_sums); });
}

// The Welch segments: flags 0 is the stft frames kernel on the same descriptor; with detrending the mean pass and the frames loop.
int welch_frames_run(bhw_table t, const bhw_params *p, uint64_t length, int device, void *stream, const bhw_stft *s, uint32_t flags,
                     const float *d_x, float *d_y, void *workspace, uint64_t workspace_bytes)
{
    int rc = bhwp_welch_checks(p, length, s, flags, d_x, d_y, workspace, workspace_bytes);
    if (!rc && t) rc = table_call_checks(t, p);
    if (rc || !s->frames) return rc;
    const BhwWelchPlan pl = bhwp_welch_plan(p, length, s, flags, t != nullptr);
    const char *what = t ? "welch segments launch (resident table)" : "welch segments launch";
    if (!pl.detrend)                                               // the stft frames kernel itself, under the Welch extent rule
        return run_source(t, p, length, device, stream, what,
                          [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab, const BhwLenPhase *lp) {
                              return bhwk_stft_frames_f32(l, c, w, pl.frames, s, d_x, d_y, tab, *lp);
                          });
    return run_source(t, p, length, device, stream, what,
                      [&](const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const int32_t *tab, const BhwLenPhase *lp) {
                          return bhwk_welch_frames_f32(l, c, w, pl, s, d_x, d_y, (float *)workspace, tab, *lp);
                      });
}

} // namespace

extern "C" {

// Each *_len call: bhwp_len_checks, then (from-table calls) the handle, then the route -- the existing calls at L = 2^phi_width.
int bhw_generate_len_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, uint64_t n0, uint64_t count, int32_t *d_out)
{
    const int rc = bhwp_len_checks(p, length);
    if (rc) return rc;
    if (!len_route(p, length)) return generate_impl(p, device, hip_stream, n0, count, d_out, nullptr);
    return generate_len(nullptr, p, length, device, hip_stream, n0, count, d_out);
}

int bhw_generate_len_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, uint64_t n0, uint64_t count,
                                int32_t *d_out)
{
    int rc = bhwp_len_checks(p, length);
    if (!rc && !t) rc = fail(BHW_ERR_BADARG, "table is NULL");
    if (rc) return rc;
    if (!len_route(p, length)) return from_table(t, p, hip_stream, n0, count, d_out);
    return generate_len(t, p, length, t->device, hip_stream, n0, count, d_out);
}

int bhw_apply_frames_len_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_frames *f, const int32_t *d_x,
                                int32_t *d_y)
{
    const int rc = bhwp_len_checks(p, length);
    return rc ? rc : frames_run(nullptr, p, len_route(p, length), device, hip_stream, f, d_x, d_y);
}

int bhw_apply_frames_len_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_frames *f,
                                    const int32_t *d_x, int32_t *d_y)
{
    int rc = bhwp_len_checks(p, length);
    if (!rc && !t) rc = fail(BHW_ERR_BADARG, "table is NULL");
    return rc ? rc : frames_run(t, p, len_route(p, length), t->device, hip_stream, f, d_x, d_y);
}

int bhw_overlap_add_len_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_ola *o, const int32_t *d_y,
                               int32_t *d_x)
{
    const int rc = bhwp_len_checks(p, length);
    return rc ? rc : ola_run(nullptr, p, len_route(p, length), device, hip_stream, o, d_y, d_x);
}

int bhw_overlap_add_len_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_ola *o, const int32_t *d_y,
                                   int32_t *d_x)
{
    int rc = bhwp_len_checks(p, length);
    if (!rc && !t) rc = fail(BHW_ERR_BADARG, "table is NULL");
    return rc ? rc : ola_run(t, p, len_route(p, length), t->device, hip_stream, o, d_y, d_x);
}

int bhw_describe_len(bhw_table t, const bhw_params *p, uint64_t length, uint64_t n0, uint64_t count, const bhw_frames *f, const bhw_ola *o,
                     char *buf, uint64_t len)
{
    int rc = bhwp_len_checks(p, length);
    if (!rc && t) rc = table_call_checks(t, p);
    if (!rc && f) rc = bhwp_frames_checks(p, f, nullptr, nullptr, false, length);
    if (!rc && o) rc = bhwp_ola_checks(p, o, nullptr, nullptr, false, length);
    return rc ? rc : bhwp_describe_len(p, t ? &t->c : nullptr, t ? t->tiled : false, length, g_len_force, n0, count, f, o, buf, len);
}

// ---- float32 frame apply and overlap-add (include/bhw.h: bhw_apply_frames_f32_device ...) -----------------------------------------
// Each *_f32 call: bhwp_f32_checks, then (from-table calls) the handle, then the checks of the int32 counterpart with L in place of N,
// then the float32 kernels: at L = 2^phi_width those of the power-of-two window, else the any-length forms (len_route).  Every route
// allocates nothing and uses no scratch.

int bhw_apply_frames_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_frames *f, const float *d_x,
                                float *d_y)
{
    return frames_f32_run(nullptr, p, length, device, hip_stream, f, d_x, d_y);
}

int bhw_apply_frames_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_frames *f,
                                    const float *d_x, float *d_y)
{
    const int rc = bhwp_f32_checks(p, length, 0);
    if (rc) return rc;
    return t ? frames_f32_run(t, p, length, t->device, hip_stream, f, d_x, d_y) : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_overlap_add_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_ola *o, uint32_t flags,
                               const float *d_y, float *d_x)
{
    return ola_f32_run(nullptr, p, length, device, hip_stream, o, flags, d_y, d_x);
}

int bhw_overlap_add_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_ola *o, uint32_t flags,
                                   const float *d_y, float *d_x)
{
    const int rc = bhwp_f32_checks(p, length, flags);
    if (rc) return rc;
    return t ? ola_f32_run(t, p, length, t->device, hip_stream, o, flags, d_y, d_x) : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_f32(bhw_table t, const bhw_params *p, uint64_t length, const bhw_frames *f, const bhw_ola *o, uint32_t flags, char *buf,
                     uint64_t len)
{
    int rc = bhwp_f32_checks(p, length, flags);
    if (!rc && t) rc = table_call_checks(t, p);
    if (!rc && f) rc = bhwp_frames_checks(p, f, nullptr, nullptr, false, length);
    if (!rc && o) rc = bhwp_ola_checks(p, o, nullptr, nullptr, false, length);
    return rc ? rc : bhwp_describe_f32(p, t ? &t->c : nullptr, length, g_len_force, f, o, flags, buf, len);
}

// ---- batched, centred STFT framing and overlap-add (include/bhw.h: bhw_stft_frames_f32_device ...) ------------------------------------

int bhw_stft_frames_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, const float *d_x,
                               float *d_y)
{
    return stft_frames_run(nullptr, p, length, device, hip_stream, s, d_x, d_y);
}

int bhw_stft_frames_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, const float *d_x,
                                   float *d_y)
{
    const int rc = bhwp_f32_checks(p, length, 0);
    if (rc) return rc;
    return t ? stft_frames_run(t, p, length, t->device, hip_stream, s, d_x, d_y) : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_istft_ola_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                             const float *d_y, float *d_x)
{
    return istft_ola_run(nullptr, p, length, device, hip_stream, s, flags, d_y, d_x);
}

int bhw_istft_ola_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                 const float *d_y, float *d_x)
{
    const int rc = bhwp_f32_checks(p, length, flags);
    if (rc) return rc;
    return t ? istft_ola_run(t, p, length, t->device, hip_stream, s, flags, d_y, d_x) : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_stft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, int inverse, uint32_t flags, char *buf,
                      uint64_t len)
{
    int rc = bhwp_f32_checks(p, length, flags);
    if (!rc && t) rc = table_call_checks(t, p);
    if (!rc) rc = bhwp_stft_checks(p, length, s, inverse != 0, flags, nullptr, nullptr, false);
    return rc ? rc : bhwp_describe_stft(p, t ? &t->c : nullptr, length, s, inverse != 0, flags, buf, len);
}

// ---- fused window and real FFT (include/bhw.h: bhw_stft_fft_f32_device ...) ------------------------------------------------------------

int bhw_stft_fft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                            const float *d_x, float *d_Y)
{
    return stft_fft_run(nullptr, p, length, device, hip_stream, s, flags, d_x, d_Y);
}

int bhw_stft_fft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                const float *d_x, float *d_Y)
{
    const int rc = bhwp_stft_fft_checks(p, length, s, flags, d_x, d_Y);
    if (rc) return rc;
    return t ? stft_fft_run(t, p, length, t->device, hip_stream, s, flags, d_x, d_Y) : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_stft_fft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len)
{
    int rc = bhwp_stft_fft_checks(p, length, s, flags, nullptr, nullptr, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_stft_fft(p, t ? &t->c : nullptr, length, s, flags, buf, len);
}

// ---- fused power and filter-bank spectrogram (include/bhw.h: bhw_spectrogram_f32_device ...) -------------------------------------------

int bhw_spectrogram_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                               const bhw_fbank *fb, const float *d_x, float *d_P)
{
    return spectrogram_run(nullptr, p, length, device, hip_stream, s, flags, fb, d_x, d_P);
}

int bhw_spectrogram_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                   const bhw_fbank *fb, const float *d_x, float *d_P)
{
    const int rc = bhwp_spectrogram_checks(p, length, s, flags, fb, d_x, d_P);
    if (rc) return rc;
    return t ? spectrogram_run(t, p, length, t->device, hip_stream, s, flags, fb, d_x, d_P) : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_spectrogram(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                             char *buf, uint64_t len)
{
    int rc = bhwp_spectrogram_checks(p, length, s, flags, fb, nullptr, nullptr, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_spectrogram(p, t ? &t->c : nullptr, length, s, flags, fb, buf, len);
}

// ---- fused Welch PSD (include/bhw.h: bhw_welch_fft_f32_device ...) ----------------------------------------------------------------------

uint64_t bhw_welch_fft_workspace_bytes(const bhw_stft *s)
{
    return s && s->struct_size == sizeof(bhw_stft) ? bhwp_welch_fft_workspace_bytes(s) : 0;
}

int bhw_welch_fft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                             double scale, uint32_t psd_flags, const float *d_x, float *d_P, uint64_t p_stride, void *workspace,
                             uint64_t workspace_bytes)
{
    return welch_fft_run(nullptr, p, length, device, hip_stream, s, flags, scale, psd_flags, d_x, d_P, p_stride, workspace, workspace_bytes);
}

int bhw_welch_fft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                 double scale, uint32_t psd_flags, const float *d_x, float *d_P, uint64_t p_stride, void *workspace,
                                 uint64_t workspace_bytes)
{
    const int rc = bhwp_welch_fft_checks(p, length, s, flags, scale, psd_flags, p_stride, d_x, d_P, workspace, workspace_bytes);
    if (rc) return rc;
    return t ? welch_fft_run(t, p, length, t->device, hip_stream, s, flags, scale, psd_flags, d_x, d_P, p_stride, workspace, workspace_bytes)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_welch_fft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len)
{
    int rc = bhwp_welch_fft_checks(p, length, s, flags, 0.0, 0, 0, nullptr, nullptr, nullptr, 0, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_welch_fft(p, t ? &t->c : nullptr, length, s, flags, buf, len);
}

// ---- fused Welch cross spectra (include/bhw.h: bhw_csd_fft_f32_device ...) ------------------------------------------------------------------

uint64_t bhw_csd_fft_workspace_bytes(const bhw_stft *s)
{
    return s && s->struct_size == sizeof(bhw_stft) ? bhwp_csd_fft_workspace_bytes(s) : 0;
}

int bhw_csd_fft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                           double scale, uint32_t csd_flags, const float *d_x, const float *d_y, float *d_Pxy, float *d_Pxx, float *d_Pyy,
                           float *d_Cxy, float *d_H1, uint64_t o_stride, void *workspace, uint64_t workspace_bytes)
{
    float *const outs[kCsdOutputs] = {d_Pxy, d_Pxx, d_Pyy, d_Cxy, d_H1};
    return csd_fft_run(nullptr, p, length, device, hip_stream, s, flags, scale, csd_flags, d_x, d_y, outs, o_stride, workspace, workspace_bytes);
}

int bhw_csd_fft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                               double scale, uint32_t csd_flags, const float *d_x, const float *d_y, float *d_Pxy, float *d_Pxx,
                               float *d_Pyy, float *d_Cxy, float *d_H1, uint64_t o_stride, void *workspace, uint64_t workspace_bytes)
{
    float *const outs[kCsdOutputs] = {d_Pxy, d_Pxx, d_Pyy, d_Cxy, d_H1};
    const int rc = bhwp_csd_fft_checks(p, length, s, flags, scale, csd_flags, o_stride, d_x, d_y, (const void *const *)outs, workspace,
                                       workspace_bytes);
    if (rc) return rc;
    return t ? csd_fft_run(t, p, length, t->device, hip_stream, s, flags, scale, csd_flags, d_x, d_y, outs, o_stride, workspace, workspace_bytes)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_csd_fft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint32_t csd_flags, char *buf,
                         uint64_t len)
{
    int rc = bhwp_csd_fft_checks(p, length, s, flags, 0.0, csd_flags, 0, nullptr, nullptr, nullptr, nullptr, 0, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_csd_fft(p, t ? &t->c : nullptr, length, s, flags, csd_flags, buf, len);
}

// ---- fused Welch PSD for I/Q input (include/bhw.h: bhw_welch_cfft_f32_device ...) -----------------------------------------------------------

uint64_t bhw_welch_cfft_workspace_bytes(const bhw_stft *s)
{
    return s && s->struct_size == sizeof(bhw_stft) ? bhwp_welch_cfft_workspace_bytes(s) : 0;
}

int bhw_welch_cfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                              double scale, const float *d_x, float *d_P, uint64_t p_stride, void *workspace, uint64_t workspace_bytes)
{
    return welch_cfft_run(nullptr, p, length, device, hip_stream, s, flags, scale, d_x, d_P, p_stride, workspace, workspace_bytes);
}

int bhw_welch_cfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                  double scale, const float *d_x, float *d_P, uint64_t p_stride, void *workspace, uint64_t workspace_bytes)
{
    const int rc = bhwp_welch_cfft_checks(p, length, s, flags, scale, p_stride, d_x, d_P, workspace, workspace_bytes);
    if (rc) return rc;
    return t ? welch_cfft_run(t, p, length, t->device, hip_stream, s, flags, scale, d_x, d_P, p_stride, workspace, workspace_bytes)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_welch_cfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len)
{
    int rc = bhwp_welch_cfft_checks(p, length, s, flags, 0.0, 0, nullptr, nullptr, nullptr, 0, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_welch_cfft(p, t ? &t->c : nullptr, length, s, flags, buf, len);
}

// ---- fused Welch PSD for I/Q input at mixed-radix n_fft (include/bhw.h: bhw_welch_cmfft_f32_device ...) ----------------------------------

uint64_t bhw_welch_cmfft_workspace_bytes(const bhw_stft *s)
{
    return s && s->struct_size == sizeof(bhw_stft) ? bhwp_welch_cmfft_workspace_bytes(s) : 0;
}

int bhw_welch_cmfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                               double scale, const float *d_x, float *d_P, uint64_t p_stride, void *workspace, uint64_t workspace_bytes)
{
    return welch_cmfft_run(nullptr, p, length, device, hip_stream, s, flags, scale, d_x, d_P, p_stride, workspace, workspace_bytes);
}

int bhw_welch_cmfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                   double scale, const float *d_x, float *d_P, uint64_t p_stride, void *workspace, uint64_t workspace_bytes)
{
    const int rc = bhwp_welch_cmfft_checks(p, length, s, flags, scale, p_stride, d_x, d_P, workspace, workspace_bytes);
    if (rc) return rc;
    return t ? welch_cmfft_run(t, p, length, t->device, hip_stream, s, flags, scale, d_x, d_P, p_stride, workspace, workspace_bytes)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_welch_cmfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len)
{
    int rc = bhwp_welch_cmfft_checks(p, length, s, flags, 0.0, 0, nullptr, nullptr, nullptr, 0, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_welch_cmfft(p, t ? &t->c : nullptr, length, s, flags, buf, len);
}

// ---- fused max-hold / min-hold traces for I/Q input (include/bhw.h: bhw_hold_cfft_f32_device ..., bhw_hold_cmfft_f32_device ...) ----------

uint64_t bhw_hold_cfft_workspace_bytes(const bhw_stft *s)
{
    return s && s->struct_size == sizeof(bhw_stft) ? bhwp_hold_cfft_workspace_bytes(s) : 0;
}

int bhw_hold_cfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                             double scale, const float *d_x, float *d_max, float *d_min, uint64_t p_stride, void *workspace,
                             uint64_t workspace_bytes)
{
    return hold_cfft_run(nullptr, p, length, device, hip_stream, s, flags, scale, d_x, d_max, d_min, p_stride, workspace, workspace_bytes);
}

int bhw_hold_cfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                 double scale, const float *d_x, float *d_max, float *d_min, uint64_t p_stride, void *workspace,
                                 uint64_t workspace_bytes)
{
    const int rc = bhwp_hold_cfft_checks(p, length, s, flags, scale, p_stride, d_x, d_max, d_min, workspace, workspace_bytes);
    if (rc) return rc;
    return t ? hold_cfft_run(t, p, length, t->device, hip_stream, s, flags, scale, d_x, d_max, d_min, p_stride, workspace, workspace_bytes)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_hold_cfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint32_t traces, char *buf,
                           uint64_t len)
{
    int rc = bhwp_hold_cfft_checks(p, length, s, flags, 0.0, 0, nullptr, nullptr, nullptr, nullptr, 0, false);
    if (!rc) rc = bhwp_hold_traces_check(traces);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_hold_cfft(p, t ? &t->c : nullptr, length, s, flags, traces, buf, len);
}

uint64_t bhw_hold_cmfft_workspace_bytes(const bhw_stft *s)
{
    return s && s->struct_size == sizeof(bhw_stft) ? bhwp_hold_cmfft_workspace_bytes(s) : 0;
}

int bhw_hold_cmfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                              double scale, const float *d_x, float *d_max, float *d_min, uint64_t p_stride, void *workspace,
                              uint64_t workspace_bytes)
{
    return hold_cmfft_run(nullptr, p, length, device, hip_stream, s, flags, scale, d_x, d_max, d_min, p_stride, workspace, workspace_bytes);
}

int bhw_hold_cmfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                  double scale, const float *d_x, float *d_max, float *d_min, uint64_t p_stride, void *workspace,
                                  uint64_t workspace_bytes)
{
    const int rc = bhwp_hold_cmfft_checks(p, length, s, flags, scale, p_stride, d_x, d_max, d_min, workspace, workspace_bytes);
    if (rc) return rc;
    return t ? hold_cmfft_run(t, p, length, t->device, hip_stream, s, flags, scale, d_x, d_max, d_min, p_stride, workspace, workspace_bytes)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_hold_cmfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint32_t traces, char *buf,
                            uint64_t len)
{
    int rc = bhwp_hold_cmfft_checks(p, length, s, flags, 0.0, 0, nullptr, nullptr, nullptr, nullptr, 0, false);
    if (!rc) rc = bhwp_hold_traces_check(traces);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_hold_cmfft(p, t ? &t->c : nullptr, length, s, flags, traces, buf, len);
}

// ---- fused Welch PSD at mixed-radix n_fft (include/bhw.h: bhw_welch_mfft_f32_device ...) ---------------------------------------------------

uint64_t bhw_welch_mfft_workspace_bytes(const bhw_stft *s)
{
    return s && s->struct_size == sizeof(bhw_stft) ? bhwp_welch_mfft_workspace_bytes(s) : 0;
}

int bhw_welch_mfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                              double scale, uint32_t psd_flags, const float *d_x, float *d_P, uint64_t p_stride, void *workspace,
                              uint64_t workspace_bytes)
{
    return welch_mfft_run(nullptr, p, length, device, hip_stream, s, flags, scale, psd_flags, d_x, d_P, p_stride, workspace, workspace_bytes);
}

int bhw_welch_mfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                  double scale, uint32_t psd_flags, const float *d_x, float *d_P, uint64_t p_stride, void *workspace,
                                  uint64_t workspace_bytes)
{
    const int rc = bhwp_welch_mfft_checks(p, length, s, flags, scale, psd_flags, p_stride, d_x, d_P, workspace, workspace_bytes);
    if (rc) return rc;
    return t ? welch_mfft_run(t, p, length, t->device, hip_stream, s, flags, scale, psd_flags, d_x, d_P, p_stride, workspace, workspace_bytes)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_welch_mfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len)
{
    int rc = bhwp_welch_mfft_checks(p, length, s, flags, 0.0, 0, 0, nullptr, nullptr, nullptr, 0, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_welch_mfft(p, t ? &t->c : nullptr, length, s, flags, buf, len);
}

// ---- fused max-hold / min-hold traces for real input (include/bhw.h: bhw_hold_fft_f32_device ..., bhw_hold_mfft_f32_device ...) ------------

uint64_t bhw_hold_fft_workspace_bytes(const bhw_stft *s)
{
    return s && s->struct_size == sizeof(bhw_stft) ? bhwp_hold_fft_workspace_bytes(s) : 0;
}

int bhw_hold_fft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags, double scale,
                            uint32_t psd_flags, const float *d_x, float *d_max, float *d_min, uint64_t p_stride, void *workspace, uint64_t workspace_bytes)
{
    return hold_fft_run(nullptr, p, length, device, hip_stream, s, flags, scale, psd_flags, d_x, d_max, d_min, p_stride, workspace,
                        workspace_bytes);
}

int bhw_hold_fft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags, double scale,
                                uint32_t psd_flags, const float *d_x, float *d_max, float *d_min, uint64_t p_stride, void *workspace, uint64_t workspace_bytes)
{
    const int rc = bhwp_hold_fft_checks(p, length, s, flags, scale, psd_flags, p_stride, d_x, d_max, d_min, workspace, workspace_bytes);
    if (rc) return rc;
    return t ? hold_fft_run(t, p, length, t->device, hip_stream, s, flags, scale, psd_flags, d_x, d_max, d_min, p_stride, workspace,
                            workspace_bytes)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_hold_fft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint32_t traces, char *buf,
                          uint64_t len)
{
    int rc = bhwp_hold_fft_checks(p, length, s, flags, 0.0, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, false);
    if (!rc) rc = bhwp_hold_traces_check(traces);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_hold_fft(p, t ? &t->c : nullptr, length, s, flags, traces, buf, len);
}

uint64_t bhw_hold_mfft_workspace_bytes(const bhw_stft *s)
{
    return s && s->struct_size == sizeof(bhw_stft) ? bhwp_hold_mfft_workspace_bytes(s) : 0;
}

int bhw_hold_mfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags, double scale,
                             uint32_t psd_flags, const float *d_x, float *d_max, float *d_min, uint64_t p_stride, void *workspace, uint64_t workspace_bytes)
{
    return hold_mfft_run(nullptr, p, length, device, hip_stream, s, flags, scale, psd_flags, d_x, d_max, d_min, p_stride, workspace,
                         workspace_bytes);
}

int bhw_hold_mfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags, double scale,
                                 uint32_t psd_flags, const float *d_x, float *d_max, float *d_min, uint64_t p_stride, void *workspace, uint64_t workspace_bytes)
{
    const int rc = bhwp_hold_mfft_checks(p, length, s, flags, scale, psd_flags, p_stride, d_x, d_max, d_min, workspace, workspace_bytes);
    if (rc) return rc;
    return t ? hold_mfft_run(t, p, length, t->device, hip_stream, s, flags, scale, psd_flags, d_x, d_max, d_min, p_stride, workspace,
                             workspace_bytes)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_hold_mfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, uint32_t traces, char *buf,
                           uint64_t len)
{
    int rc = bhwp_hold_mfft_checks(p, length, s, flags, 0.0, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, false);
    if (!rc) rc = bhwp_hold_traces_check(traces);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_hold_mfft(p, t ? &t->c : nullptr, length, s, flags, traces, buf, len);
}

// ---- mixed-radix fused window and real FFT (include/bhw.h: bhw_stft_mfft_f32_device ...) -----------------------------------------------

int bhw_stft_mfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                             const bhw_fbank *fb, const float *d_x, float *d_out)
{
    return stft_mfft_run(nullptr, p, length, device, hip_stream, s, flags, fb, d_x, d_out);
}

int bhw_stft_mfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                 const bhw_fbank *fb, const float *d_x, float *d_out)
{
    const int rc = bhwp_stft_mfft_checks(p, length, s, flags, fb, d_x, d_out);
    if (rc) return rc;
    return t ? stft_mfft_run(t, p, length, t->device, hip_stream, s, flags, fb, d_x, d_out) : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_stft_mfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                           char *buf, uint64_t len)
{
    int rc = bhwp_stft_mfft_checks(p, length, s, flags, fb, nullptr, nullptr, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_stft_mfft(p, t ? &t->c : nullptr, length, s, flags, fb, buf, len);
}

// ---- fused window and complex FFT for I/Q input (include/bhw.h: bhw_stft_cfft_f32_device ...) ------------------------------------------

int bhw_stft_cfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                             const void *d_x, void *d_Y)
{
    return stft_cfft_run(nullptr, p, length, device, hip_stream, s, flags, (const float *)d_x, (float *)d_Y);
}

int bhw_stft_cfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                 const void *d_x, void *d_Y)
{
    const int rc = bhwp_stft_cfft_checks(p, length, s, flags, d_x, d_Y);
    if (rc) return rc;
    return t ? stft_cfft_run(t, p, length, t->device, hip_stream, s, flags, (const float *)d_x, (float *)d_Y)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_stft_cfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len)
{
    int rc = bhwp_stft_cfft_checks(p, length, s, flags, nullptr, nullptr, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_stft_cfft(p, t ? &t->c : nullptr, length, s, flags, buf, len);
}

// ---- mixed-radix fused window and complex FFT for I/Q input (include/bhw.h: bhw_stft_cmfft_f32_device ...) ----------------------------

int bhw_stft_cmfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                              const void *d_x, void *d_Y)
{
    return stft_cmfft_run(nullptr, p, length, device, hip_stream, s, flags, (const float *)d_x, (float *)d_Y);
}

int bhw_stft_cmfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                  const void *d_x, void *d_Y)
{
    const int rc = bhwp_stft_cmfft_checks(p, length, s, flags, d_x, d_Y);
    if (rc) return rc;
    return t ? stft_cmfft_run(t, p, length, t->device, hip_stream, s, flags, (const float *)d_x, (float *)d_Y)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_stft_cmfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len)
{
    int rc = bhwp_stft_cmfft_checks(p, length, s, flags, nullptr, nullptr, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_stft_cmfft(p, t ? &t->c : nullptr, length, s, flags, buf, len);
}

// ---- fused inverse real FFT, window and overlap-add (include/bhw.h: bhw_istft_fft_f32_device ...) --------------------------------------

int bhw_istft_fft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                             const float *d_Y, float *d_x)
{
    return istft_fft_run(nullptr, p, length, device, hip_stream, s, flags, d_Y, d_x);
}

int bhw_istft_fft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                 const float *d_Y, float *d_x)
{
    const int rc = bhwp_istft_fft_checks(p, length, s, flags, d_Y, d_x);
    if (rc) return rc;
    return t ? istft_fft_run(t, p, length, t->device, hip_stream, s, flags, d_Y, d_x) : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_istft_fft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len)
{
    int rc = bhwp_istft_fft_checks(p, length, s, flags, nullptr, nullptr, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_istft_fft(p, t ? &t->c : nullptr, length, s, flags, buf, len);
}

// ---- fused STFT, spectral mask and inverse STFT (include/bhw.h: bhw_mask_fft_f32_device ...) --------------------------------------------

int bhw_mask_fft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                            uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out)
{
    return mask_fft_run(nullptr, p, length, device, hip_stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
}

int bhw_mask_fft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                                uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride,
                                float *d_out)
{
    const int rc = bhwp_mask_fft_checks(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
    if (rc) return rc;
    return t ? mask_fft_run(t, p, length, t->device, hip_stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_mask_fft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                          uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len)
{
    int rc = bhwp_mask_fft_checks(p, length, sa, ss, flags, nullptr, nullptr, g_stride, g_batch_stride, nullptr, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_mask_fft(p, t ? &t->c : nullptr, length, sa, ss, flags, g_stride, g_batch_stride, buf, len);
}

// ---- fused STFT, spectral mask and inverse STFT at mixed-radix n_fft (include/bhw.h: bhw_mask_mfft_f32_device ...) -------------------------

int bhw_mask_mfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                             uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out)
{
    return mask_mfft_run(nullptr, p, length, device, hip_stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
}

int bhw_mask_mfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                                 uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride,
                                 float *d_out)
{
    const int rc = bhwp_mask_mfft_checks(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
    if (rc) return rc;
    return t ? mask_mfft_run(t, p, length, t->device, hip_stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_mask_mfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                           uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len)
{
    int rc = bhwp_mask_mfft_checks(p, length, sa, ss, flags, nullptr, nullptr, g_stride, g_batch_stride, nullptr, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_mask_mfft(p, t ? &t->c : nullptr, length, sa, ss, flags, g_stride, g_batch_stride, buf, len);
}

// ---- fused STFT, complex spectral gain and inverse STFT (include/bhw.h: bhw_cmask_fft_f32_device ...) ----------------------------------

int bhw_cmask_fft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                             uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out)
{
    return cmask_fft_run(nullptr, p, length, device, hip_stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
}

int bhw_cmask_fft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                                 uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride,
                                 float *d_out)
{
    const int rc = bhwp_cmask_fft_checks(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
    if (rc) return rc;
    return t ? cmask_fft_run(t, p, length, t->device, hip_stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_cmask_fft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                           uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len)
{
    int rc = bhwp_cmask_fft_checks(p, length, sa, ss, flags, nullptr, nullptr, g_stride, g_batch_stride, nullptr, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_cmask_fft(p, t ? &t->c : nullptr, length, sa, ss, flags, g_stride, g_batch_stride, buf, len);
}

// ---- fused STFT, complex spectral gain and inverse STFT at mixed-radix n_fft (include/bhw.h: bhw_cmask_mfft_f32_device ...) ---------------

int bhw_cmask_mfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                              uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out)
{
    return cmask_mfft_run(nullptr, p, length, device, hip_stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
}

int bhw_cmask_mfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,
                                  uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride,
                                  float *d_out)
{
    const int rc = bhwp_cmask_mfft_checks(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);
    if (rc) return rc;
    return t ? cmask_mfft_run(t, p, length, t->device, hip_stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_cmask_mfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,
                            uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len)
{
    int rc = bhwp_cmask_mfft_checks(p, length, sa, ss, flags, nullptr, nullptr, g_stride, g_batch_stride, nullptr, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_cmask_mfft(p, t ? &t->c : nullptr, length, sa, ss, flags, g_stride, g_batch_stride, buf, len);
}

// ---- fused STFT, real or complex gain per bin and inverse STFT for I/Q input (include/bhw.h: bhw_mask_cfft_f32_device ...) -------------
// The three entry points of each of the four calls, in the shape of the ones above: NAME in {mask_cfft, cmask_cfft, mask_cmfft,
// cmask_cmfft}.
#define BHW_MASK_IQ_ENTRIES(NAME)                                                                                                               \
    int bhw_##NAME##_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,      \
                                uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride, uint64_t g_batch_stride, float *d_out)    \
    {                                                                                                                                           \
        return NAME##_run(nullptr, p, length, device, hip_stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);                    \
    }                                                                                                                                           \
    int bhw_##NAME##_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa,                     \
                                    const bhw_stft *ss, uint32_t flags, const float *d_x, const float *d_g, uint64_t g_stride,                   \
                                    uint64_t g_batch_stride, float *d_out)                                                                       \
    {                                                                                                                                           \
        const int rc = bhwp_##NAME##_checks(p, length, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out);                               \
        if (rc) return rc;                                                                                                                      \
        return t ? NAME##_run(t, p, length, t->device, hip_stream, sa, ss, flags, d_x, d_g, g_stride, g_batch_stride, d_out)                    \
                 : fail(BHW_ERR_BADARG, "table is NULL");                                                                                       \
    }                                                                                                                                           \
    int bhw_describe_##NAME(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,           \
                            uint64_t g_stride, uint64_t g_batch_stride, char *buf, uint64_t len)                                                 \
    {                                                                                                                                           \
        int rc = bhwp_##NAME##_checks(p, length, sa, ss, flags, nullptr, nullptr, g_stride, g_batch_stride, nullptr, false);                    \
        if (!rc && t) rc = table_call_checks(t, p);                                                                                             \
        return rc ? rc : bhwp_describe_##NAME(p, t ? &t->c : nullptr, length, sa, ss, flags, g_stride, g_batch_stride, buf, len);                \
    }
BHW_MASK_IQ_ENTRIES(mask_cfft)
BHW_MASK_IQ_ENTRIES(cmask_cfft)
BHW_MASK_IQ_ENTRIES(mask_cmfft)
BHW_MASK_IQ_ENTRIES(cmask_cmfft)
#undef BHW_MASK_IQ_ENTRIES

// ---- fused multichannel filter-and-sum (include/bhw.h: bhw_beam_fft_f32_device ..., bhw_beam_mfft_f32_device ...) -------------------------
// The three entry points of each family, in the shape of the ones above: NAME in {beam_fft, beam_mfft}.
#define BHW_BEAM_ENTRIES(NAME)                                                                                                                  \
    int bhw_##NAME##_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *sa, const bhw_stft *ss,      \
                                uint32_t flags, const float *d_x, uint32_t n_ch, uint64_t x_ch_stride, const float *d_g, uint64_t g_stride,     \
                                uint64_t g_ch_stride, uint64_t g_batch_stride, float *d_out)                                                     \
    {                                                                                                                                           \
        const BhwBeamAxis ch{n_ch, x_ch_stride, g_ch_stride};                                                                                   \
        return NAME##_run(nullptr, p, length, device, hip_stream, sa, ss, flags, d_x, ch, d_g, g_stride, g_batch_stride, d_out);                \
    }                                                                                                                                           \
    int bhw_##NAME##_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *sa,                     \
                                    const bhw_stft *ss, uint32_t flags, const float *d_x, uint32_t n_ch, uint64_t x_ch_stride,                   \
                                    const float *d_g, uint64_t g_stride, uint64_t g_ch_stride, uint64_t g_batch_stride, float *d_out)            \
    {                                                                                                                                           \
        const BhwBeamAxis ch{n_ch, x_ch_stride, g_ch_stride};                                                                                   \
        const int rc = bhwp_##NAME##_checks(p, length, sa, ss, flags, d_x, ch, d_g, g_stride, g_batch_stride, d_out);                           \
        if (rc) return rc;                                                                                                                      \
        return t ? NAME##_run(t, p, length, t->device, hip_stream, sa, ss, flags, d_x, ch, d_g, g_stride, g_batch_stride, d_out)                \
                 : fail(BHW_ERR_BADARG, "table is NULL");                                                                                       \
    }                                                                                                                                           \
    int bhw_describe_##NAME(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *sa, const bhw_stft *ss, uint32_t flags,           \
                            uint32_t n_ch, uint64_t x_ch_stride, uint64_t g_stride, uint64_t g_ch_stride, uint64_t g_batch_stride, char *buf,    \
                            uint64_t len)                                                                                                       \
    {                                                                                                                                           \
        const BhwBeamAxis ch{n_ch, x_ch_stride, g_ch_stride};                                                                                   \
        int rc = bhwp_##NAME##_checks(p, length, sa, ss, flags, nullptr, ch, nullptr, g_stride, g_batch_stride, nullptr, false);                \
        if (!rc && t) rc = table_call_checks(t, p);                                                                                             \
        return rc ? rc : bhwp_describe_##NAME(p, t ? &t->c : nullptr, length, sa, ss, flags, ch, g_stride, g_batch_stride, buf, len);            \
    }
BHW_BEAM_ENTRIES(beam_fft)
BHW_BEAM_ENTRIES(beam_mfft)
#undef BHW_BEAM_ENTRIES

// ---- fused log spectrogram, log-mel and MFCC (include/bhw.h: bhw_logspec_f32_device ..., bhw_logspec_mfft_f32_device ...) -------------

int bhw_logspec_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                           const bhw_fbank *fb, const bhw_logspec *ls, const float *d_x, float *d_out)
{
    return logspec_run(false, nullptr, p, length, device, hip_stream, s, flags, fb, ls, d_x, d_out);
}

int bhw_logspec_mfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                const bhw_fbank *fb, const bhw_logspec *ls, const float *d_x, float *d_out)
{
    return logspec_run(true, nullptr, p, length, device, hip_stream, s, flags, fb, ls, d_x, d_out);
}

static int logspec_from_table(bool mixed, bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s,
                              uint32_t flags, const bhw_fbank *fb, const bhw_logspec *ls, const float *d_x, float *d_out)
{
    const int rc = bhwp_logspec_checks(mixed, p, length, s, flags, fb, ls, d_x, d_out);
    if (rc) return rc;
    return t ? logspec_run(mixed, t, p, length, t->device, hip_stream, s, flags, fb, ls, d_x, d_out) : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_logspec_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                               const bhw_fbank *fb, const bhw_logspec *ls, const float *d_x, float *d_out)
{
    return logspec_from_table(false, t, p, length, hip_stream, s, flags, fb, ls, d_x, d_out);
}

int bhw_logspec_mfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                    const bhw_fbank *fb, const bhw_logspec *ls, const float *d_x, float *d_out)
{
    return logspec_from_table(true, t, p, length, hip_stream, s, flags, fb, ls, d_x, d_out);
}

static int describe_logspec(bool mixed, bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags,
                            const bhw_fbank *fb, const bhw_logspec *ls, char *buf, uint64_t len)
{
    int rc = bhwp_logspec_checks(mixed, p, length, s, flags, fb, ls, nullptr, nullptr, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_logspec(mixed, p, t ? &t->c : nullptr, length, s, flags, fb, ls, buf, len);
}

int bhw_describe_logspec(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                         const bhw_logspec *ls, char *buf, uint64_t len)
{
    return describe_logspec(false, t, p, length, s, flags, fb, ls, buf, len);
}

int bhw_describe_logspec_mfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_fbank *fb,
                              const bhw_logspec *ls, char *buf, uint64_t len)
{
    return describe_logspec(true, t, p, length, s, flags, fb, ls, buf, len);
}

// ---- fused inverse mixed-radix FFT, window and overlap-add (include/bhw.h: bhw_istft_mfft_f32_device ...) ------------------------------

int bhw_istft_mfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                              const float *d_Y, float *d_x)
{
    return istft_mfft_run(nullptr, p, length, device, hip_stream, s, flags, d_Y, d_x);
}

int bhw_istft_mfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                  const float *d_Y, float *d_x)
{
    const int rc = bhwp_istft_mfft_checks(p, length, s, flags, d_Y, d_x);
    if (rc) return rc;
    return t ? istft_mfft_run(t, p, length, t->device, hip_stream, s, flags, d_Y, d_x) : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_istft_mfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len)
{
    int rc = bhwp_istft_mfft_checks(p, length, s, flags, nullptr, nullptr, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_istft_mfft(p, t ? &t->c : nullptr, length, s, flags, buf, len);
}

// ---- fused inverse complex FFT, window and overlap-add for I/Q output (include/bhw.h: bhw_istft_cfft_f32_device ...) --------------------

int bhw_istft_cfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                              const float *d_Y, float *d_x)
{
    return istft_cfft_run(nullptr, p, length, device, hip_stream, s, flags, d_Y, d_x);
}

int bhw_istft_cfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                  const float *d_Y, float *d_x)
{
    const int rc = bhwp_istft_cfft_checks(p, length, s, flags, d_Y, d_x);
    if (rc) return rc;
    return t ? istft_cfft_run(t, p, length, t->device, hip_stream, s, flags, d_Y, d_x) : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_istft_cfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len)
{
    int rc = bhwp_istft_cfft_checks(p, length, s, flags, nullptr, nullptr, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_istft_cfft(p, t ? &t->c : nullptr, length, s, flags, buf, len);
}

// ---- fused inverse mixed-radix complex FFT, window and overlap-add for I/Q output (include/bhw.h: bhw_istft_cmfft_f32_device ...) -------

int bhw_istft_cmfft_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                               const float *d_Y, float *d_x)
{
    return istft_cmfft_run(nullptr, p, length, device, hip_stream, s, flags, d_Y, d_x);
}

int bhw_istft_cmfft_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                   const float *d_Y, float *d_x)
{
    const int rc = bhwp_istft_cmfft_checks(p, length, s, flags, d_Y, d_x);
    if (rc) return rc;
    return t ? istft_cmfft_run(t, p, length, t->device, hip_stream, s, flags, d_Y, d_x) : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_describe_istft_cmfft(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, char *buf, uint64_t len)
{
    int rc = bhwp_istft_cmfft_checks(p, length, s, flags, nullptr, nullptr, false);
    if (!rc && t) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_istft_cmfft(p, t ? &t->c : nullptr, length, s, flags, buf, len);
}

// ---- Welch's method (include/bhw.h: bhw_window_sums_device ...) ------------------------------------------------------------------------

int bhw_window_sums_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, uint32_t flags, uint64_t *d_sums)
{
    return window_sums_run(nullptr, p, length, device, hip_stream, flags, d_sums);
}

int bhw_window_sums_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, uint32_t flags, uint64_t *d_sums)
{
    const int rc = bhwp_sums_checks(p, length, flags, d_sums);
    if (rc) return rc;
    return t ? window_sums_run(t, p, length, t->device, hip_stream, flags, d_sums) : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_welch_frames_f32_device(const bhw_params *p, uint64_t length, int device, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                const float *d_x, float *d_y, void *workspace, uint64_t workspace_bytes)
{
    return welch_frames_run(nullptr, p, length, device, hip_stream, s, flags, d_x, d_y, workspace, workspace_bytes);
}

int bhw_welch_frames_f32_from_table(bhw_table t, const bhw_params *p, uint64_t length, void *hip_stream, const bhw_stft *s, uint32_t flags,
                                    const float *d_x, float *d_y, void *workspace, uint64_t workspace_bytes)
{
    const int rc = bhwp_welch_checks(p, length, s, flags, d_x, d_y, workspace, workspace_bytes);
    if (rc) return rc;
    return t ? welch_frames_run(t, p, length, t->device, hip_stream, s, flags, d_x, d_y, workspace, workspace_bytes)
             : fail(BHW_ERR_BADARG, "table is NULL");
}

int bhw_welch_psd_f32(int device, void *hip_stream, const bhw_psd *d, const float *d_Y, float *d_P, void *workspace, uint64_t workspace_bytes)
{
    const int rc = bhwp_psd_checks(d, d_Y, d_P, workspace, workspace_bytes);
    if (rc) return rc;
    const BhwPsdPlan pl = bhwp_psd_plan(d);
    DeviceGuard guard(device);
    if (const int g = guard.status()) return g;
    const int e = bhwk_welch_psd_f32(BhwLaunch{device, hip_stream}, pl, d, d_Y, d_P, (double *)workspace);
    return e ? fail_hip(e, "welch psd launch") : BHW_OK;
}

int bhw_describe_welch(bhw_table t, const bhw_params *p, uint64_t length, const bhw_stft *s, uint32_t flags, const bhw_psd *d, char *buf,
                       uint64_t len)
{
    if (s && d) return fail(BHW_ERR_BADARG, "pass the segments descriptor or the periodogram descriptor, not both");
    int rc;
    if (d) rc = bhwp_psd_checks(d, nullptr, nullptr, nullptr, 0, false);
    else if (s) rc = bhwp_welch_checks(p, length, s, flags, nullptr, nullptr, nullptr, 0, false);
    else rc = bhwp_sums_checks(p, length, flags, nullptr, false);
    if (!rc && t && !d) rc = table_call_checks(t, p);
    return rc ? rc : bhwp_describe_welch(p, t && !d ? &t->c : nullptr, length, s, flags, d, buf, len);
}

int bhw_welch_csd_f32(int device, void *hip_stream, const bhw_csd *d, const float *d_X, const float *d_Y, float *d_Pxy, float *d_Pxx,
                      float *d_Pyy, float *d_Cxy, float *d_H1, void *workspace, uint64_t workspace_bytes)
{
    float *const outs[kCsdOutputs] = {d_Pxy, d_Pxx, d_Pyy, d_Cxy, d_H1};
    const int rc = bhwp_csd_checks(d, d_X, d_Y, (const void *const *)outs, workspace, workspace_bytes);
    if (rc) return rc;
    const BhwCsdPlan pl = bhwp_csd_plan(d);
    DeviceGuard guard(device);
    if (const int g = guard.status()) return g;
    const int e = bhwk_welch_csd_f32(BhwLaunch{device, hip_stream}, pl, d, d_X, d_Y, outs, (double *)workspace);
    return e ? fail_hip(e, "welch csd launch") : BHW_OK;
}

// Development hook (not part of the ABI in include/bhw.h): on != 0 sends the *_len calls at L = 2^phi_width to the any-length kernels
// as well (process-wide), so that tests can compare them with the power-of-two kernels.  Returns the previous setting.
int bhw_dbg_len_force_kernels(int on) { return g_len_force.exchange(on != 0) ? 1 : 0; }

} // extern "C"
