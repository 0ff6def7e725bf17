// bhw_ola.h -- the lane structure of the weighted overlap-add, shared by its int32 (bhw_ola.hip) and float32 (bhw_ola_f32.h) kernels:
// the launch arguments, the residue and rows of a lane, the frames that reach them, and the host side that fills the arguments.
//
// Output t = q * hop + r.  A lane owns one residue r and a block of Q consecutive hops; lane s is numbered from t0 (it holds the
// residue of t0 + s).  For the rows of one workgroup row block it sums the products of frames f = q - j, j in [jlo, jhi]; the trip
// count it reports is its own, and the kernels run the wave's largest with the other lanes masked.
//   - Both kernels take their arguments from OlaIo / ola_args and their trip count from wave_max.
//   - ola_lane / ola_rows are the lane arithmetic of bhw_ola.hip's ola_loop, statement for statement.  The float32 loop calls them;
//     the int32 loop keeps its inline form, because calling them there reorders the gfx950 code of all 288 int32 instances (same
//     instructions, another schedule), and those instruction streams are kept identical.  tests/cpp/san_ola.cpp and san_f32.cpp replay
//     the two.
#pragma once
#include "bhw_device.h"

namespace {

// The launch arguments of an overlap-add kernel whose samples are of type E (int32_t or float).
template <typename E>
struct OlaIo {
    const E *y;
    E *x;
    uint64_t n;          // N = 2^phi_width, or the length L of a window of any length
    uint64_t frames, hop, y_stride, count;
    uint64_t lanes;      // residues in use: min(hop, count)
    uint64_t rows;       // ceil(count / hop)
    uint64_t row_blocks; // workgroup rows of fy * Q hops
    uint64_t q0, r0;     // t0 = q0 * hop + r0
    uint64_t rlim;       // residues r < rlim are reached by jmax frames, r in [rlim, N) by jmax - 1, r >= N by none
    int64_t jmax;        // ceil(N / hop)
    uint32_t rx;         // lanes along the residue (a power of two)
    uint32_t fy;         // rows side by side in a workgroup: kOlaBlock / rx
    uint32_t q;          // Q: hops of one lane, 1..kOlaQMax
    uint32_t shift;
    uint32_t io;         // 0: one channel; 1: two channels, 4-byte accesses; 2: two channels, one 8-byte access
};

__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m));
    return v;
}

// The residue of this lane: s (numbered from t0), ok (s < lanes), r and the hop qb of t0 + s, and jr, the frames that reach the
// residue (j < jr).
struct OlaLane {
    uint64_t s, r;
    int64_t qb, jr;
    bool ok;
};

template <typename E>
__device__ __forceinline__ OlaLane ola_lane(const OlaIo<E> &a)
{
    OlaLane ln;
    ln.s = (uint64_t)blockIdx.x * a.rx + (threadIdx.x & (a.rx - 1u));
    ln.ok = ln.s < a.lanes;
    ln.r = a.r0 + ln.s;                                            // s < hop: at most one wrap
    ln.qb = (int64_t)a.q0;
    if (ln.r >= a.hop) {
        ln.r -= a.hop;
        ++ln.qb;
    }
    ln.jr = (!ln.ok || ln.r >= a.n) ? 0 : (ln.r < a.rlim ? a.jmax : a.jmax - 1);
    return ln;
}

// The rows of this lane in row block `by` (frames: a.frames, read once by the caller): the first output u0 (count when none), nrow of them, the hop qa of the first row, and the
// frames that reach them, f = qa + i - j for j in [jlo, jhi] (trip = jhi - jlo + 1 of them, 0 when none).
struct OlaRows {
    uint64_t u0;
    int64_t qa, jlo, jhi;
    uint32_t nrow, trip;
};

template <typename E>
__device__ __forceinline__ OlaRows ola_rows(const OlaIo<E> &a, const OlaLane &ln, int64_t frames, uint64_t by, uint32_t ty)
{
    OlaRows rw;
    const uint64_t ia = (by * a.fy + ty) * a.q;                    // first row (hop index relative to t0) of this lane
    // rows of this lane with an output u = i * hop + s inside [0, count): a prefix of the Q rows (ia < rows keeps ia * hop below
    // count whatever the hop)
    rw.u0 = ia < a.rows ? ia * a.hop + ln.s : a.count;
    rw.nrow = 0;
    if (ln.ok && rw.u0 < a.count) {
        const uint64_t left = (a.count - rw.u0 - 1) / a.hop + 1;
        rw.nrow = left < a.q ? (uint32_t)left : a.q;
    }
    // frames that reach these rows: f = qb + i - j in [0, frames), j in [0, jr)
    rw.qa = ln.qb + (int64_t)ia;
    rw.jlo = rw.qa - frames + 1 > 0 ? rw.qa - frames + 1 : 0;
    rw.jhi = (rw.qa + (int64_t)rw.nrow - 1) < ln.jr - 1 ? rw.qa + (int64_t)rw.nrow - 1 : ln.jr - 1;
    rw.trip = (rw.nrow && rw.jhi >= rw.jlo) ? (uint32_t)(rw.jhi - rw.jlo + 1) : 0u;
    return rw;
}

// The arguments of a launch of plan pl for descriptor o (host side).
template <typename E>
inline void ola_args(OlaIo<E> &a, const BhwOlaPlan &pl, const bhw_ola *o, const E *d_y, E *d_x)
{
    a.y = d_y;
    a.x = d_x;
    a.n = pl.len;                                                  // N = 2^phi_width, or L
    a.frames = o->frames;
    a.hop = o->hop;
    a.y_stride = pl.y_stride;
    a.count = o->count;
    a.lanes = pl.lanes;
    a.rows = pl.rows;
    a.row_blocks = pl.row_blocks;
    a.q0 = pl.q0;
    a.r0 = pl.r0;
    a.jmax = (int64_t)pl.jmax;
    a.rlim = a.n - (pl.jmax - 1) * o->hop;                         // (jmax - 1) * hop < N (or L)
    a.rx = pl.rx;
    a.fy = pl.fy;
    a.q = pl.q;
    a.shift = o->shift;
    a.io = pair_io(o->channels, d_y, d_x, pl.y_stride);
}

} // namespace
