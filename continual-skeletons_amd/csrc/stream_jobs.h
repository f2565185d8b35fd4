// stream_jobs.h -- what the launches over "the segments of SOME streams in a run of slots of some rings" share
// (stream_reset.hip zeroes them, stream_move.hip copies them; stream_prime.hip takes the table / grid helper): the device
// form of a ring's slot run, the host resolver of a ring job of include/cskel.h, the grid of a by-value job table and the
// device walk over a run's segments.  What is done to a segment stays with each kernel.
#pragma once
#include "mfma_core.h"

// Both layouts of include/cskel.h reduce to "segment of stream n in row (slot, row) starts at
// (slot * rows + row) * row_stride + n * seg" (pooling ring [slots][N][C]: one row of N * C words per slot, seg = C).  The
// run is n_slots slots from slot0 on, wrapping at depth.  Words are 32-bit patterns.
struct SlotRun {
    uint32_t *ring;
    int64_t row_stride;
    int32_t depth, rows, slot0, n_slots, seg, pad_;
};

__host__ __device__ static inline int64_t run_segments(const SlotRun &d, int n_streams) { return (int64_t)d.n_slots * d.rows * n_streams; }

// Host: check job `i` of the entry `what` (the prefix of its messages) against a slab of n_total streams and fill `d`.
// `slots(d)` makes the entry's own checks of the run inside the ring -- behind the dims, in front of the kind -- sets
// d.slot0 / d.n_slots and returns 0, or fails as the entry does.
template <class Slots>
static inline int resolve_ring_job(const char *what, int i, int kind, void *ring, int64_t row_floats, int depth, int rows, int seg,
                                   int n_total, SlotRun &d, Slots slots) {
    if (!ring) CSK_FAIL("%s: null pointer (ring of job %d)", what, i);
    if (reinterpret_cast<uintptr_t>(ring) & 3) CSK_FAIL("%s: ring of job %d is not 4-byte aligned", what, i);
    if (depth < 1 || rows < 1 || seg < 1 || row_floats < 1) CSK_FAIL("%s: bad dims in job %d", what, i);
    if (slots(d)) return -1;
    d.ring = static_cast<uint32_t *>(ring), d.depth = depth, d.seg = seg, d.pad_ = 0;
    if (kind == CSK_SCRUB_BLOCK_RING) {
        if ((int64_t)n_total * seg > row_floats)
            CSK_FAIL("%s: %d streams of %d floats cannot fit a row of %lld floats (job %d)", what, n_total, seg, (long long)row_floats, i);
        d.row_stride = row_floats, d.rows = rows;
    } else if (kind == CSK_SCRUB_POOL_RING) {
        if (rows != n_total || seg != row_floats)
            CSK_FAIL("%s: a pooling ring has one row of seg = row_floats floats per stream (job %d: rows %d, slab %d)", what, i, rows,
                     n_total);
        d.row_stride = (int64_t)rows * row_floats, d.rows = 1;
    } else {
        CSK_FAIL("%s: unknown ring kind %d in job %d", what, kind, i);
    }
    return 0;
}

// Host: the grid of a launch over a by-value table of which the first n entries are used -- y = entry, x = the blocks the
// largest entry wants (`most` work items, `per_block` of them to a block), at most `cap`.  The entries behind n are never
// indexed; they are filled so that the table is defined.
template <class Job, int MAX>
static inline dim3 table_grid(Job (&job)[MAX], int n, int64_t most, int per_block, int64_t cap) {
    for (int i = n; i < MAX; ++i) job[i] = job[0];
    const int64_t want = (most + per_block - 1) / per_block;
    return dim3((unsigned)(want < cap ? want : cap), (unsigned)n);
}

// Device: grid x strides over the run's segments (slot of the run, row, listed stream -- streams fastest, so neighbouring
// 16-lane groups touch neighbouring parts of one row); 16 lanes (`sub` = 0..15) share one segment.  A stream index outside
// [0, n_total) is skipped.  f(k, i, row, p, seg, sub): listed stream k, slot i of the run, p = the segment in the ring.
template <class F>
__device__ __forceinline__ void walk_segments(const SlotRun &j, const int32_t *__restrict__ streams, int n_streams, int n_total, F f) {
    const int sub = threadIdx.x & 15;
    const int64_t total = run_segments(j, n_streams);
    for (int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4; g < total; g += (int64_t)gridDim.x * 16) {
        const int k = (int)(g % n_streams);
        const int64_t q = g / n_streams;
        const int row = (int)(q % j.rows), i = (int)(q / j.rows);
        int slot = j.slot0 + i;
        if (slot >= j.depth) slot -= j.depth;
        const int n = streams[k];
        if (n < 0 || n >= n_total) continue;
        f(k, i, row, j.ring + ((int64_t)slot * j.rows + row) * j.row_stride + (int64_t)n * j.seg, j.seg, sub);
    }
}
