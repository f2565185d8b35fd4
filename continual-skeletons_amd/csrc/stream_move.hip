// stream_move.hip -- copy the live state of SOME streams between the continual slab and a packed buffer
// (csk_co_move_streams_f32, include/cskel.h).  One launch takes a table of jobs
// (ring, the slot of its newest live frame, how many newest slots to move, offset inside a stream's packed record) and a
// device list of stream indices; record j of the packed buffer pairs with stream streams[j].  Export reads the rings and
// writes the records, import reads the records and writes -- in every row of the window's slots -- the segments of the named
// streams and nothing else: not the neighbouring streams, not the P-padding, not the slots outside the window.  The words
// are moved as 32-bit patterns (the flags are int32, the latched rotations fp64 halves).  HBM-bound loads and stores only.
// The window's device form, the host checks of a ring job, the grid and the walk over the segments are stream_jobs.h
// (shared with stream_reset.hip); this file has the entry, the record side and what is done to a segment.
#include "stream_jobs.h"

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// device form of a job: the window as a slot run, oldest slot first, and where it stands in a record: (i * rows + row) * seg
struct MoveJob {
    SlotRun run;
    int64_t offset;
};
struct MoveTable {
    MoveJob job[CSK_CO_MOVE_MAX_JOBS];
};

// Copy src[0 .. len) to dst[0 .. len); 16 lanes (`sub` = 0..15) share one segment.  Both are 4-byte aligned and nothing
// more: a segment is M * V words (50, 36), so its alignment changes from stream to stream on the ring side and from job to
// job on the packed side.  The STORES decide the shape: up to 3 single words lead to dst's first 16-byte boundary, 16-byte
// stores cover the body, up to 3 words trail.  The body's loads are as wide as src allows at that point: 16 bytes when src
// is 16-byte aligned there, two 8-byte loads when it is 8-byte aligned (every second NTU stream), else four words.
__device__ __forceinline__ void copy_segment(uint32_t *dst, const uint32_t *src, int len, int sub) {
    const int head = (int)((4u - ((unsigned)(reinterpret_cast<uintptr_t>(dst) >> 2) & 3u)) & 3u);
    if (head > len) {                                   // shorter than its own head (len <= 2): single words
        if (sub == 0)
            for (int i = 0; i < len; ++i) dst[i] = src[i];
        return;
    }
    if (sub == 0)
        for (int i = 0; i < head; ++i) dst[i] = src[i];
    uint32_t *db = dst + head;
    const uint32_t *sb = src + head;
    const int nb = (len - head) >> 2, tail = (len - head) & 3;
    const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(sb) >> 2) & 3u;
    if (mis == 0) {
        for (int i = sub; i < nb; i += 16) *reinterpret_cast<u32x4 *>(db + 4 * i) = *reinterpret_cast<const u32x4 *>(sb + 4 * i);
    } else if (mis == 2) {
        for (int i = sub; i < nb; i += 16) {
            const u32x2 a = *reinterpret_cast<const u32x2 *>(sb + 4 * i), b = *reinterpret_cast<const u32x2 *>(sb + 4 * i + 2);
            *reinterpret_cast<u32x4 *>(db + 4 * i) = u32x4{a.x, a.y, b.x, b.y};
        }
    } else {
        for (int i = sub; i < nb; i += 16) {
            const uint32_t *s = sb + 4 * i;
            *reinterpret_cast<u32x4 *>(db + 4 * i) = u32x4{s[0], s[1], s[2], s[3]};
        }
    }
    if (sub == 15)
        for (int i = 0; i < tail; ++i) db[4 * nb + i] = sb[4 * nb + i];
}

// grid: y = job, x walks the window's segments (walk_segments, stream_jobs.h) and copies each from or to its place in
// record k.
__global__ __launch_bounds__(256) void move_streams_kernel(const MoveTable t, uint32_t *__restrict__ packed, int64_t record_words,
                                                           const int32_t *__restrict__ streams, int n_streams, int n_total,
                                                           int to_ring) {
    const MoveJob &j = t.job[blockIdx.y];
    walk_segments(j.run, streams, n_streams, n_total, [&](int k, int i, int row, uint32_t *in_ring, int seg, int sub) {
        uint32_t *in_record = packed + (int64_t)k * record_words + j.offset + ((int64_t)i * j.run.rows + row) * seg;
        if (to_ring)
            copy_segment(in_ring, in_record, seg, sub);
        else
            copy_segment(in_record, in_ring, seg, sub);
    });
}

extern "C" int csk_co_move_streams_f32(const csk_move_job *jobs, int n_jobs, void *packed, int64_t record_floats, const int32_t *streams,
                                       int n_streams, int n_total, int to_ring, void *stream) {
    if (!jobs) CSK_FAIL("co_move_streams: null pointer (jobs)");
    if (n_jobs < 1 || n_jobs > CSK_CO_MOVE_MAX_JOBS) CSK_FAIL("co_move_streams: 1..%d jobs per launch, got %d", CSK_CO_MOVE_MAX_JOBS, n_jobs);
    if (n_streams < 0) CSK_FAIL("co_move_streams: n_streams < 0");
    if (n_total < 1) CSK_FAIL("co_move_streams: the slab holds n_total >= 1 streams, got %d", n_total);
    if (record_floats < 1) CSK_FAIL("co_move_streams: a record of %lld floats", (long long)record_floats);
    if (to_ring != 0 && to_ring != 1) CSK_FAIL("co_move_streams: to_ring is 0 (export) or 1 (import), got %d", to_ring);
    if (n_streams > 0 && (!streams || !packed)) CSK_FAIL("co_move_streams: null pointer (streams, packed)");
    if (reinterpret_cast<uintptr_t>(packed) & 3) CSK_FAIL("co_move_streams: the packed buffer is not 4-byte aligned");
    MoveTable t;
    int n = 0;
    int64_t most = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const csk_move_job &s = jobs[i];
        SlotRun &d = t.job[n].run;
        const auto run_of_job = [&](SlotRun &run) {     // this entry's own checks: the window, as a run from its oldest slot
            if (s.newest < 0 || s.newest >= s.depth) CSK_FAIL("co_move_streams: newest slot %d of job %d outside a ring of %d slots", s.newest, i, s.depth);
            if (s.window < 0 || s.window > s.depth)
                CSK_FAIL("co_move_streams: a window of %d slots in job %d is longer than the ring (%d slots)", s.window, i, s.depth);
            run.slot0 = s.newest + 1 - s.window;        // > -depth
            if (run.slot0 < 0) run.slot0 += s.depth;
            run.n_slots = s.window;
            return 0;
        };
        if (resolve_ring_job("co_move_streams", i, s.kind, s.ring, s.row_floats, s.depth, s.rows, s.seg, n_total, d, run_of_job)) return -1;
        const int64_t words = run_segments(d, 1) * d.seg;
        if (s.offset < 0 || s.offset + words > record_floats)
            CSK_FAIL("co_move_streams: job %d covers floats [%lld, %lld) of a record of %lld", i, (long long)s.offset,
                     (long long)(s.offset + words), (long long)record_floats);
        t.job[n].offset = s.offset;
        if (d.n_slots == 0) continue;                   // an empty window: nothing to launch for it
        if (run_segments(d, n_streams) > most) most = run_segments(d, n_streams);
        ++n;
    }
    if (n == 0 || n_streams == 0) return 0;
    hipLaunchKernelGGL(move_streams_kernel, table_grid(t.job, n, most, 16, 4096), dim3(256), 0, (hipStream_t)stream, t,
                       reinterpret_cast<uint32_t *>(packed), record_floats, streams, n_streams, n_total, to_ring);
    return (int)hipGetLastError();
}
