// stream_reset.hip -- zero the state of SOME streams of the continual slab (csk_co_scrub_streams_f32, include/cskel.h).
// One launch takes a table of jobs (ring, run of slots) and a device list of stream indices and zeroes, in every row of
// every slot of each run, the segments of those streams -- nothing else: not the neighbouring streams, not the P-padding
// behind the last one.  Two uses (co_reset.py): the full reset of a stream (all slots of every ring) and the per-cycle
// scrub of what the not-yet-live blocks wrote for a warming stream (the slots one cycle wrote).  HBM-bound stores only.
// The job's device form, its host checks, the grid and the walk over the segments are stream_jobs.h (shared with
// stream_move.hip); this file has the entry and what is done to a segment.
#include "stream_jobs.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct ScrubTable {
    SlotRun job[CSK_CO_SCRUB_MAX_JOBS];
};

// Zero p[0 .. len) with the widest stores its alignment allows; 16 lanes (`sub` = 0..15) share one segment.  p is 4-byte
// aligned: up to 3 floats lead to the first 16-byte boundary (one 4-byte store, one 8-byte store or both -- after an odd
// float the address is 8-byte aligned), 16-byte stores cover the body, up to 3 floats trail (8-byte, then 4-byte).
__device__ __forceinline__ void zero_segment(float *p, int len, int sub) {
    const int head = (int)((4u - ((unsigned)(reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3u);
    if (head > len) {                                   // shorter than its own head (len <= 2): scalars
        if (sub == 0)
            for (int i = 0; i < len; ++i) p[i] = 0.f;
        return;
    }
    if (sub == 0) {
        if (head & 1) p[0] = 0.f;
        if (head & 2) *reinterpret_cast<f32x2 *>(p + (head & 1)) = f32x2{0.f, 0.f};
    }
    float *body = p + head;
    const int nb = (len - head) >> 2, tail = (len - head) & 3;
    for (int i = sub; i < nb; i += 16) *reinterpret_cast<f32x4 *>(body + 4 * i) = f32x4{0.f, 0.f, 0.f, 0.f};
    if (sub == 15) {
        float *q = body + 4 * nb;
        if (tail & 2) *reinterpret_cast<f32x2 *>(q) = f32x2{0.f, 0.f};
        if (tail & 1) q[tail & 2] = 0.f;
    }
}

// grid: y = job, x walks the job's segments (walk_segments, stream_jobs.h) and zeroes each.
__global__ __launch_bounds__(256) void scrub_streams_kernel(const ScrubTable t, const int32_t *__restrict__ streams, int n_streams,
                                                            int n_total) {
    walk_segments(t.job[blockIdx.y], streams, n_streams, n_total,
                  [](int, int, int, uint32_t *p, int seg, int sub) { zero_segment(reinterpret_cast<float *>(p), seg, sub); });
}

extern "C" int csk_co_scrub_streams_f32(const csk_scrub_job *jobs, int n_jobs, const int32_t *streams, int n_streams, int n_total,
                                        void *stream) {
    if (!jobs) CSK_FAIL("co_scrub_streams: null pointer (jobs)");
    if (n_jobs < 1 || n_jobs > CSK_CO_SCRUB_MAX_JOBS) CSK_FAIL("co_scrub_streams: 1..%d jobs per launch, got %d", CSK_CO_SCRUB_MAX_JOBS, n_jobs);
    if (n_streams < 0) CSK_FAIL("co_scrub_streams: n_streams < 0");
    if (n_total < 1) CSK_FAIL("co_scrub_streams: the slab holds n_total >= 1 streams, got %d", n_total);
    if (n_streams > n_total) CSK_FAIL("co_scrub_streams: %d stream indices cannot fit a slab of %d streams", n_streams, n_total);
    if (n_streams > 0 && !streams) CSK_FAIL("co_scrub_streams: null pointer (streams)");
    ScrubTable t;
    int n = 0;
    int64_t most = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const csk_scrub_job &s = jobs[i];
        SlotRun &d = t.job[n];
        const auto run_of_job = [&](SlotRun &run) {     // this entry's own checks: the run as the caller names it
            if (s.slot0 < 0 || s.slot0 >= s.depth) CSK_FAIL("co_scrub_streams: slot0 %d of job %d outside a ring of %d slots", s.slot0, i, s.depth);
            if (s.n_slots < 0 || s.n_slots > s.depth)
                CSK_FAIL("co_scrub_streams: a run of %d slots in job %d is longer than the ring (%d slots)", s.n_slots, i, s.depth);
            run.slot0 = s.slot0, run.n_slots = s.n_slots;
            return 0;
        };
        if (resolve_ring_job("co_scrub_streams", i, s.kind, s.ring, s.row_floats, s.depth, s.rows, s.seg, n_total, d, run_of_job)) return -1;
        if (d.n_slots == 0) continue;                   // an empty run: nothing to launch for it
        if (run_segments(d, n_streams) > most) most = run_segments(d, n_streams);
        ++n;
    }
    if (n == 0 || n_streams == 0) return 0;
    hipLaunchKernelGGL(scrub_streams_kernel, table_grid(t.job, n, most, 16, 4096), dim3(256), 0, (hipStream_t)stream, t, streams, n_streams,
                       n_total);
    return (int)hipGetLastError();
}
