// stream_reset.hip -- zero the state of SOME streams of the continual slab (csk_co_scrub_streams_f32, include/cskel.h).
// One launch takes a table of jobs (ring, run of slots) and a device list of stream indices and zeroes, in every row of
// every slot of each run, the segments of those streams -- nothing else: not the neighbouring streams, not the P-padding
// behind the last one.  Two uses (co_reset.py): the full reset of a stream (all slots of every ring) and the per-cycle
// scrub of what the not-yet-live blocks wrote for a warming stream (the slots one cycle wrote).  HBM-bound stores only.
#include "mfma_core.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

// device form of a job: both layouts of include/cskel.h reduce to "segment of stream n in row (slot, row) starts at
// (slot * rows + row) * row_stride + n * seg" (pooling ring [slots][N][C]: one row of N * C floats per slot, seg = C)
struct ScrubJob {
    float *ring;
    int64_t row_stride;
    int32_t depth, rows, slot0, n_slots, seg, pad_;
};
struct ScrubTable {
    ScrubJob job[CSK_CO_SCRUB_MAX_JOBS];
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

// grid: y = job, x strides over the job's segments (slot of the run, row, listed stream -- streams fastest, so neighbouring
// 16-lane groups write neighbouring parts of one row).  An index outside [0, n_total) writes nothing.
__global__ __launch_bounds__(256) void scrub_streams_kernel(const ScrubTable t, const int32_t *__restrict__ streams, int n_streams,
                                                            int n_total) {
    const ScrubJob &j = t.job[blockIdx.y];
    const int sub = threadIdx.x & 15;
    const int64_t total = (int64_t)j.n_slots * j.rows * n_streams;
    for (int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4; g < total; g += (int64_t)gridDim.x * 16) {
        const int k = (int)(g % n_streams);
        const int64_t q = g / n_streams;
        const int row = (int)(q % j.rows);
        int slot = j.slot0 + (int)(q / j.rows);
        if (slot >= j.depth) slot -= j.depth;
        const int n = streams[k];
        if (n < 0 || n >= n_total) continue;
        zero_segment(j.ring + ((int64_t)slot * j.rows + row) * j.row_stride + (int64_t)n * j.seg, j.seg, sub);
    }
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
        if (!s.ring) CSK_FAIL("co_scrub_streams: null pointer (ring of job %d)", i);
        if (reinterpret_cast<uintptr_t>(s.ring) & 3) CSK_FAIL("co_scrub_streams: ring of job %d is not 4-byte aligned", i);
        if (s.depth < 1 || s.rows < 1 || s.seg < 1 || s.row_floats < 1) CSK_FAIL("co_scrub_streams: bad dims in job %d", i);
        if (s.slot0 < 0 || s.slot0 >= s.depth) CSK_FAIL("co_scrub_streams: slot0 %d of job %d outside a ring of %d slots", s.slot0, i, s.depth);
        if (s.n_slots < 0 || s.n_slots > s.depth)
            CSK_FAIL("co_scrub_streams: a run of %d slots in job %d is longer than the ring (%d slots)", s.n_slots, i, s.depth);
        ScrubJob &d = t.job[n];
        if (s.kind == CSK_SCRUB_BLOCK_RING) {
            if ((int64_t)n_total * s.seg > s.row_floats)
                CSK_FAIL("co_scrub_streams: %d streams of %d floats cannot fit a row of %lld floats (job %d)", n_total, s.seg,
                         (long long)s.row_floats, i);
            d = {s.ring, s.row_floats, s.depth, s.rows, s.slot0, s.n_slots, s.seg, 0};
        } else if (s.kind == CSK_SCRUB_POOL_RING) {
            if (s.rows != n_total || s.seg != s.row_floats)
                CSK_FAIL("co_scrub_streams: a pooling ring has one row of seg = row_floats floats per stream (job %d: rows %d, slab %d)", i,
                         s.rows, n_total);
            d = {s.ring, (int64_t)s.rows * s.row_floats, s.depth, 1, s.slot0, s.n_slots, s.seg, 0};
        } else {
            CSK_FAIL("co_scrub_streams: unknown ring kind %d in job %d", s.kind, i);
        }
        if (d.n_slots == 0) continue;                   // an empty run: nothing to launch for it
        const int64_t segs = (int64_t)d.n_slots * d.rows * n_streams;
        if (segs > most) most = segs;
        ++n;
    }
    if (n == 0 || n_streams == 0) return 0;
    for (int i = n; i < CSK_CO_SCRUB_MAX_JOBS; ++i) t.job[i] = t.job[0];   // never indexed (grid y = n); keeps the table defined
    const int64_t want = (most + 15) / 16;
    const unsigned blocks = (unsigned)(want < 4096 ? want : 4096);
    hipLaunchKernelGGL(scrub_streams_kernel, dim3(blocks, (unsigned)n), dim3(256), 0, (hipStream_t)stream, t, streams, n_streams, n_total);
    return (int)hipGetLastError();
}
