// stream_move.hip -- copy the live state of SOME streams between the continual slab and a packed buffer
// (csk_co_move_streams_f32, include/cskel.h): the copying counterpart of stream_reset.hip.  One launch takes a table of jobs
// (ring, the slot of its newest live frame, how many newest slots to move, offset inside a stream's packed record) and a
// device list of stream indices; record j of the packed buffer pairs with stream streams[j].  Export reads the rings and
// writes the records, import reads the records and writes -- in every row of the window's slots -- the segments of the named
// streams and nothing else: not the neighbouring streams, not the P-padding, not the slots outside the window.  The words
// are moved as 32-bit patterns (the flags are int32, the latched rotations fp64 halves).  HBM-bound loads and stores only.
#include "mfma_core.h"

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// device form of a job: as ScrubJob (stream_reset.hip), "segment of stream n in row (slot, row) starts at
// (slot * rows + row) * row_stride + n * seg"; in the record the window's slots go oldest first: (i * rows + row) * seg
struct MoveJob {
    uint32_t *ring;
    int64_t row_stride, offset;
    int32_t depth, rows, slot0, n_slots, seg, pad_;
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

// grid: y = job, x strides over the job's segments (slot of the window, row, listed stream -- streams fastest, as the scrub
// kernel).  An index outside [0, n_total) moves nothing.
__global__ __launch_bounds__(256) void move_streams_kernel(const MoveTable t, uint32_t *__restrict__ packed, int64_t record_words,
                                                           const int32_t *__restrict__ streams, int n_streams, int n_total,
                                                           int to_ring) {
    const MoveJob &j = t.job[blockIdx.y];
    const int sub = threadIdx.x & 15;
    const int64_t total = (int64_t)j.n_slots * j.rows * n_streams;
    for (int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4; g < total; g += (int64_t)gridDim.x * 16) {
        const int k = (int)(g % n_streams);
        const int64_t q = g / n_streams;
        const int row = (int)(q % j.rows), i = (int)(q / j.rows);
        int slot = j.slot0 + i;
        if (slot >= j.depth) slot -= j.depth;
        const int n = streams[k];
        if (n < 0 || n >= n_total) continue;
        uint32_t *in_ring = j.ring + ((int64_t)slot * j.rows + row) * j.row_stride + (int64_t)n * j.seg;
        uint32_t *in_record = packed + (int64_t)k * record_words + j.offset + ((int64_t)i * j.rows + row) * j.seg;
        if (to_ring)
            copy_segment(in_ring, in_record, j.seg, sub);
        else
            copy_segment(in_record, in_ring, j.seg, sub);
    }
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
        if (!s.ring) CSK_FAIL("co_move_streams: null pointer (ring of job %d)", i);
        if (reinterpret_cast<uintptr_t>(s.ring) & 3) CSK_FAIL("co_move_streams: ring of job %d is not 4-byte aligned", i);
        if (s.depth < 1 || s.rows < 1 || s.seg < 1 || s.row_floats < 1) CSK_FAIL("co_move_streams: bad dims in job %d", i);
        if (s.newest < 0 || s.newest >= s.depth) CSK_FAIL("co_move_streams: newest slot %d of job %d outside a ring of %d slots", s.newest, i, s.depth);
        if (s.window < 0 || s.window > s.depth)
            CSK_FAIL("co_move_streams: a window of %d slots in job %d is longer than the ring (%d slots)", s.window, i, s.depth);
        MoveJob &d = t.job[n];
        int slot0 = s.newest + 1 - s.window;            // the window's oldest slot; > -depth
        if (slot0 < 0) slot0 += s.depth;
        if (s.kind == CSK_SCRUB_BLOCK_RING) {
            if ((int64_t)n_total * s.seg > s.row_floats)
                CSK_FAIL("co_move_streams: %d streams of %d floats cannot fit a row of %lld floats (job %d)", n_total, s.seg,
                         (long long)s.row_floats, i);
            d = {reinterpret_cast<uint32_t *>(s.ring), s.row_floats, s.offset, s.depth, s.rows, slot0, s.window, s.seg, 0};
        } else if (s.kind == CSK_SCRUB_POOL_RING) {
            if (s.rows != n_total || s.seg != s.row_floats)
                CSK_FAIL("co_move_streams: a pooling ring has one row of seg = row_floats floats per stream (job %d: rows %d, slab %d)", i,
                         s.rows, n_total);
            d = {reinterpret_cast<uint32_t *>(s.ring), (int64_t)s.rows * s.row_floats, s.offset, s.depth, 1, slot0, s.window, s.seg, 0};
        } else {
            CSK_FAIL("co_move_streams: unknown ring kind %d in job %d", s.kind, i);
        }
        if (s.offset < 0 || s.offset + (int64_t)d.n_slots * d.rows * d.seg > record_floats)
            CSK_FAIL("co_move_streams: job %d covers floats [%lld, %lld) of a record of %lld", i, (long long)s.offset,
                     (long long)(s.offset + (int64_t)d.n_slots * d.rows * d.seg), (long long)record_floats);
        if (d.n_slots == 0) continue;                   // an empty window: nothing to launch for it
        const int64_t segs = (int64_t)d.n_slots * d.rows * n_streams;
        if (segs > most) most = segs;
        ++n;
    }
    if (n == 0 || n_streams == 0) return 0;
    for (int i = n; i < CSK_CO_MOVE_MAX_JOBS; ++i) t.job[i] = t.job[0];    // never indexed (grid y = n); keeps the table defined
    const int64_t want = (most + 15) / 16;
    const unsigned blocks = (unsigned)(want < 4096 ? want : 4096);
    hipLaunchKernelGGL(move_streams_kernel, dim3(blocks, (unsigned)n), dim3(256), 0, (hipStream_t)stream, t, reinterpret_cast<uint32_t *>(packed),
                       record_floats, streams, n_streams, n_total, to_ring);
    return (int)hipGetLastError();
}
