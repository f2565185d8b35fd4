// stream_prime.hip -- write the packed records of some streams (the layout of stream_move.hip) from the
// tensors of a CLIP pass over their history (csk_co_prime_pack_f32, include/cskel.h; co_prime.py).  One
// launch takes a table of jobs; record k of the packed buffer belongs to stream k of every source tensor.
//   ring job   a clip tensor (n * M, C, T_src, V): the frames first .. first + window - 1 of the stream's M skeleton
//              sequences become [frame, oldest first][row c][segment m * V + v] -- the order in which a ring slot holds a
//              stream (position n * M * V + m * V + v of a channel-major row: input_norm_frames_kernel, frame_to_slot) and
//              stream_move.hip packs it.  A frame in front of the clip (index < 0) is +0.0: what the zeroed rings of a fresh
//              model hold there.  Words travel as 32-bit patterns.
//   pool job   the same kind of source, the last block's output: entry i is the spatial mean of frame first + i over the
//              stream's M * V positions, C floats per entry -- the arithmetic and the summation order of co_head_kernel's
//              pool (head.hip): lane-strided partial sums over j = m * V + v, the xor butterfly 32 .. 1, one division by
//              (float)(M * V).  That loop is interleaved sixteen rows deep with the head's ring store, so it is restated
//              here and not shared; tests/test_gpu_stream_prime.py holds the two together bit for bit.
//   words job  a per-stream array [n][words] (flags, latched rotations, the previous raw frame): a plain copy.
// HBM-bound: source runs are V contiguous floats at stride T_src * V, the stores are contiguous.  The jobs read clip tensors,
// not rings, so of stream_jobs.h this file takes the grid of a by-value job table only.
#include "stream_jobs.h"

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct PrimeJob {
    const uint32_t *src;
    int64_t offset;             // of the job's words inside a record
    int64_t len;                // words of the job per stream
    int32_t kind, rows, t_src, first, window, pad_;
};
struct PrimeTable {
    PrimeJob job[CSK_CO_MOVE_MAX_JOBS];
};

// Ring and words jobs: a thread owns one 16-byte aligned group of four record words -- lanes hold consecutive groups, so a
// wave stores 1 KiB in one piece -- and the groups at either end of the job's run, where the run is not aligned, store their
// words one by one.  A record starts at any 4-byte boundary (record_words may be odd), hence `mis`, the run's word offset
// behind the 16-byte boundary in front of it, per stream and job.
__device__ __forceinline__ void pack_run(const PrimeJob &j, uint32_t *__restrict__ run, int64_t k, int64_t q, int M, int V) {
    const int mis = (int)((reinterpret_cast<uintptr_t>(run) >> 2) & 3u);
    const int64_t e0 = 4 * q - mis;                     // first run word of this group; < 0 only in group 0
    if (e0 >= j.len) return;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (j.kind == CSK_PRIME_WORDS) {
        const uint32_t *s = j.src + k * j.len;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e0 + u >= 0 && e0 + u < j.len) w[u] = s[e0 + u];
    } else {
        // run word e = ((i * rows + c) * M + m) * V + v; the four words of a group are walked with carries
        const int64_t lo = e0 < 0 ? 0 : e0;
        int v = (int)(lo % V);
        int64_t r = lo / V;
        int m = (int)(r % M);
        r /= M;
        int c = (int)(r % j.rows), i = (int)(r / j.rows);
        const int64_t chan = (int64_t)j.t_src * V;      // floats of one (sequence, channel) of the source
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (e0 + u < 0 || e0 + u >= j.len) continue;
            const int t = j.first + i;
            if (t >= 0) w[u] = j.src[(((k * M + m) * j.rows + c) * chan) + (int64_t)t * V + v];
            if (++v == V) {
                v = 0;
                if (++m == M) {
                    m = 0;
                    if (++c == j.rows) c = 0, ++i;
                }
            }
        }
    }
    if (e0 >= 0 && e0 + 4 <= j.len) {
        *reinterpret_cast<u32x4 *>(run + e0) = u32x4{w[0], w[1], w[2], w[3]};
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e0 + u >= 0 && e0 + u < j.len) run[e0 + u] = w[u];
    }
}

// grid: y = job, x strides over the job's work items -- (stream, group of four words) for ring and words jobs, one WAVE per
// (stream, entry, channel) for the pool job
__global__ __launch_bounds__(256) void prime_pack_kernel(const PrimeTable t, uint32_t *__restrict__ packed, int64_t record_words,
                                                         int n_streams, int M, int V) {
    const PrimeJob &j = t.job[blockIdx.y];
    if (j.kind == CSK_PRIME_POOL) {
        const int lane = threadIdx.x & 63, MV = M * V;
        const int64_t total = (int64_t)n_streams * j.window * j.rows;
        const int64_t chan = (int64_t)j.t_src * V;
        for (int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6; g < total; g += (int64_t)gridDim.x * 4) {
            const int c = (int)(g % j.rows);
            const int64_t r = g / j.rows;
            const int i = (int)(r % j.window);
            const int64_t k = r / j.window;
            const int tf = j.first + i;
            float a = 0.f;
            if (tf >= 0) {
                const float *src = reinterpret_cast<const float *>(j.src) + (k * M * j.rows + c) * chan + (int64_t)tf * V;
                for (int p = lane; p < MV; p += 64) a += src[(int64_t)(p / V) * j.rows * chan + p % V];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
                a = a / (float)MV;
            }
            if (lane == 0) reinterpret_cast<float *>(packed)[k * record_words + j.offset + (int64_t)i * j.rows + c] = a;
        }
        return;
    }
    const int64_t groups = (j.len + 3) / 4 + 1;         // enough for any misalignment of the run
    const int64_t total = groups * n_streams;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int64_t k = g / groups;
        pack_run(j, packed + k * record_words + j.offset, k, g % groups, M, V);
    }
}

extern "C" int csk_co_prime_pack_f32(const csk_prime_job *jobs, int n_jobs, void *packed, int64_t record_floats, int n_streams, int M,
                                     int V, void *stream) {
    if (!jobs) CSK_FAIL("co_prime_pack: null pointer (jobs)");
    if (n_jobs < 1 || n_jobs > CSK_CO_MOVE_MAX_JOBS) CSK_FAIL("co_prime_pack: 1..%d jobs per launch, got %d", CSK_CO_MOVE_MAX_JOBS, n_jobs);
    if (n_streams < 0) CSK_FAIL("co_prime_pack: n_streams < 0");
    if (M < 1 || V < 1) CSK_FAIL("co_prime_pack: a stream is M >= 1 skeletons of V >= 1 joints, got M = %d, V = %d", M, V);
    if (record_floats < 1) CSK_FAIL("co_prime_pack: a record of %lld floats", (long long)record_floats);
    if (n_streams > 0 && !packed) CSK_FAIL("co_prime_pack: null pointer (packed)");
    if (reinterpret_cast<uintptr_t>(packed) & 3) CSK_FAIL("co_prime_pack: the packed buffer is not 4-byte aligned");
    PrimeTable t;
    int n = 0;
    int64_t most = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const csk_prime_job &s = jobs[i];
        if (s.kind != CSK_PRIME_RING && s.kind != CSK_PRIME_POOL && s.kind != CSK_PRIME_WORDS)
            CSK_FAIL("co_prime_pack: unknown job kind %d in job %d", s.kind, i);
        if (!s.src) CSK_FAIL("co_prime_pack: null pointer (source of job %d)", i);
        if (reinterpret_cast<uintptr_t>(s.src) & 3) CSK_FAIL("co_prime_pack: source of job %d is not 4-byte aligned", i);
        if (s.rows < 1 || s.t_src < 1) CSK_FAIL("co_prime_pack: bad dims in job %d (rows %d, t_src %d)", i, s.rows, s.t_src);
        if (s.window < 0) CSK_FAIL("co_prime_pack: a window of %d frames in job %d", s.window, i);
        if (s.kind == CSK_PRIME_WORDS && (s.first != 0 || s.window > 1 || s.t_src != 1))
            CSK_FAIL("co_prime_pack: a words job copies one array per stream (first 0, window 0 or 1, t_src 1; job %d)", i);
        if ((int64_t)s.first + s.window > s.t_src)
            CSK_FAIL("co_prime_pack: job %d takes frames [%d, %lld) of a source of %d frames", i, s.first, (long long)s.first + s.window, s.t_src);
        const int64_t len = (int64_t)s.window * s.rows * (s.kind == CSK_PRIME_RING ? (int64_t)M * V : 1);
        if (s.offset < 0 || s.offset + len > record_floats)
            CSK_FAIL("co_prime_pack: job %d covers floats [%lld, %lld) of a record of %lld", i, (long long)s.offset, (long long)(s.offset + len),
                     (long long)record_floats);
        if (len == 0) continue;                         // an empty window: nothing to launch for it
        t.job[n] = {reinterpret_cast<const uint32_t *>(s.src), s.offset, len, s.kind, s.rows, s.t_src, s.first, s.window, 0};
        const int64_t blocks = s.kind == CSK_PRIME_POOL ? ((int64_t)n_streams * s.window * s.rows + 3) / 4
                                                        : (((len + 3) / 4 + 1) * n_streams + 255) / 256;
        if (blocks > most) most = blocks;
        ++n;
    }
    if (n == 0 || n_streams == 0) return 0;
    hipLaunchKernelGGL(prime_pack_kernel, table_grid(t.job, n, most, 1, 8192), dim3(256), 0, (hipStream_t)stream, t,
                       reinterpret_cast<uint32_t *>(packed), record_floats, n_streams, M, V);
    return (int)hipGetLastError();
}
