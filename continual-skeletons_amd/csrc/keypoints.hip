// keypoints.hip -- Kinetics keypoint intake on the device (csk_select_people_f32, csk_select_people_frames_f32;
// include/cskel.h).  Counterpart of the reference's offline datasets/data_preparation/kinetics400_prep.py:100-138
// (Feeder_kinetics.__getitem__): per (sample, frame) the P people a pose estimator found, k (P, V, 3) = (x, y, score) per
// joint, are ranked by the sum of their joint scores, the best M are kept, x and y are centred, y is flipped and the
// coordinates of joints with score 0 are zeroed -- written channel-first, as the models take it.
// A one-pass, HBM-bound permute.  An item is one (sample, frame); a workgroup takes batches of B consecutive items of one
// source buffer (a contiguous span of B * P * V * 3 words), stages the span into LDS with coalesced loads (16 bytes per lane
// where the span is 16-byte aligned -- B is a multiple of 4, so it is whenever the buffer is -- dwords otherwise), forms the
// P fp64 score sums of every item (one thread each) and the order of its people (one thread per item), and stores the
// 3 * V * M outputs of every item from LDS, consecutive threads to consecutive addresses of a run.  There is no arithmetic
// across items, so the bits do not depend on B.  Both entries are this one kernel: the frames form is the clip form with
// T = 1 and one pair of pointers per frame.
#include "mfma_core.h"

namespace {

constexpr int KP_THREADS = 256;
constexpr int KP_MAX_P = 8, KP_MAX_V = 64;
constexpr int KP_MAX_B = 32;            // items of a batch, at most: KP_MAX_B * KP_MAX_P sums = one thread each
constexpr int KP_STAGE = 8192;          // words of the staging buffer (32 KiB); the largest item has 8 * 64 * 3 = 1536
constexpr int KP_TARGET_BATCHES = 1024; // B shrinks (down to 4) until a launch has about this many batches

#define CSK_REJECT(...)                                 \
    do {                                                \
        snprintf(csk_err_buf(), 256, __VA_ARGS__);      \
        return -2;                                      \
    } while (0)

struct KpBuffers {
    const float *src[8];
    float *dst[8];
};

// q is placed before p (q != p): the larger sum first, equal sums by index, a NaN sum behind every number
__device__ __forceinline__ bool placed_before(double sq, int q, double sp, int p) {
    const bool nq = sq != sq, np = sp != sp;
    if (nq || np) return nq == np ? q < p : np;
    return sq > sp || (sq == sp && q < p);
}

// src[f] holds `per` items of P * V * 3 words; item j of it is (n, t) = (j / T, j % T) and goes to dst[f] (per / T, 3, T, V, M).
// bpp = batches per buffer = ceil(per / B); batches = buffers * bpp.
__global__ __launch_bounds__(KP_THREADS) void select_people_kernel(const KpBuffers f, int64_t batches, int64_t bpp, int64_t per, int B,
                                                                    int T, int P, int V, int M) {
    __shared__ __attribute__((aligned(16))) float stage[KP_STAGE];
    __shared__ double sums[KP_MAX_B * KP_MAX_P];
    __shared__ unsigned char order[KP_MAX_B * KP_MAX_P];
    const int tid = (int)threadIdx.x;
    const int PV3 = P * V * 3, VM = V * M;
    for (int64_t b = blockIdx.x; b < batches; b += gridDim.x) {             // uniform per workgroup (barriers inside)
        const int fr = (int)(b / bpp);
        const int64_t j0 = (b - fr * bpp) * B;
        const int nb = per - j0 < B ? (int)(per - j0) : B;
        const float *span = f.src[fr] + j0 * PV3;
        const int len = nb * PV3;
        if ((reinterpret_cast<uintptr_t>(span) & 15) == 0) {
            const int len4 = len >> 2;
            for (int q = tid; q < len4; q += KP_THREADS)
                *reinterpret_cast<f32x4 *>(stage + 4 * q) = *reinterpret_cast<const f32x4 *>(span + 4 * q);
            for (int e = 4 * len4 + tid; e < len; e += KP_THREADS) stage[e] = span[e];
        } else {
            for (int e = tid; e < len; e += KP_THREADS) stage[e] = span[e];
        }
        __syncthreads();
        if (tid < nb * P) {                                                 // S[p] = sum of the V scores, fp64, v ascending
            const float *s = stage + tid * V * 3 + 2;
            double acc = 0.0;
            for (int v = 0; v < V; ++v) acc += (double)s[3 * v];
            sums[tid] = acc;
        }
        __syncthreads();
        if (tid < nb) {                                                     // the order of the item's people
            for (int p = 0; p < P; ++p) {
                const double sp = sums[tid * P + p];
                int rank = 0;
                for (int q = 0; q < P; ++q)
                    if (q != p && placed_before(sums[tid * P + q], q, sp, p)) ++rank;
                order[tid * KP_MAX_P + rank] = (unsigned char)p;
            }
        }
        __syncthreads();
        const int work = nb * 3 * VM;
        float *dst = f.dst[fr];
        for (int e = tid; e < work; e += KP_THREADS) {
            // clip form: (c, item, vm) -- a channel's frames of one sample are consecutive; T = 1: (item, c, vm), as dst lies
            int i, c;
            const int vm = e % VM;
            if (T == 1) {
                c = (e / VM) % 3;
                i = e / (3 * VM);
            } else {
                i = (e / VM) % nb;
                c = e / (VM * nb);
            }
            const int v = vm / M, m = vm - v * M;
            const int p = order[i * KP_MAX_P + m];
            const float *j = stage + ((i * P + p) * V + v) * 3;
            const float s = j[2];
            float val = s;
            if (c == 0) val = s == 0.f ? 0.f : j[0] - 0.5f;
            if (c == 1) val = s == 0.f ? 0.f : -(j[1] - 0.5f);                 // subtract, then negate: y == 0.5 gives -0.0
            const int64_t jt = j0 + i, n = jt / T, t = jt - n * T;
            dst[((n * 3 + c) * T + t) * VM + vm] = val;
        }
        __syncthreads();                                                    // before the next batch overwrites the stage
    }
}

int check_people(const char *who, int P, int V, int M) {
    if (P > KP_MAX_P || M > P) CSK_REJECT("%s: 1 <= M <= P <= %d people, got M = %d, P = %d", who, KP_MAX_P, M, P);
    if (V > KP_MAX_V) CSK_REJECT("%s: 1 <= V <= %d joints, got %d", who, KP_MAX_V, V);
    return 0;
}

int launch(const KpBuffers &f, int buffers, int64_t per, int T, int P, int V, int M, hipStream_t stream) {
    const int PV3 = P * V * 3;
    int B = KP_STAGE / PV3 / 4 * 4;                     // a multiple of 4: every batch of a 16-byte aligned buffer is aligned
    B = B > KP_MAX_B ? KP_MAX_B : B;                    // (>= 4: the largest item has 1536 words)
    while (B > 4 && (per + B - 1) / B * buffers < KP_TARGET_BATCHES) B -= 4;
    const int64_t bpp = (per + B - 1) / B, batches = bpp * buffers;
    const dim3 grid((unsigned)(batches < 65536 ? batches : 65536)), block(KP_THREADS);
    hipLaunchKernelGGL(select_people_kernel, grid, block, 0, stream, f, batches, bpp, per, B, T, P, V, M);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int csk_select_people_f32(const float *k, float *out, int N, int T, int P, int V, int M, void *stream) {
    if (!k || !out) CSK_FAIL("select_people: null pointer");
    if (k == out) CSK_FAIL("select_people: out must not be k (the order of a frame's people is read after they are written)");
    if (N <= 0 || T <= 0 || P <= 0 || V <= 0 || M <= 0) CSK_FAIL("select_people: bad dims");
    if (const int rc = check_people("select_people", P, V, M)) return rc;
    KpBuffers f;
    for (int i = 0; i < 8; ++i) {
        f.src[i] = k;
        f.dst[i] = out;
    }
    return launch(f, 1, (int64_t)N * T, T, P, V, M, (hipStream_t)stream);
}

extern "C" int csk_select_people_frames_f32(const float *const *frames, float *const *dst, int r, int N, int P, int V, int M,
                                            void *stream) {
    if (!frames || !dst) CSK_FAIL("select_people_frames: null pointer");
    if (r < 1 || r > 8) CSK_REJECT("select_people_frames: a cycle holds 1..8 frames, got %d", r);
    if (N <= 0 || P <= 0 || V <= 0 || M <= 0) CSK_FAIL("select_people_frames: bad dims");
    if (const int rc = check_people("select_people_frames", P, V, M)) return rc;
    KpBuffers f;
    for (int i = 0; i < 8; ++i) {
        f.src[i] = frames[i < r ? i : r - 1];
        f.dst[i] = dst[i < r ? i : r - 1];
        if (!f.src[i] || !f.dst[i]) CSK_FAIL("select_people_frames: null frame");
    }
    for (int i = 0; i < r; ++i)
        for (int j = 0; j < r; ++j)
            if (f.dst[i] == f.src[j] || (j != i && f.dst[i] == f.dst[j]))
                CSK_FAIL("select_people_frames: every dst must be a buffer of its own, none of them a source frame");
    return launch(f, r, N, 1, P, V, M, (hipStream_t)stream);
}
