// modality.hip -- bone / motion input modalities derived from the joint tensor on the device (csk_derive_modality_f32,
// csk_derive_modality_frames_f32; include/cskel.h).  Counterpart of the reference's offline numpy scripts
// datasets/data_preparation/bone_data_prep.py:158-163 (b[v] = x[v] - x[parent(v)], read from the original x) and
// motion_data_prep.py:28-30 (m[t] = x[t+1] - x[t], m[T-1] = 0).  Every subtraction is one fp32 rounding, in the order the
// header states; nothing is reassociated (no fast-math), so the result equals numpy's bit for bit.
// HBM-bound: one pass, each thread owns 4 consecutive floats -- a 16-byte load of x and a 16-byte store of the result
// when the tensors are 16-byte aligned, scalar accesses otherwise and for the last total % 4 floats.  The second operands
// (the parent joint of the same frame row, the neighbouring frame) are 4-byte loads of lines the pass has in cache anyway.
#include "mfma_core.h"

namespace {

constexpr int MOD_MAX_V = 64;       // joints the by-value parent table holds
constexpr int MOD_MAX_VM = 512;     // floats of one frame row (V * M) the LDS offset table holds

#define CSK_REJECT(...)                                 \
    do {                                                \
        snprintf(csk_err_buf(), 256, __VA_ARGS__);      \
        return -2;                                      \
    } while (0)

struct ParentTable {
    int32_t p[MOD_MAX_V];
};

// doff[j], j = v * M + m: distance in floats from an element of a frame row (V, M) back to its parent joint's element
// (v - parent(v)) * M -- so the parent of x[i] is x[i - doff[j]], inside the same row because parent(v) is in [0, V)
__device__ __forceinline__ void fill_parent_offsets(int *doff, const ParentTable &par, int V, int M) {
    for (int j = threadIdx.x; j < V * M; j += blockDim.x) {
        const int v = j / M;
        doff[j] = (v - par.p[v]) * M;
    }
    __syncthreads();
}

__device__ __forceinline__ void load4(const float *p, bool vec, int n, float (&a)[4]) {
    if (vec && n == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4 *>(p);
        a[0] = q[0]; a[1] = q[1]; a[2] = q[2]; a[3] = q[3];
    } else {
        for (int e = 0; e < 4; ++e) a[e] = e < n ? p[e] : 0.f;
    }
}

__device__ __forceinline__ void store4(float *p, bool vec, int n, const float (&a)[4]) {
    if (vec && n == 4) {
        *reinterpret_cast<f32x4 *>(p) = f32x4{a[0], a[1], a[2], a[3]};
    } else {
        for (int e = 0; e < 4; ++e)
            if (e < n) p[e] = a[e];
    }
}

// clip form: x, out (N, C, T, V, M) flat; element i lies in frame row i / VM (rows = N * C * T, frame t = row % T) at row
// position j = i % VM.  The next frame of the same (n, c) plane is VM floats further on.
template <int MODE>
__global__ __launch_bounds__(256) void derive_clip_kernel(const float *__restrict__ x, float *__restrict__ out, const ParentTable par,
                                                          int T, int V, int M, int64_t total, int vec) {
    __shared__ int doff[MOD_MAX_VM];
    fill_parent_offsets(doff, par, V, M);
    const int VM = V * M;
    const int64_t groups = (total + 3) >> 2;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const int64_t i0 = g << 2;
        const int n = (int)(total - i0 < 4 ? total - i0 : 4);
        const int64_t row = i0 / VM;
        int j = (int)(i0 - row * VM), t = (int)(row % T);
        float a[4], r[4];
        load4(x + i0, vec, n, a);
        for (int e = 0; e < 4; ++e) {
            while (j >= VM) {                           // the group runs on into the next frame row
                j -= VM;
                if (++t == T) t = 0;
            }
            r[e] = 0.f;
            if (e < n) {
                const float *xi = x + i0 + e;
                const int d = doff[j];
                if (MODE == CSK_MODALITY_BONE) {
                    r[e] = a[e] - xi[-d];
                } else if (t < T - 1) {                 // the last frame of a clip has no successor: 0
                    if (MODE == CSK_MODALITY_JOINT_MOTION) {
                        r[e] = xi[VM] - a[e];
                    } else {
                        const float b1 = xi[VM] - xi[VM - d];
                        const float b0 = a[e] - xi[-d];
                        r[e] = b1 - b0;
                    }
                }
            }
            ++j;
        }
        store4(out + i0, vec, n, r);
    }
}

struct ModFrames {
    const float *src[8];
    float *dst[8];
};

// step form: every frame (N, C, V, M) flat; a stream owns CVM = C * V * M consecutive floats.  A workgroup takes chunks of
// S whole streams (S a multiple of 4: a chunk starts on a 16-byte boundary of an aligned frame) and is the only one that
// reads or writes the previous-frame buffer and the flags of those streams: it derives all r frames of the cycle (frame 0
// against `prev`, where the stream's flag is set; frame f >= 1 against frame f - 1), and only then -- behind a barrier --
// stores the cycle's last raw frame into `prev` and sets the flags.  The parent of an element is in its own stream.
template <int MODE>
__global__ __launch_bounds__(256) void derive_frames_kernel(const ModFrames f, int r, const ParentTable par, float *__restrict__ prev,
                                                            int32_t *__restrict__ has_prev, int update, int N, int CVM, int V, int M,
                                                            int S, int vec) {
    __shared__ int doff[MOD_MAX_VM];
    fill_parent_offsets(doff, par, V, M);
    const int VM = V * M;
    const int chunks = (N + S - 1) / S;
    for (int chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {          // uniform per workgroup (barrier inside)
        const int n0 = chunk * S;
        const int ns = N - n0 < S ? N - n0 : S;
        const int span = ns * CVM, groups = (span + 3) >> 2;
        const int base = n0 * CVM;
        for (int q = threadIdx.x; q < groups; q += 256) {
            const int n = span - 4 * q < 4 ? span - 4 * q : 4;
            const int i0 = base + 4 * q;
            const int j0 = i0 % VM;
            bool have[4];
            for (int e = 0; e < 4; ++e)
                have[e] = MODE != CSK_MODALITY_BONE && e < n && has_prev[n0 + (4 * q + e) / CVM] != 0;
            float a[4], pa[4], res[4];
            if (MODE != CSK_MODALITY_BONE) load4(prev + i0, vec, n, pa);
            const float *before = prev;
            for (int fr = 0; fr < r; ++fr) {
                const float *cur = f.src[fr];
                load4(cur + i0, vec, n, a);
                int j = j0;
                for (int e = 0; e < 4; ++e) {
                    while (j >= VM) j -= VM;
                    res[e] = 0.f;
                    if (e < n) {
                        const int d = doff[j];
                        if (MODE == CSK_MODALITY_BONE) {
                            res[e] = a[e] - cur[i0 + e - d];
                        } else if (fr > 0 || have[e]) {     // a stream's first frame has no predecessor: 0
                            if (MODE == CSK_MODALITY_JOINT_MOTION) {
                                res[e] = a[e] - pa[e];
                            } else {
                                const float b1 = a[e] - cur[i0 + e - d];
                                const float b0 = pa[e] - before[i0 + e - d];
                                res[e] = b1 - b0;
                            }
                        }
                    }
                    ++j;
                }
                store4(f.dst[fr] + i0, vec, n, res);
                for (int e = 0; e < 4; ++e) pa[e] = a[e];
                before = cur;
            }
        }
        if (MODE != CSK_MODALITY_BONE && update) {
            __syncthreads();                            // every read of prev / has_prev of this chunk has returned
            const float *last = f.src[r - 1];
            for (int q = threadIdx.x; q < groups; q += 256) {
                const int n = span - 4 * q < 4 ? span - 4 * q : 4;
                float a[4];
                load4(last + base + 4 * q, vec, n, a);
                store4(prev + base + 4 * q, vec, n, a);
            }
            if ((int)threadIdx.x < ns) has_prev[n0 + threadIdx.x] = 1;
        }
    }
}

// mode and parent table, checked on the host before anything is launched; fills the by-value table
int check_mode_and_parents(const char *who, int mode, const int32_t *parents, int V, ParentTable *t) {
    if (mode != CSK_MODALITY_BONE && mode != CSK_MODALITY_JOINT_MOTION && mode != CSK_MODALITY_BONE_MOTION)
        CSK_REJECT("%s: unknown mode %d (CSK_MODALITY_BONE / _JOINT_MOTION / _BONE_MOTION; joint input needs no derivation)", who, mode);
    for (int v = 0; v < MOD_MAX_V; ++v) t->p[v] = v;
    if (mode == CSK_MODALITY_JOINT_MOTION) return 0;
    if (!parents) CSK_FAIL("%s: the bone modes need a parent table", who);
    for (int v = 0; v < V; ++v) {
        if (parents[v] < 0 || parents[v] >= V) CSK_REJECT("%s: parent %d of joint %d outside [0, %d)", who, (int)parents[v], v, V);
        t->p[v] = parents[v];
    }
    return 0;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int csk_derive_modality_f32(const float *x, float *out, int mode, const int32_t *parents, int N, int C, int T, int V, int M,
                                       void *stream) {
    if (!x || !out) CSK_FAIL("derive_modality: null pointer");
    if (x == out) CSK_FAIL("derive_modality: out must not be x (the neighbours of an element are read after it is written)");
    if (N <= 0 || C <= 0 || T <= 0 || V <= 0 || M <= 0) CSK_FAIL("derive_modality: bad dims");
    if (V > MOD_MAX_V || V * M > MOD_MAX_VM) CSK_FAIL("derive_modality: built for V <= %d and V * M <= %d", MOD_MAX_V, MOD_MAX_VM);
    ParentTable t;
    if (const int rc = check_mode_and_parents("derive_modality", mode, parents, V, &t)) return rc;
    const int64_t total = (int64_t)N * C * T * V * M;
    const int vec = aligned16(x) && aligned16(out);
    const int64_t want = ((total + 3) / 4 + 255) / 256;
    const dim3 grid((unsigned)(want < 4096 ? want : 4096)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (mode == CSK_MODALITY_BONE)
        hipLaunchKernelGGL(derive_clip_kernel<CSK_MODALITY_BONE>, grid, block, 0, s, x, out, t, T, V, M, total, vec);
    else if (mode == CSK_MODALITY_JOINT_MOTION)
        hipLaunchKernelGGL(derive_clip_kernel<CSK_MODALITY_JOINT_MOTION>, grid, block, 0, s, x, out, t, T, V, M, total, vec);
    else
        hipLaunchKernelGGL(derive_clip_kernel<CSK_MODALITY_BONE_MOTION>, grid, block, 0, s, x, out, t, T, V, M, total, vec);
    return (int)hipGetLastError();
}

extern "C" int csk_derive_modality_frames_f32(const float *const *frames, float *const *dst, int r, int mode, const int32_t *parents,
                                              float *prev, int32_t *has_prev, int update, int N, int C, int V, int M, void *stream) {
    if (!frames || !dst) CSK_FAIL("derive_modality_frames: null pointer");
    if (r < 1 || r > 8) CSK_REJECT("derive_modality_frames: a cycle holds 1..8 frames, got %d", r);
    if (N <= 0 || C <= 0 || V <= 0 || M <= 0) CSK_FAIL("derive_modality_frames: bad dims");
    if (V > MOD_MAX_V || V * M > MOD_MAX_VM) CSK_FAIL("derive_modality_frames: built for V <= %d and V * M <= %d", MOD_MAX_V, MOD_MAX_VM);
    if ((int64_t)N * C * V * M >= (1ll << 31)) CSK_FAIL("derive_modality_frames: frame too large for 32-bit element indices");
    ParentTable t;
    if (const int rc = check_mode_and_parents("derive_modality_frames", mode, parents, V, &t)) return rc;
    const bool motion = mode != CSK_MODALITY_BONE;
    if (motion && (!prev || !has_prev)) CSK_FAIL("derive_modality_frames: the motion modes need the previous-frame buffer and the flags");
    ModFrames f;
    int vec = !motion || aligned16(prev);
    for (int i = 0; i < 8; ++i) {
        f.src[i] = frames[i < r ? i : r - 1];
        f.dst[i] = dst[i < r ? i : r - 1];
        if (!f.src[i] || !f.dst[i]) CSK_FAIL("derive_modality_frames: null frame");
        vec = vec && aligned16(f.src[i]) && aligned16(f.dst[i]);
    }
    for (int i = 0; i < r; ++i) {
        if (motion && (f.src[i] == prev || f.dst[i] == prev)) CSK_FAIL("derive_modality_frames: prev must not be a frame of the cycle");
        for (int k = 0; k < r; ++k)
            if (f.dst[i] == f.src[k] || (k != i && f.dst[i] == f.dst[k]))
                CSK_FAIL("derive_modality_frames: every dst must be a buffer of its own, none of them a source frame");
    }
    const int CVM = C * V * M;
    int S = 1024 / CVM / 4 * 4;                         // streams per chunk: about 1024 floats, a multiple of 4, at most 256
    S = S < 4 ? 4 : (S > 256 ? 256 : S);
    const int chunks = (N + S - 1) / S;
    const dim3 grid((unsigned)(chunks < 2048 ? chunks : 2048)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (mode == CSK_MODALITY_BONE)
        hipLaunchKernelGGL(derive_frames_kernel<CSK_MODALITY_BONE>, grid, block, 0, s, f, r, t, prev, has_prev, update, N, CVM, V, M, S, vec);
    else if (mode == CSK_MODALITY_JOINT_MOTION)
        hipLaunchKernelGGL(derive_frames_kernel<CSK_MODALITY_JOINT_MOTION>, grid, block, 0, s, f, r, t, prev, has_prev, update, N, CVM, V, M, S, vec);
    else
        hipLaunchKernelGGL(derive_frames_kernel<CSK_MODALITY_BONE_MOTION>, grid, block, 0, s, f, r, t, prev, has_prev, update, N, CVM, V, M, S, vec);
    return (int)hipGetLastError();
}
