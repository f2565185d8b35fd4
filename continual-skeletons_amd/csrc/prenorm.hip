// prenorm.hip -- pre-normalisation of raw skeleton frames on the device (csk_prenorm_f32, csk_prenorm_frames_f32;
// include/cskel.h).  Counterpart of the reference's offline datasets/data_preparation/preprocess.py:41-90: every frame is
// centred on the main body's joint 1, then rotated by two matrices taken from the FIRST frame of the sample / stream
// (rotation.py:10-50): Rz turns the zaxis bone onto z, Rx the xaxis line of the z-rotated frame onto x.  The bones are fp32
// differences; everything from there to the 18 matrix entries is fp64; a stage is a three-term fp64 dot rounded to fp32
// once.  The padding of null frames (preprocess.py:18-39) looks ahead and is not reproduced, in either form.
// HBM-bound: a workgroup is one wavefront and owns whole samples (times a frame range) or whole streams.  One lane per owned
// sample / stream does the fp64 work from the five joints of frame 0 it needs and leaves the matrices in LDS; behind a
// barrier every lane takes 4 consecutive positions of the contiguous (v, m) axis: its three channels with 16-byte (or
// 8-byte) accesses where the address allows, scalar ones otherwise and for the last positions of a segment.  No access is
// predicated past an operand: a group is cut to the positions the segment has.
#include "mfma_core.h"

namespace {

constexpr int PN_THREADS = 64;
constexpr int PN_POSITIONS = 256;   // positions of one clip work item / floats of the streams of one step chunk, about
constexpr int PN_MAX_S = 32;        // streams of one step chunk, at most (one lane each does the fp64 work)

typedef float f32x2 __attribute__((ext_vector_type(2)));

#define CSK_REJECT(...)                                 \
    do {                                                \
        snprintf(csk_err_buf(), 256, __VA_ARGS__);      \
        return -2;                                      \
    } while (0)

struct Joints {
    int z0, z1, x0, x1;
};

__device__ __forceinline__ bool is_null(float a, float b, float c) { return (a + b) + c == 0.f; }

// fp32(m . fp64(s)): m row-major 3x3
__device__ __forceinline__ void rotate3(const double *m, float a, float b, float c, float &oa, float &ob, float &oc) {
    const double x = a, y = b, z = c;
    oa = (float)fma(m[2], z, fma(m[1], y, m[0] * x));
    ob = (float)fma(m[5], z, fma(m[4], y, m[3] * x));
    oc = (float)fma(m[8], z, fma(m[7], y, m[6] * x));
}

// rotation.py:10-50 in fp64: the matrix that turns the bone d onto the unit axis e_k (k = 2: z, k = 0: x), identity for a
// vanishing bone, a vanishing rotation axis or a vanishing angle.  axis = d x e_k.
__device__ __forceinline__ void align_to_axis(double dx, double dy, double dz, int k, double *m) {
#pragma clang fp contract(off)
    const double ax = k == 2 ? dy : 0.0, ay = k == 2 ? -dx : dz, az = k == 2 ? 0.0 : -dy;
    double angle = 0.0;
    if (fabs(dx) + fabs(dy) + fabs(dz) >= 1e-6) {
        double c = (k == 2 ? dz : dx) / sqrt(dx * dx + dy * dy + dz * dz);
        c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
        angle = acos(c);
    }
    m[0] = m[4] = m[8] = 1.0;
    m[1] = m[2] = m[3] = m[5] = m[6] = m[7] = 0.0;
    if (fabs(ax) + fabs(ay) + fabs(az) < 1e-6 || fabs(angle) < 1e-6) return;
    const double inv = sqrt(ax * ax + ay * ay + az * az);
    double s, a;
    sincos(angle / 2.0, &s, &a);
    const double b = -(ax / inv) * s, c = -(ay / inv) * s, d = -(az / inv) * s;
    const double aa = a * a, bb = b * b, cc = c * c, dd = d * d;
    const double bc = b * c, ad = a * d, ac = a * c, ab = a * b, bd = b * d, cd = c * d;
    m[0] = aa + bb - cc - dd; m[1] = 2 * (bc + ad);     m[2] = 2 * (bd - ac);
    m[3] = 2 * (bc - ad);     m[4] = aa + cc - bb - dd; m[5] = 2 * (cd + ab);
    m[6] = 2 * (bd + ac);     m[7] = 2 * (cd - ab);     m[8] = aa + dd - bb - cc;
}

// The two matrices a sample / stream latches from its first frame; r0, r1, r2: that frame's channel rows (V, M).  Both
// entries come through here, so that the clip form and the step form agree bit for bit.  m[0..9) = Rz, m[9..18) = Rx.
__device__ __forceinline__ void latch_rotations(const float *r0, const float *r1, const float *r2, int M, const Joints jt, double *m) {
    const float c0 = r0[M], c1 = r1[M], c2 = r2[M];                 // centre: joint 1 of the main body
    float s[4][3];
    bool null[4];
    const int joint[4] = {jt.z0, jt.z1, jt.x0, jt.x1};
    for (int i = 0; i < 4; ++i) {
        const float a = r0[joint[i] * M], b = r1[joint[i] * M], c = r2[joint[i] * M];
        null[i] = is_null(a, b, c);
        s[i][0] = null[i] ? 0.f : a - c0;
        s[i][1] = null[i] ? 0.f : b - c1;
        s[i][2] = null[i] ? 0.f : c - c2;
    }
    align_to_axis((double)(s[1][0] - s[0][0]), (double)(s[1][1] - s[0][1]), (double)(s[1][2] - s[0][2]), 2, m);
    float t[2][3];
    for (int i = 0; i < 2; ++i) {
        rotate3(m, s[2 + i][0], s[2 + i][1], s[2 + i][2], t[i][0], t[i][1], t[i][2]);
        if (null[2 + i]) t[i][0] = t[i][1] = t[i][2] = 0.f;
    }
    align_to_axis((double)(t[0][0] - t[1][0]), (double)(t[0][1] - t[1][1]), (double)(t[0][2] - t[1][2]), 0, m + 9);
}

__device__ __forceinline__ void load4(const float *p, int n, float (&a)[4]) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    if (n == 4 && (addr & 15) == 0) {
        const f32x4 q = *reinterpret_cast<const f32x4 *>(p);
        a[0] = q[0]; a[1] = q[1]; a[2] = q[2]; a[3] = q[3];
    } else if (n == 4 && (addr & 7) == 0) {
        const f32x2 q = *reinterpret_cast<const f32x2 *>(p), w = *reinterpret_cast<const f32x2 *>(p + 2);
        a[0] = q[0]; a[1] = q[1]; a[2] = w[0]; a[3] = w[1];
    } else {
        for (int e = 0; e < 4; ++e) a[e] = e < n ? p[e] : 0.f;
    }
}

__device__ __forceinline__ void store4(float *p, int n, const float (&a)[4]) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    if (n == 4 && (addr & 15) == 0) {
        *reinterpret_cast<f32x4 *>(p) = f32x4{a[0], a[1], a[2], a[3]};
    } else if (n == 4 && (addr & 7) == 0) {
        *reinterpret_cast<f32x2 *>(p) = f32x2{a[0], a[1]};
        *reinterpret_cast<f32x2 *>(p + 2) = f32x2{a[2], a[3]};
    } else {
        for (int e = 0; e < 4; ++e)
            if (e < n) p[e] = a[e];
    }
}

// n (1..4) consecutive positions from p0 on of three channel rows that run on over whole frames of VM floats each (row
// position p lies in frame p / VM); the centre of a frame is its element M.  s -> d, the same positions.
__device__ __forceinline__ void normalise4(const float *s0, const float *s1, const float *s2, float *d0, float *d1, float *d2, int p0,
                                           int n, int VM, int M, const double *m) {
    float a[4], b[4], c[4], oa[4], ob[4], oc[4];
    load4(s0 + p0, n, a);
    load4(s1 + p0, n, b);
    load4(s2 + p0, n, c);
    int fr = p0 / VM, left = (fr + 1) * VM - p0;                    // positions left in the frame of element e
    float c0 = s0[fr * VM + M], c1 = s1[fr * VM + M], c2 = s2[fr * VM + M];
    for (int e = 0; e < 4; ++e) {
        oa[e] = ob[e] = oc[e] = 0.f;
        if (e < n) {
            if (left == 0) {                                        // the group runs on into the next frame: its centre
                ++fr;
                left = VM;
                c0 = s0[fr * VM + M]; c1 = s1[fr * VM + M]; c2 = s2[fr * VM + M];
            }
            --left;
            if (!is_null(a[e], b[e], c[e])) {
                float ta, tb, tc;
                rotate3(m, a[e] - c0, b[e] - c1, c[e] - c2, ta, tb, tc);
                rotate3(m + 9, ta, tb, tc, oa[e], ob[e], oc[e]);
            }
        }
    }
    store4(d0 + p0, n, oa);
    store4(d1 + p0, n, ob);
    store4(d2 + p0, n, oc);
}

// clip form: x, out (N, 3, T, V, M).  A work item is one sample and FT frames [t0, t1) of it: the (n, c) plane is contiguous
// over frames, so the item's segment of a channel is (t1 - t0) * VM consecutive floats.  Lane 0 latches the sample's matrices
// from its frame 0 (every item of a sample computes the same 18 doubles).
__global__ __launch_bounds__(PN_THREADS) void prenorm_clip_kernel(const float *__restrict__ x, float *__restrict__ out, int64_t items,
                                                                  int per_sample, int FT, int T, int VM, int M, const Joints jt) {
    __shared__ double rot[18];
    const int64_t plane = (int64_t)T * VM;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {      // uniform per workgroup (barriers inside)
        const int64_t n = item / per_sample;
        const int t0 = (int)(item - n * per_sample) * FT;
        const int t1 = t0 + FT < T ? t0 + FT : T;
        const float *s0 = x + 3 * n * plane, *s1 = s0 + plane, *s2 = s1 + plane;
        float *d0 = out + 3 * n * plane, *d1 = d0 + plane, *d2 = d1 + plane;
        if (threadIdx.x == 0) latch_rotations(s0, s1, s2, M, jt, rot);
        __syncthreads();
        const int lo = t0 * VM, len = (t1 - t0) * VM;
        for (int q = threadIdx.x; 4 * q < len; q += PN_THREADS) {
            const int n4 = len - 4 * q < 4 ? len - 4 * q : 4;
            normalise4(s0 + lo, s1 + lo, s2 + lo, d0 + lo, d1 + lo, d2 + lo, 4 * q, n4, VM, M, rot);
        }
        __syncthreads();                                                    // before the next item overwrites rot
    }
}

struct PnFrames {
    const float *src[8];
    float *dst[8];
};

// step form: every frame (N, 3, V, M).  A workgroup takes chunks of S whole streams and is the only one that reads or writes
// their rows of rot_state (N, 18) and has_rot (N,): lane i < ns owns stream n0 + i, reads its matrices (flag set) or latches
// them from frame 0 of this cycle (flag clear) into LDS, and -- with update, behind the barrier that ends the chunk's reads
// -- stores what it latched and sets the flag.
__global__ __launch_bounds__(PN_THREADS) void prenorm_frames_kernel(const PnFrames f, int r, double *__restrict__ rot_state,
                                                                    int32_t *__restrict__ has_rot, int update, int N, int S, int VM, int M,
                                                                    const Joints jt) {
    __shared__ double rot[PN_MAX_S][18];
    const int chunks = (N + S - 1) / S;
    const int G = (VM + 3) >> 2;                                            // groups of 4 positions in a channel row
    for (int chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {      // uniform per workgroup (barriers inside)
        const int n0 = chunk * S;
        const int ns = N - n0 < S ? N - n0 : S;
        const int own = (int)threadIdx.x;
        bool latched = false;
        if (own < ns) {
            const int n = n0 + own;
            if (has_rot[n] != 0) {
                for (int i = 0; i < 18; ++i) rot[own][i] = rot_state[(int64_t)n * 18 + i];
            } else {
                const float *s0 = f.src[0] + (int64_t)n * 3 * VM;
                latch_rotations(s0, s0 + VM, s0 + 2 * VM, M, jt, rot[own]);
                latched = true;
            }
        }
        __syncthreads();
        const int work = r * ns * G;
        for (int w = threadIdx.x; w < work; w += PN_THREADS) {
            const int q = w % G, s = (w / G) % ns, fr = w / (G * ns);
            const int n4 = VM - 4 * q < 4 ? VM - 4 * q : 4;
            const int64_t base = (int64_t)(n0 + s) * 3 * VM;
            const float *s0 = f.src[fr] + base;
            float *d0 = f.dst[fr] + base;
            normalise4(s0, s0 + VM, s0 + 2 * VM, d0, d0 + VM, d0 + 2 * VM, 4 * q, n4, VM, M, rot[s]);
        }
        __syncthreads();                                // every read of this chunk's state and of its LDS copy has returned
        if (update && latched) {
            const int n = n0 + own;
            for (int i = 0; i < 18; ++i) rot_state[(int64_t)n * 18 + i] = rot[own][i];
            has_rot[n] = 1;
        }
        __syncthreads();                                // before the next chunk overwrites rot
    }
}

int check_joints(const char *who, int V, int z0, int z1, int x0, int x1, Joints *jt) {
    if (V < 2) CSK_REJECT("%s: the centre is joint 1: V >= 2, got %d", who, V);
    const int idx[4] = {z0, z1, x0, x1};
    const char *name[4] = {"zaxis[0]", "zaxis[1]", "xaxis[0]", "xaxis[1]"};
    for (int i = 0; i < 4; ++i)
        if (idx[i] < 0 || idx[i] >= V) CSK_REJECT("%s: joint %s = %d outside [0, %d)", who, name[i], idx[i], V);
    *jt = {z0, z1, x0, x1};
    return 0;
}

}  // namespace

extern "C" int csk_prenorm_f32(const float *x, float *out, int N, int T, int V, int M, int zaxis0, int zaxis1, int xaxis0, int xaxis1,
                               void *stream) {
    if (!x || !out) CSK_FAIL("prenorm: null pointer");
    if (x == out) CSK_FAIL("prenorm: out must not be x (a frame's centre is read after it is written)");
    if (N <= 0 || T <= 0 || V <= 0 || M <= 0) CSK_FAIL("prenorm: bad dims");
    Joints jt;
    if (const int rc = check_joints("prenorm", V, zaxis0, zaxis1, xaxis0, xaxis1, &jt)) return rc;
    if ((int64_t)T * V * M >= (1ll << 29)) CSK_FAIL("prenorm: a sample's channel plane is too large for 32-bit positions");
    const int VM = V * M;
    const int FT = PN_POSITIONS / VM > 1 ? PN_POSITIONS / VM : 1;
    const int per_sample = (T + FT - 1) / FT;
    const int64_t items = (int64_t)N * per_sample;
    const dim3 grid((unsigned)(items < 65536 ? items : 65536)), block(PN_THREADS);
    hipLaunchKernelGGL(prenorm_clip_kernel, grid, block, 0, (hipStream_t)stream, x, out, items, per_sample, FT, T, VM, M, jt);
    return (int)hipGetLastError();
}

extern "C" int csk_prenorm_frames_f32(const float *const *frames, float *const *dst, int r, double *rot, int32_t *has_rot, int update,
                                      int N, int V, int M, int zaxis0, int zaxis1, int xaxis0, int xaxis1, void *stream) {
    if (!frames || !dst) CSK_FAIL("prenorm_frames: null pointer");
    if (r < 1 || r > 8) CSK_REJECT("prenorm_frames: a cycle holds 1..8 frames, got %d", r);
    if (N <= 0 || V <= 0 || M <= 0) CSK_FAIL("prenorm_frames: bad dims");
    Joints jt;
    if (const int rc = check_joints("prenorm_frames", V, zaxis0, zaxis1, xaxis0, xaxis1, &jt)) return rc;
    if (!rot || !has_rot) CSK_FAIL("prenorm_frames: the latched rotations (rot) and their flags (has_rot) are missing");
    if ((int64_t)N * 3 * V * M >= (1ll << 31)) CSK_FAIL("prenorm_frames: frame too large for 32-bit element indices");
    PnFrames f;
    for (int i = 0; i < 8; ++i) {
        f.src[i] = frames[i < r ? i : r - 1];
        f.dst[i] = dst[i < r ? i : r - 1];
        if (!f.src[i] || !f.dst[i]) CSK_FAIL("prenorm_frames: null frame");
    }
    for (int i = 0; i < r; ++i)
        for (int k = 0; k < r; ++k)
            if (f.dst[i] == f.src[k] || (k != i && f.dst[i] == f.dst[k]))
                CSK_FAIL("prenorm_frames: every dst must be a buffer of its own, none of them a source frame");
    const int VM = V * M;
    int S = PN_POSITIONS / (3 * VM);                    // streams per chunk: about PN_POSITIONS floats, 1..PN_MAX_S
    S = S < 1 ? 1 : (S > PN_MAX_S ? PN_MAX_S : S);
    const int chunks = (N + S - 1) / S;
    const dim3 grid((unsigned)(chunks < 65536 ? chunks : 65536)), block(PN_THREADS);
    hipLaunchKernelGGL(prenorm_frames_kernel, grid, block, 0, (hipStream_t)stream, f, r, rot, has_rot, update, N, S, VM, M, jt);
    return (int)hipGetLastError();
}
