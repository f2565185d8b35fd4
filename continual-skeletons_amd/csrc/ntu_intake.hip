// ntu_intake.hip -- NTU RGB+D body intake for whole clips on the device (csk_ntu_intake_f32; include/cskel.h).
// Counterpart of the first two thirds of the reference's offline NTU pipeline: read_xyz's choice of the bodies with the largest
// motion energy (datasets/data_preparation/ntu60_prep.py:101-128), gendata's placement into max_frame frames (:169-177) and the
// null-frame padding that opens pre_normalization (preprocess.py:18-39).  bodies (N, T, P, V, 3) -> out (N, 3, T_out, V, M).
// One workgroup of 16 waves per clip; an item is one (frame, body) = V * 3 contiguous floats, read by one wave (lane l takes the
// elements l, l + 64, l + 128; 64 = 1 mod 3, so element slot k of lane l is coordinate (l + k) mod 3).  Wave w owns the frames
// t = w mod 16 and walks them in ascending order, four frames' loads in flight, once per body:
//   pass 1  null flags (ballot of "any element != 0") into LDS and the fp64 coordinate sums (a null frame adds exact zeros)
//   pass 2  the fp64 squared deviations of the non-null frames from the means
// each followed by a butterfly over the lanes and a sum over the waves in wave order: the order of every sum is a function of
// (T, V) alone -- the same for every body, clip and batch.  Then one lane per body ranks the energies, one wave per kept body
// scans its flags into a table of source frames (ballot + popcount prefix), and all waves gather the output rows (c, t), V * M
// consecutive floats each.  Every index comes from the flags, never from a value: NaN coordinates cannot leave the operands.
#include "mfma_core.h"

namespace {

constexpr int NI_THREADS = 1024, NI_WAVES = NI_THREADS / 64;
constexpr int NI_MAX_P = 8, NI_MAX_V = 64, NI_SLOTS = NI_MAX_V * 3 / 64;    // element slots of a lane: 3
constexpr int NI_MAX_T = 1024;          // frames of the output, at most (CSK_NTU_MAX_FRAMES): the tables below live in LDS
constexpr int NI_FRAMES = 4;            // frames a wave loads before it reduces them (in ascending order)
constexpr int NI_ROWS = 4;              // output rows a wave gathers before it stores them
static_assert(NI_MAX_T == CSK_NTU_MAX_FRAMES && NI_MAX_T <= 65536, "the source-frame table holds 16-bit frame indices");

#define CSK_REJECT(...)                                 \
    do {                                                \
        snprintf(csk_err_buf(), 256, __VA_ARGS__);      \
        return -2;                                      \
    } while (0)

__device__ __forceinline__ double wave_sum(double v) {        // xor butterfly: every lane ends with the same bits
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// the slot of this lane that holds coordinate c: k with (l3 + k) mod 3 == c
__device__ __forceinline__ double slot_of(const double (&a)[NI_SLOTS], int l3, int c) {
    const int k = (c - l3 + 3) % 3;
    return k == 0 ? a[0] : k == 1 ? a[1] : a[2];
}

// q is placed before p (q != p): the larger energy first, equal energies the HIGHER index first (numpy's argsort()[::-1]);
// a NaN energy behind every number -- a total order, so the ranks are a permutation whatever the data
__device__ __forceinline__ bool placed_before(double eq, int q, double ep, int p) {
    const bool nq = eq != eq, np = ep != ep;
    if (nq || np) return nq == np ? q > p : np;
    return eq > ep || (eq == ep && q > p);
}

__global__ __launch_bounds__(NI_THREADS) void ntu_intake_kernel(const float *__restrict__ bodies, float *__restrict__ out, int T, int P,
                                                                int V, int M, int T_out) {
    __shared__ unsigned char flag[NI_MAX_P * NI_MAX_T];         // [p][t], stride T: frame t of body p is non-null
    __shared__ unsigned short table[NI_MAX_P * NI_MAX_T];       // [m][j], stride NI_MAX_T: source frame of position j < len[m]
    __shared__ double wsum[NI_MAX_P][NI_WAVES][3];
    __shared__ int wcnt[NI_MAX_P][NI_WAVES];
    __shared__ double mean[NI_MAX_P][3], energy[NI_MAX_P];
    __shared__ int count[NI_MAX_P], sel[NI_MAX_P], len[NI_MAX_P];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, l3 = lane % 3;
    const int V3 = V * 3, PV3 = P * V3;
    const float *clip = bodies + (int64_t)blockIdx.x * T * PV3;
    float *dst = out + (int64_t)blockIdx.x * 3 * T_out * V * M;

    for (int pass = 0; pass < 2; ++pass) {
        for (int p = 0; p < P; ++p) {
            double acc[NI_SLOTS] = {0.0, 0.0, 0.0}, mu[NI_SLOTS];
            int cnt = 0;
#pragma unroll
            for (int k = 0; k < NI_SLOTS; ++k) mu[k] = pass ? mean[p][(l3 + k) % 3] : 0.0;
            for (int t0 = wave; t0 < T; t0 += NI_WAVES * NI_FRAMES) {       // uniform per wave (ballots inside)
                float x[NI_FRAMES][NI_SLOTS];
#pragma unroll
                for (int u = 0; u < NI_FRAMES; ++u) {
                    const int t = t0 + u * NI_WAVES;
#pragma unroll
                    for (int k = 0; k < NI_SLOTS; ++k) {
                        const int e = lane + 64 * k;
                        x[u][k] = t < T && e < V3 ? clip[(t * P + p) * V3 + e] : 0.f;
                    }
                }
#pragma unroll
                for (int u = 0; u < NI_FRAMES; ++u) {
                    const int t = t0 + u * NI_WAVES;
                    if (pass == 0) {
                        const bool any = __ballot(x[u][0] != 0.f || x[u][1] != 0.f || x[u][2] != 0.f) != 0ull;   // -0.0 is zero
                        if (t < T) {
                            if (lane == 0) flag[p * T + t] = any;
                            cnt += any;
                        }
#pragma unroll
                        for (int k = 0; k < NI_SLOTS; ++k) acc[k] += (double)x[u][k];
                    } else if (t < T && flag[p * T + t]) {
#pragma unroll
                        for (int k = 0; k < NI_SLOTS; ++k) {
                            const double d = (double)x[u][k] - mu[k];
                            if (lane + 64 * k < V3) acc[k] += d * d;
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double s = wave_sum(slot_of(acc, l3, c));
                if (lane == 0) wsum[p][wave][c] = s;
            }
            if (pass == 0 && lane == 0) wcnt[p][wave] = cnt;
        }
        __syncthreads();
        if (pass == 0) {
            if (tid < P * 3) {                                              // means over (non-null frames x V)
                const int p = tid / 3, c = tid - p * 3;
                double s = 0.0;
                int n = 0;
                for (int w = 0; w < NI_WAVES; ++w) {
                    s += wsum[p][w][c];
                    n += wcnt[p][w];
                }
                mean[p][c] = n ? s / ((double)n * V) : 0.0;
                if (c == 0) count[p] = n;
            }
        } else if (tid < P) {                                               // energy = sum over c of the population std
            double e = 0.0;
            if (count[tid])
                for (int c = 0; c < 3; ++c) {
                    double ss = 0.0;
                    for (int w = 0; w < NI_WAVES; ++w) ss += wsum[tid][w][c];
                    e += sqrt(ss / ((double)count[tid] * V));
                }
            energy[tid] = e;
        }
        __syncthreads();
    }
    if (tid < P) {
        int rank = 0;
        for (int q = 0; q < P; ++q)
            if (q != tid && placed_before(energy[q], q, energy[tid], tid)) ++rank;
        sel[rank] = tid;
    }
    __syncthreads();
    if (wave < M) {                                                         // M <= 8 < NI_WAVES: one wave per kept body
        const unsigned char *fl = flag + sel[wave] * T;
        unsigned short *tb = table + wave * NI_MAX_T;
        const bool compact = fl[0] == 0;                                    // frame 0 null: the non-null frames move to the front
        int run = 0, last = -1;
        for (int base = 0; base < T; base += 64) {
            const int t = base + lane;
            const bool f = t < T && fl[t];
            const unsigned long long mask = __ballot(f);
            if (compact) {
                if (f) tb[run + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)t;
                run += __popcll(mask);
            } else if (mask) {
                last = base + 63 - __clzll((long long)mask);
            }
        }
        const int L = compact ? run : last + 1;                             // frame 0 present: gaps stay, the clip ends at its last frame
        if (!compact)
            for (int j = lane; j < L; j += 64) tb[j] = (unsigned short)j;
        if (lane == 0) len[wave] = L;
    }
    __syncthreads();
    const int VM = V * M, rows = 3 * T_out;
    for (int e = lane; e < VM; e += 64) {
        const int v = e / M, m = e - v * M, L = len[m];
        const int off = sel[m] * V3 + v * 3;
        const unsigned short *tb = table + m * NI_MAX_T;
        for (int r0 = wave * NI_ROWS; r0 < rows; r0 += NI_WAVES * NI_ROWS) {
            float val[NI_ROWS];
#pragma unroll
            for (int u = 0; u < NI_ROWS; ++u) {
                const int row = r0 + u, c = row / T_out, t = row - c * T_out;
                val[u] = 0.f;                                               // an empty body: +0
                if (row < rows && L) val[u] = clip[(int)tb[t % L] * PV3 + off + c];
            }
#pragma unroll
            for (int u = 0; u < NI_ROWS; ++u)
                if (r0 + u < rows) dst[(r0 + u) * VM + e] = val[u];
        }
    }
}

}  // namespace

extern "C" int csk_ntu_intake_f32(const float *bodies, float *out, int N, int T, int P, int V, int M, int T_out, void *stream) {
    if (!bodies || !out) CSK_FAIL("ntu_intake: null pointer");
    if (bodies == out) CSK_FAIL("ntu_intake: out must not be bodies (every output frame is gathered from the whole clip)");
    if (N <= 0 || T <= 0 || P <= 0 || V <= 0 || M <= 0 || T_out <= 0) CSK_FAIL("ntu_intake: bad dims");
    if (P > NI_MAX_P || M > P) CSK_REJECT("ntu_intake: 1 <= M <= P <= %d bodies, got M = %d, P = %d", NI_MAX_P, M, P);
    if (V > NI_MAX_V) CSK_REJECT("ntu_intake: 1 <= V <= %d joints, got %d", NI_MAX_V, V);
    if (T_out < T || T_out > NI_MAX_T) CSK_REJECT("ntu_intake: T <= T_out <= %d frames, got T = %d, T_out = %d", NI_MAX_T, T, T_out);
    hipLaunchKernelGGL(ntu_intake_kernel, dim3((unsigned)N), dim3(NI_THREADS), 0, (hipStream_t)stream, bodies, out, T, P, V, M, T_out);
    return (int)hipGetLastError();
}
