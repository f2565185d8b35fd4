// str.hip -- S-TR spatial-attention graph unit (GcnUnitAttention, models/s_tr/s_tr.py:303-477, only_attention form):
//     x^  = data_bn(x)                                    per-(c, v) affine, applied while x is staged      (s_tr.py:432-435)
//     qkv = W_qkv x^ + b_qkv                              1x1 conv, q rows pre-scaled by dkh^-0.5            (s_tr.py:199-230)
//     o   = per frame and head: softmax_j(q_i . k_j) v_j  Nh = 8 heads over the V joints of a frame         (s_tr.py:134-197)
//     y   = ReLU(W_out' o + b_out' + s_c x)               attn_out with BN folded in; s_c x = the skip       (s_tr.py:462-477)
// Three launches, split at two HBM buffers (scratch): (1) data_bn + QKV GEMM, (2) attention, (3) output projection + epilogue.
// Both GEMMs are one fp32-MFMA kernel (v_mfma_f32_32x32x2_f32): a 64-row x 256-column tile, 16-channel K chunks staged
// through LDS with a register prefetch of the next chunk.  The attention runs on VALU from an LDS image of one frame.
//
// Addressing (x, y): element (seg, c, f, v) at seg * seg_stride + c * chan_stride + f * V + v -- one entry serves the clip
// layout (seg = sample, chan stride = T V) and the continual channel-major ring slots (seg = slot, chan stride = P,
// frames = skeletons).  The scratch buffers are dense: qkv [n_seg][2 dk + dv][frames V], o [n_seg][dv][frames V].
#include "mfma_core.h"

namespace {

constexpr int SG_MT = 64;            // packed weights pad rows (GEMM M) to a multiple of this
constexpr int SG_NT = 256;           // columns per tile (4 waves x 64)
constexpr int SG_KC = 16;            // K chunk
constexpr int SG_XLD = SG_NT + 32;   // LDS row stride: the two k rows of an MFMA k-step land on opposite bank halves

struct StrGemmParams {
    const float *x;                  // B operand rows [seg][K][cols]
    int64_t x_seg, x_chan;
    const float *w;                  // packed [K][Mpad] (row m of the conv = column m), rows >= M zero
    const float *bias;               // [Mpad]
    const float *in_scale, *in_shift;// [K][V] affine applied at staging (data_bn), or unused
    const float *res;                // residual rows [seg][M][cols] times res_scale[m] (the skip), or unused
    int64_t r_seg, r_chan;
    const float *res_scale;
    float *y;
    int64_t y_seg, y_chan;
    int K, M, Mpad, ncols, V;
    unsigned vmagic, mtiles, ctiles;
};

// y[m, col] = (RELU ?)( sum_k w[k][m] * x'[k, col] + bias[m] (+ res_scale[m] * res[m, col]) ),  x' = AFFINE ? s[k,v] x + t[k,v] : x
// A tile is 32 MI rows x 256 columns; a wave owns all its rows x 64 columns (MI x 2 accumulators of 32 x 32).  MI = 4 (128
// rows) halves the staging of x per MFMA against MI = 2 (see launch_str_gemm for where it is taken).
template <int MI, bool AFFINE, bool RES, bool RELU>
__global__ __launch_bounds__(NTHREADS, 2) void str_gemm_kernel(const StrGemmParams p) {
    constexpr int MT = 32 * MI, WLD = MT + 32, M4 = MT / 4, WB = SG_KC * M4 / NTHREADS;
    static_assert(WB * NTHREADS == SG_KC * M4, "whole weight vectors per thread");
    __shared__ __attribute__((aligned(16))) float Wl[SG_KC * WLD];
    __shared__ __attribute__((aligned(16))) float Xl[SG_KC * SG_XLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kh = lane >> 5;
    const unsigned wid = xcd_contiguous_id(blockIdx.x, gridDim.x);
    const int mt = (int)(wid % p.mtiles), ct = (int)((wid / p.mtiles) % p.ctiles);
    const int seg = (int)(wid / (p.mtiles * p.ctiles));
    const int m0 = mt * MT, col0 = ct * SG_NT;

    // staging: thread tid owns column col0 + tid (clamped into the row; the surplus columns are never stored) of all KC rows,
    // and WB 16-byte vectors of the weight chunk (vector e = u * 256 + tid: chunk row e / M4, rows m0 + 4 (e % M4) ..)
    const int scol = min(col0 + tid, p.ncols - 1);
    const int sv = scol - div_magic(scol, p.vmagic) * p.V;
    const float *xs = p.x + (int64_t)seg * p.x_seg + scol;
    const int wr = tid / M4, wc = (tid % M4) * 4, wstep = NTHREADS / M4;       // vector u: chunk row wr + u * wstep
    const float *ws = p.w + (int64_t)wr * p.Mpad + m0 + wc;
    float xv[SG_KC];
    f32x4 wv[WB];
    auto issue = [&](int k0) {
#pragma unroll
        for (int r = 0; r < SG_KC; ++r) xv[r] = xs[(int64_t)(k0 + r) * p.x_chan];
        if (AFFINE) {
#pragma unroll
            for (int r = 0; r < SG_KC; ++r)
                xv[r] = __builtin_fmaf(xv[r], p.in_scale[(k0 + r) * p.V + sv], p.in_shift[(k0 + r) * p.V + sv]);
        }
#pragma unroll
        for (int u = 0; u < WB; ++u) wv[u] = *reinterpret_cast<const f32x4 *>(ws + (int64_t)(k0 + u * wstep) * p.Mpad);
    };
    f32x16 acc[MI][2];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = p.K / SG_KC;
    issue(0);
    for (int kc = 0; kc < nk; ++kc) {
        __syncthreads();                                  // the previous chunk's fragment reads are done
#pragma unroll
        for (int r = 0; r < SG_KC; ++r) Xl[r * SG_XLD + tid] = xv[r];
#pragma unroll
        for (int u = 0; u < WB; ++u) *reinterpret_cast<f32x4 *>(Wl + (wr + u * wstep) * WLD + wc) = wv[u];
        __syncthreads();
        if (kc + 1 < nk) issue((kc + 1) * SG_KC);         // in flight under this chunk's MFMAs
        const float *wl = Wl + kh * WLD + l31;
        const float *xl = Xl + kh * SG_XLD + wave * 64 + l31;
#pragma unroll
        for (int s = 0; s < SG_KC / 2; ++s) {
            const float b0 = xl[2 * s * SG_XLD], b1 = xl[2 * s * SG_XLD + 32];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const float a = wl[2 * s * WLD + 32 * mi];
                acc[mi][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[mi][0], 0, 0, 0);
                acc[mi][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[mi][1], 0, 0, 0);
            }
        }
    }

    // epilogue: C/D of 32x32: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    float *yb = p.y + (int64_t)seg * p.y_seg;
    const float *rb = RES ? p.res + (int64_t)seg * p.r_seg : nullptr;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int col = col0 + wave * 64 + ni * 32 + l31;
        if (col >= p.ncols) continue;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (m >= p.M) continue;
                float v = acc[mi][ni][r] + p.bias[m];
                if (RES) v = __builtin_fmaf(p.res_scale[m], rb[(int64_t)m * p.r_chan + col], v);
                if (RELU) v = relu_nan(v);
                yb[(int64_t)m * p.y_chan + col] = v;
            }
        }
    }
}

// One frame per workgroup: the frame's 2 dk + dv qkv rows x V joints are staged in LDS; thread (h, i) (h < 8 heads, i < V
// query joints) forms its V logits, the softmax over the key index j with max subtraction and expf, and the dvh outputs
// o[h dvh + d][i] = sum_j w_j v[h dvh + d][j].  dkh = DKH, dvh = 4 DKH (dk = C_out / 4, dv = C_out, Nh = 8).
template <int V, int DKH>
__global__ __launch_bounds__(NTHREADS) void str_attention_kernel(const float *__restrict__ qkv, float *__restrict__ o,
                                                                  int frames, int ncols) {
    constexpr int NH = 8, DK = NH * DKH, DVH = 4 * DKH, DV = NH * DVH, R = 2 * DK + DV;
    static_assert(NH * V <= NTHREADS, "one thread per (head, query joint)");
    __shared__ float S[R * V];
    const int tid = threadIdx.x;
    const int seg = blockIdx.x / frames, f = blockIdx.x - seg * frames;
    const float *src = qkv + (int64_t)seg * R * ncols + f * V;
    for (int e = tid; e < R * V; e += NTHREADS) {
        const int row = e / V, j = e - row * V;
        S[e] = src[(int64_t)row * ncols + j];
    }
    __syncthreads();
    if (tid >= NH * V) return;
    const int h = tid / V, i = tid - h * V;
    float q[DKH];
#pragma unroll
    for (int d = 0; d < DKH; ++d) q[d] = S[(h * DKH + d) * V + i];
    const float *kr = S + (DK + h * DKH) * V;
    float l[V];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        float a = 0.f;
#pragma unroll
        for (int d = 0; d < DKH; ++d) a = __builtin_fmaf(q[d], kr[d * V + j], a);
        l[j] = a;
        mx = fmaxf(mx, a);
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        l[j] = expf(l[j] - mx);
        sum += l[j];
    }
    const float inv = 1.f / sum;
#pragma unroll
    for (int j = 0; j < V; ++j) l[j] *= inv;
    const float *vr = S + (2 * DK + h * DVH) * V;
    float *dst = o + (int64_t)seg * DV * ncols + (int64_t)(h * DVH) * ncols + f * V + i;
    for (int d = 0; d < DVH; ++d) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) a = __builtin_fmaf(l[j], vr[d * V + j], a);
        dst[(int64_t)d * ncols] = a;
    }
}

// The row tile is a function of the launch kind and M only.  The QKV launch (AFFINE: data_bn applied at staging, the costly
// part of its chunk) takes 128 rows where the packed width Mpad is a multiple of 128 (M = 96, 384; no tile reads weight columns
// beyond Mpad); the output projection and M = 192 take 64 rows.  Measured at NTU batch 256 (profiles/HISTORY.md round 8): 128-row
// tiles cut the 256-channel QKV launch from 3.21 to 2.69 ms but slowed every output projection (128 ch: 1.15 -> 1.65 ms).
// The ONE copy of the rule: launch_str_gemm switches on it, csk_str_unit_f32_route reports it.  Host arithmetic only.
struct StrGemmTiling {
    int Mpad, mi;                    // packed width; MI of the instantiation (4: 128-row tiles, 2: 64-row tiles)
    unsigned mtiles, ctiles, grid;
};
StrGemmTiling str_gemm_tiling(bool affine, int M, int ncols, int n_seg) {
    StrGemmTiling t;
    t.Mpad = round_up(M, SG_MT);
    const bool wide = affine && M > 64 && t.Mpad % 128 == 0;
    t.mi = wide ? 4 : 2;
    t.mtiles = (unsigned)(t.Mpad / (wide ? 128 : 64));
    t.ctiles = (unsigned)((ncols + SG_NT - 1) / SG_NT);
    t.grid = t.mtiles * t.ctiles * (unsigned)n_seg;
    return t;
}

template <bool AFFINE, bool RES, bool RELU>
int launch_str_gemm(StrGemmParams &p, int n_seg, hipStream_t s) {
    const StrGemmTiling t = str_gemm_tiling(AFFINE, p.M, p.ncols, n_seg);
    p.Mpad = t.Mpad;
    p.mtiles = t.mtiles;
    p.ctiles = t.ctiles;
    p.vmagic = vmagic_of(p.V);
    const dim3 grid(t.grid);
    if constexpr (AFFINE) {
        if (t.mi == 4) {
            hipLaunchKernelGGL((str_gemm_kernel<4, AFFINE, RES, RELU>), grid, dim3(NTHREADS), 0, s, p);
            return (int)hipGetLastError();
        }
    }
    hipLaunchKernelGGL((str_gemm_kernel<2, AFFINE, RES, RELU>), grid, dim3(NTHREADS), 0, s, p);
    return (int)hipGetLastError();
}

template <int V, int DKH>
int launch_str_attention(const float *qkv, float *o, int n_seg, int frames, hipStream_t s) {
    hipLaunchKernelGGL((str_attention_kernel<V, DKH>), dim3((unsigned)(n_seg * frames)), dim3(NTHREADS), 0, s, qkv, o, frames,
                       frames * V);
    return (int)hipGetLastError();
}

template <int V>
int launch_str_attention_v(int dkh, const float *qkv, float *o, int n_seg, int frames, hipStream_t s) {
    switch (dkh) {
    case 1: return launch_str_attention<V, 1>(qkv, o, n_seg, frames, s);
    case 2: return launch_str_attention<V, 2>(qkv, o, n_seg, frames, s);
    case 4: return launch_str_attention<V, 4>(qkv, o, n_seg, frames, s);
    default: return launch_str_attention<V, 8>(qkv, o, n_seg, frames, s);
    }
}

}  // namespace

#define CSK_UNSUPPORTED(...)                            \
    do {                                                \
        snprintf(csk_err_buf(), 256, __VA_ARGS__);      \
        return -2;                                      \
    } while (0)

// The shape arguments of the unit, refused or accepted in one place for the entry and for the route query: -1 / -2 with the message
// set, or 0 with dkh and the row count of the qkv image.
static int str_unit_shape(int n_seg, int c_in, int c_out, int frames, int V, bool has_res, int *dkh_out, int *rows_out) {
    if (n_seg <= 0 || frames <= 0 || c_in <= 0 || c_out <= 0) CSK_FAIL("str_unit: n_seg, frames, c_in, c_out must be positive");
    if (V != 18 && V != 25) CSK_UNSUPPORTED("str_unit: built for V in {18, 25}, got V = %d", V);
    const int dk = c_out / 4, dkh = dk / 8;
    if (c_out % 32 || (dkh != 1 && dkh != 2 && dkh != 4 && dkh != 8))
        CSK_UNSUPPORTED("str_unit: built for C_out in {32, 64, 128, 256} (dkh = C_out / 32 in {1, 2, 4, 8}), got C_out = %d", c_out);
    if (c_in % SG_KC) CSK_UNSUPPORTED("str_unit: C_in must be a multiple of %d, got %d", SG_KC, c_in);
    if (has_res && c_in != c_out) CSK_FAIL("str_unit: the skip (res_scale) needs C_in == C_out (s_tr.py:468)");
    const int64_t ncols = (int64_t)frames * V;
    const int rows = 2 * dk + c_out;
    if ((int64_t)n_seg * frames >= (1ll << 31) || (int64_t)rows * ncols >= (1ll << 31) ||
        (int64_t)n_seg * ((ncols + SG_NT - 1) / SG_NT) * (round_up(rows, SG_MT) / SG_MT) >= (1ll << 31))
        CSK_FAIL("str_unit: launch too large");
    *dkh_out = dkh;
    *rows_out = rows;
    return 0;
}

extern "C" int csk_str_unit_f32_route(int n_seg, int c_in, int c_out, int frames, int V, int has_res, int32_t *route) {
    if (!route) CSK_FAIL("str_unit_route: null route");
    int dkh, rows;
    if (const int rc = str_unit_shape(n_seg, c_in, c_out, frames, V, has_res != 0, &dkh, &rows)) return rc;
    const int ncols = frames * V;
    const StrGemmTiling a = str_gemm_tiling(true, rows, ncols, n_seg), b = str_gemm_tiling(false, c_out, ncols, n_seg);
    const int32_t r[CSK_STR_ROUTE_WORDS] = {a.mi, (int32_t)a.mtiles, (int32_t)a.ctiles, (int32_t)a.grid, V, dkh, n_seg * frames,
                                            has_res != 0, b.mi, (int32_t)b.mtiles, (int32_t)b.ctiles, (int32_t)b.grid};
    for (int i = 0; i < CSK_STR_ROUTE_WORDS; ++i) route[i] = r[i];
    return 0;
}

extern "C" int csk_str_unit_f32(const float *x, float *y, float *scratch, int64_t scratch_floats, const float *w_qkv,
                                const float *b_qkv, const float *in_scale, const float *in_shift, const float *w_out,
                                const float *b_out, const float *res_scale, int n_seg, int c_in, int c_out, int frames, int V,
                                int64_t x_seg_stride, int64_t x_chan_stride, int64_t y_seg_stride, int64_t y_chan_stride,
                                void *stream) {
    if (!x || !y || !scratch || !w_qkv || !b_qkv || !in_scale || !in_shift || !w_out || !b_out)
        CSK_FAIL("str_unit: null operand");
    int dkh, rows;
    if (const int rc = str_unit_shape(n_seg, c_in, c_out, frames, V, res_scale != nullptr, &dkh, &rows)) return rc;
    const int64_t ncols = (int64_t)frames * V;
    if (x_chan_stride < ncols || y_chan_stride < ncols) CSK_FAIL("str_unit: channel stride shorter than frames * V");
    if (x_seg_stride < 0 || y_seg_stride < 0) CSK_FAIL("str_unit: negative segment stride");
    if (scratch_floats < (int64_t)n_seg * (rows + c_out) * ncols)
        CSK_FAIL("str_unit: scratch holds %lld floats, needs n_seg * (2 dk + 2 dv) * frames * V = %lld", (long long)scratch_floats,
                 (long long)((int64_t)n_seg * (rows + c_out) * ncols));
    if ((reinterpret_cast<uintptr_t>(w_qkv) | reinterpret_cast<uintptr_t>(w_out)) & 15)
        CSK_FAIL("str_unit: packed weights must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float *qkv = scratch, *o = scratch + (int64_t)n_seg * rows * ncols;

    StrGemmParams p{};
    p.x = x; p.x_seg = x_seg_stride; p.x_chan = x_chan_stride;
    p.w = w_qkv; p.bias = b_qkv; p.in_scale = in_scale; p.in_shift = in_shift;
    p.y = qkv; p.y_seg = (int64_t)rows * ncols; p.y_chan = ncols;
    p.K = c_in; p.M = rows; p.ncols = (int)ncols; p.V = V;
    int rc = launch_str_gemm<true, false, false>(p, n_seg, s);
    if (rc) return rc;

    rc = V == 18 ? launch_str_attention_v<18>(dkh, qkv, o, n_seg, frames, s) : launch_str_attention_v<25>(dkh, qkv, o, n_seg, frames, s);
    if (rc) return rc;

    StrGemmParams q{};
    q.x = o; q.x_seg = (int64_t)c_out * ncols; q.x_chan = ncols;
    q.w = w_out; q.bias = b_out;
    q.res = x; q.r_seg = x_seg_stride; q.r_chan = x_chan_stride;
    q.res_scale = res_scale;
    q.y = y; q.y_seg = y_seg_stride; q.y_chan = y_chan_stride;
    q.K = c_out; q.M = c_out; q.ncols = (int)ncols; q.V = V;
    return res_scale ? launch_str_gemm<false, true, true>(q, n_seg, s) : launch_str_gemm<false, false, true>(q, n_seg, s);
}
