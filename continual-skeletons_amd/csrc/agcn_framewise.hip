// agcn_framewise.hip -- the adaptive graph-conv stage of A-GCN applied PER FRAME to a whole clip tensor on gfx950: for every
// (segment, frame) exactly what the step form computes for that skeleton frame (models/coa_gcn/coa_gcn.py:11-14, the module's
// forward_stepping; agcn.py: AdaptiveGraphConvolution.stage), in ONE launch and without the per-frame adjacencies ever
// reaching memory.  Per frame f of segment n (x_f = x[n, :, f, :], C_in x V):
//     E_f          = W_e x_f + b_e                                          six 1x1 embedding convs, 6 inter rows (pair-major)
//     L_i[v, w]    = sum_k Ea_i[k, v] Eb_i[k, w] / inter                    i = 0, 1, 2
//     adj_i[v, w]  = softmax over v of L_i[., w] + a_sum_i[v, w]            a_sum = A + graph_attn
//     y_f          = ReLU( sum_i W'_i (x_f adj_i) + b' + gcn_residual(x_f) )   BN folded; residual = identity or 4th subset
// A workgroup owns a tile of FT = 128 / V whole frames of one segment (a wave = 32 columns, as in gcn_dense.hip) and runs
//   (1) per pair i: the embedding GEMM of its 2 inter rows over C_in (fp32 MFMA, 16-channel chunks, ping-pong LDS, register
//       prefetch), the E tile to LDS, then per frame one wave forms logits (inter / 2 MFMAs) and the softmax in registers --
//       the arithmetic of agcn_embed_attention_kernel's step form in agcn.hip, operand for operand -- and writes
//       adj[i][f][w][v] to LDS (3 FT V V floats: 27 KB at V = 18, 37.5 KB at V = 25);
//   (2) every lane loads the 3 V adjacency values of ITS output column (f, w) from LDS into registers, and the stage runs as in
//       gcn_dense.hip: B_i[c][f, w] = sum_v x[c][f, v] adj_i[f][v, w] on the vector ALU (even and odd joints in separate chains,
//       then one add) feeding the fp32-MFMA channel mix, for the C_out / MT row tiles in turn, epilogue as there.
// x is read once per pair and once per row tile (from L2 after the first pass).  The LDS work area is shared by the phases:
//   inter = 16: 63 KB, inter = 32: 79 KB (two workgroups per CU), inter = 64: 105 KB (one: the 128-row E tile of a pair).
// Built for V in {18, 25}, inter in {16, 32, 64} with C_out = 4 inter (the module's coff_embedding), any C_in.
// Every output column depends on its own frame only and is formed by the same instruction sequence wherever the frame sits in
// a tile: a frame's bits do not depend on T, on the tile it falls into or on its neighbours.
#include <type_traits>

#include "mfma_core.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float fw_exp(float x) { return __expf(x); }      // as sm_exp / sm_rcp of agcn.hip
__device__ __forceinline__ float fw_rcp(float sum) { return 1.f / sum; }

struct FwParams {
    const float *x, *w, *bias, *we, *be, *a_sum;
    float *y;
    int64_t x_seg_stride, x_chan_stride, y_seg_stride, y_chan_stride;
    int Cin, CinPad, Cout, Mpad, EMpad, frames, ident;
    unsigned qtiles;
};

template <int INTER, int V>
struct FwShape {
    static constexpr int VPAD = (V + 3) & ~3, FT = 128 / V, LDX = FT * VPAD;
    static constexpr int EMT = 2 * INTER, EKC = 16, EBUF = EKC * EMT + EKC * LDX, ESLD = 128 + 4;
    static constexpr int MT = INTER == 16 ? 64 : 128, KC2 = 8;
    static constexpr int ADJ = (3 * FT * V * V + 3) & ~3;
    static constexpr int bufsz(int R) { return R * KC2 * MT + KC2 * LDX; }
    static constexpr int work(int R) {
        int a = 2 * EBUF, b = EMT * ESLD, c = 2 * bufsz(R);
        return a > b ? (a > c ? a : c) : (b > c ? b : c);
    }
    static constexpr size_t lds_bytes(int R) { return (size_t)(ADJ + work(R)) * sizeof(float); }
};

template <int INTER, int V, bool CONVRES>
__global__ __launch_bounds__(NTHREADS, INTER == 64 ? 1 : 2) void agcn_stage_framewise_kernel(const FwParams p) {
    using S = FwShape<INTER, V>;
    constexpr int VP = (V + 1) / 2, VPAD = S::VPAD, FT = S::FT, LDX = S::LDX;
    constexpr bool EVEN = V % 2 == 0;
    constexpr int XSL = EVEN ? 64 : 128, RPS = NTHREADS / XSL;     // staging slots per activation row: joint pairs / joints
    constexpr int EMT = S::EMT, ENB = EMT / 32, EKC = S::EKC, ENS = EKC / 2, EM4 = EMT / 4;
    constexpr int EWB = (EKC * EM4 + NTHREADS - 1) / NTHREADS, EXB = EKC * XSL / NTHREADS;
    constexpr int EWSZ = EKC * EMT, EBUF = S::EBUF, ESLD = S::ESLD;
    constexpr int MT = S::MT, NB = MT / 32, R = CONVRES ? 4 : 3, KC2 = S::KC2, NS = KC2 / 2, M4 = MT / 4;
    constexpr int WB = (R * KC2 * M4 + NTHREADS - 1) / NTHREADS, XB = KC2 * XSL / NTHREADS;
    constexpr int WSZ = R * KC2 * MT, BUFSZ = S::bufsz(R);
    static_assert(FT * V <= 128 && V <= 26 && EMT % 32 == 0 && INTER % 2 == 0, "tile shape");
    extern __shared__ __attribute__((aligned(16))) float smem_fw[];
    float *adjL = smem_fw, *work = smem_fw + S::ADJ;              // adj[i][f][w][v]; staging buffers / E tile

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kh = lane >> 5;
    const unsigned wid = xcd_contiguous_id(blockIdx.x, gridDim.x);
    const int qt = (int)(wid % p.qtiles), seg = (int)(wid / p.qtiles);
    const int Q = p.frames * V;
    const int ta = qt * FT, q0 = ta * V;
    const int fcnt = min(FT, p.frames - ta);                       // frames of this tile
    const int ncol = fcnt * V;
    const int j = wave * 32 + l31;                                 // this lane's column (frame jf, joint jw)
    const bool jv = j < ncol;
    const int jf = jv ? j / V : 0, jw = jv ? j - jf * V : 0;
    const int xcol = jf * VPAD + jw, xoff = jf * VPAD;
    const float *seg_base = p.x + (int64_t)seg * p.x_seg_stride;

    // activation staging, both phases: slot -> (frame, joint pair) with 8-byte loads (even V: every frame of a row starts
    // 8-byte aligned) or (frame, joint); out-of-range slots are clamped: they re-stage the last element
    typedef std::conditional_t<EVEN, f32x2, float> xs_t;
    unsigned xgo, xlo;
    const int xrow0 = tid / XSL;
    if constexpr (EVEN) {
        const int pr = min(tid % XSL, fcnt * VP - 1);
        const int f = pr / VP, w2 = pr - f * VP;
        xgo = (unsigned)(q0 + 2 * pr);
        xlo = (unsigned)(f * VPAD + 2 * w2);
    } else {
        const int e = min(tid % XSL, ncol - 1);
        const int f = e / V;
        xgo = (unsigned)(q0 + e);
        xlo = (unsigned)(f * VPAD + (e - f * V));
    }

    // ---- phase 1: embeddings + attention of the tile's frames, pair by pair -> adjL -------------------------------------
    {
        f32x4 wv[EWB];
        xs_t xv[EXB];
        unsigned wgo[EWB], wlo[EWB];
#pragma unroll
        for (int u = 0; u < EWB; ++u) {
            const int e = min(u * NTHREADS + tid, EKC * EM4 - 1);
            const int row = e / EM4, m4 = e % EM4;
            wgo[u] = (unsigned)(row * p.EMpad + m4 * 4);
            wlo[u] = (unsigned)(e * 4);
        }
        const int nchunks = p.CinPad / EKC;
        const int cl = min(l31, V - 1);
        const float inv = 1.f / (float)INTER;
        const bool col = l31 < V;
#pragma unroll 1
        for (int pr = 0; pr < 3; ++pr) {
            const int m0 = pr * EMT;
            const float *wbase = p.we + m0;
            auto issue = [&](int c0) {
#pragma unroll
                for (int u = 0; u < EWB; ++u) wv[u] = *reinterpret_cast<const f32x4 *>(wbase + (size_t)c0 * p.EMpad + wgo[u]);
#pragma unroll
                for (int u = 0; u < EXB; ++u) {
                    const int c = min(c0 + xrow0 + RPS * u, p.Cin - 1);          // clamped: padding channels carry zero weights
                    xv[u] = *reinterpret_cast<const xs_t *>(seg_base + (int64_t)c * p.x_chan_stride + xgo);
                }
            };
            auto commit = [&](float *buf) {
#pragma unroll
                for (int u = 0; u < EWB; ++u) *reinterpret_cast<f32x4 *>(buf + wlo[u]) = wv[u];
#pragma unroll
                for (int u = 0; u < EXB; ++u) *reinterpret_cast<xs_t *>(buf + EWSZ + (xrow0 + RPS * u) * LDX + xlo) = xv[u];
            };
            f32x16 acc[ENB];
#pragma unroll
            for (int i = 0; i < ENB; ++i)
#pragma unroll
                for (int g = 0; g < 16; ++g) acc[i][g] = 0.f;
            issue(0);
            commit(work);
            if (nchunks > 1) issue(EKC);
            __syncthreads();
            for (int c = 0; c < nchunks; ++c) {
                float *cur = work + (c & 1) * EBUF, *oth = work + ((c & 1) ^ 1) * EBUF;
                if (c + 1 < nchunks) commit(oth);
                if (c + 2 < nchunks) issue((c + 2) * EKC);
#pragma unroll
                for (int s = 0; s < ENS; ++s) {
                    const int kk = 2 * s + kh;
                    const float b = cur[EWSZ + kk * LDX + xcol];
                    const float *wr = cur + kk * EMT + ENB * l31;
#pragma unroll
                    for (int i = 0; i < ENB; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[i], b, acc[i], 0, 0, 0);
                }
                __syncthreads();
            }
            // E tile (+ bias) -> LDS, row-major [tile row][column]: accumulator block i, MFMA row rho is tile row ENB rho + i
            float *Es = work;
#pragma unroll
            for (int i = 0; i < ENB; ++i)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int row = ENB * ((g & 3) + 8 * (g >> 2) + 4 * kh) + i;
                    Es[row * ESLD + j] = acc[i][g] + p.be[m0 + row];
                }
            __syncthreads();
            // one wave per frame: logits = Ea^T . Eb, softmax over v in registers (column w in lanes w and w + 32)
            for (int f = wave; f < fcnt; f += NTHREADS / 64) {
                const float *ea = Es + kh * ESLD + f * V + cl;
                const float *eb = ea + INTER * ESLD;
                f32x16 lg;
#pragma unroll
                for (int g = 0; g < 16; ++g) lg[g] = 0.f;
#pragma unroll 8
                for (int s = 0; s < INTER / 2; ++s) lg = __builtin_amdgcn_mfma_f32_32x32x2f32(ea[2 * s * ESLD], eb[2 * s * ESLD], lg, 0, 0, 0);
                float m = -INFINITY;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int v = (r & 3) + 8 * (r >> 2) + 4 * kh;
                    lg[r] *= inv;
                    if (v < V) m = fmaxf(m, lg[r]);
                }
                m = fmaxf(m, __shfl_xor(m, 32));
                float sum = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int v = (r & 3) + 8 * (r >> 2) + 4 * kh;
                    lg[r] = v < V ? fw_exp(lg[r] - m) : 0.f;
                    sum += lg[r];
                }
                sum += __shfl_xor(sum, 32);
                const float rs = fw_rcp(sum);
                if (col) {
                    float *dst = adjL + ((pr * FT + f) * V + l31) * V;               // [i][f][w][v]
                    const float *as = p.a_sum + (int64_t)pr * V * V + l31;           // [i][v][w]
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int v = (r & 3) + 8 * (r >> 2) + 4 * kh;
                        if (v < V) dst[v] = lg[r] * rs + as[v * V];
                    }
                }
            }
            __syncthreads();                                       // the E tile is rewritten by the next pair / phase 2
        }
    }

    // ---- phase 2: the graph-conv stage with the lane's adjacency columns in registers ---------------------------------------
    f32x2 adj[3][VP];
    {
        const float *ab = adjL + (jf * V + jw) * V;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int i = 0; i < VP; ++i) {
                f32x2 a;
                a[0] = ab[r * FT * V * V + 2 * i];
                a[1] = 2 * i + 1 < V ? ab[r * FT * V * V + min(2 * i + 1, V - 1)] : 0.f;
                adj[r][i] = jv ? a : f32x2{0.f, 0.f};
            }
    }
    f32x4 wv[WB];
    xs_t xv[XB];
    // weight staging: slot u of a thread is element e = u * 256 + tid of the chunk's [R][KC2][MT / 4] vectors.  At MT = 128 that is
    // subset u, channel row tid / 32: the offsets of the slots differ by wave-uniform constants, one register each serves all
    unsigned wgo[WB], wlo[WB];
#pragma unroll
    for (int u = 0; u < WB; ++u) {
        const int e = min(u * NTHREADS + tid, R * KC2 * M4 - 1);
        const int row = e / M4, m4 = e % M4;
        wgo[u] = (unsigned)(((row / KC2) * p.CinPad + (row % KC2)) * p.Mpad + m4 * 4);
        wlo[u] = (unsigned)(e * 4);
    }
    const unsigned wgs = MT == 128 ? (unsigned)(p.CinPad * p.Mpad) : 0u;
    static_assert(MT != 128 || (WB == R && KC2 * M4 == NTHREADS), "one subset per slot");
    const int nchunks = p.CinPad / KC2;
#pragma unroll 1
    for (int m0 = 0; m0 < p.Mpad; m0 += MT) {
        const float *wbase = p.w + m0;
        auto issue = [&](int c0) {
#pragma unroll
            for (int u = 0; u < WB; ++u)
                wv[u] = *reinterpret_cast<const f32x4 *>(wbase + (size_t)c0 * p.Mpad + (MT == 128 ? (size_t)u * wgs + wgo[0] : (size_t)wgo[u]));
#pragma unroll
            for (int u = 0; u < XB; ++u) {
                const int c = min(c0 + xrow0 + RPS * u, p.Cin - 1);
                xv[u] = *reinterpret_cast<const xs_t *>(seg_base + (int64_t)c * p.x_chan_stride + xgo);
            }
        };
        auto commit = [&](float *buf) {
#pragma unroll
            for (int u = 0; u < WB; ++u) *reinterpret_cast<f32x4 *>(buf + (MT == 128 ? u * (KC2 * MT) + wlo[0] : wlo[u])) = wv[u];
#pragma unroll
            for (int u = 0; u < XB; ++u) *reinterpret_cast<xs_t *>(buf + WSZ + (xrow0 + RPS * u) * LDX + xlo) = xv[u];
        };
        f32x16 acc[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[i][g] = 0.f;
        issue(0);
        commit(work);
        if (nchunks > 1) issue(KC2);
        __syncthreads();
        for (int c = 0; c < nchunks; ++c) {
            float *cur = work + (c & 1) * BUFSZ, *oth = work + ((c & 1) ^ 1) * BUFSZ;
            if (c + 1 < nchunks) commit(oth);
            if (c + 2 < nchunks) issue((c + 2) * KC2);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float *bx = cur + WSZ + (2 * s + kh) * LDX + xoff;
                const float *wr = cur + (2 * s + kh) * MT + NB * l31;
                f32x4 xq[VPAD / 4];
#pragma unroll
                for (int i = 0; i < VPAD / 4; ++i) xq[i] = *reinterpret_cast<const f32x4 *>(bx + 4 * i);
                float b[R];
                if constexpr (CONVRES) b[3] = bx[jw];
                // even and odd joints in separate chains, then one add (gcn_dense.hip); odd V: the last pair holds one joint
                f32x2 sum[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
                for (int i = 0; i < VP; ++i) {
                    f32x2 xp = {xq[i / 2][2 * (i & 1)], xq[i / 2][2 * (i & 1) + 1]};
                    if (!EVEN && i == VP - 1) xp[1] = 0.f;         // (the padding slot behind the frame is never read as data)
#pragma unroll
                    for (int r = 0; r < 3; ++r) sum[r] = __builtin_elementwise_fma(xp, adj[r][i], sum[r]);
                }
#pragma unroll
                for (int r = 0; r < 3; ++r) b[r] = sum[r][0] + sum[r][1];
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int i = 0; i < NB; ++i)
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[r * KC2 * MT + i], b[r], acc[i], 0, 0, 0);
            }
            __syncthreads();
        }
        // epilogue: ReLU(acc + bias + identity residual); acc[i][g] of lane (column j, half kh) is output row
        // m0 + NB ((g & 3) + 8 (g >> 2) + 4 kh) + i
        float *oseg = p.y + (int64_t)seg * p.y_seg_stride;
        const int qc = min(q0 + j, Q - 1);
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row = m0 + NB * ((g & 3) + 8 * (g >> 2) + 4 * kh) + i;
                const float bv = p.bias[row];                      // bias is padded to Mpad
                const float r0 = p.ident ? seg_base[(int64_t)min(row, p.Cout - 1) * p.x_chan_stride + qc] : 0.f;
                const float v = relu_nan(acc[i][g] + bv + r0);
                if (jv && row < p.Cout) oseg[(int64_t)row * p.y_chan_stride + q0 + j] = v;
            }
    }
}

template <int INTER, int V, bool CONVRES>
static int launch_framewise(FwParams p, int n_seg, hipStream_t stream) {
    using S = FwShape<INTER, V>;
    const size_t lds = S::lds_bytes(CONVRES ? 4 : 3);
    void (*k)(FwParams) = agcn_stage_framewise_kernel<INTER, V, CONVRES>;
    if (const int e = csk_ensure_lds((const void *)k, lds)) return e;
    hipLaunchKernelGGL(k, dim3(p.qtiles * n_seg), dim3(NTHREADS), lds, stream, p);
    return (int)hipGetLastError();
}

// The ONE copy of the shape rule: the launcher switches on it, the route entry reports it.  Host arithmetic only.
static int framewise_route(const float *x, int n_seg, int c_in, int c_out, int inter, int frames, int V, int64_t x_seg_stride,
                           int64_t x_chan_stride, int res_mode) {
    if (n_seg <= 0 || c_in <= 0 || c_out <= 0 || inter <= 0 || frames <= 0 || V <= 0) CSK_FAIL("agcn_stage_framewise: bad dims");
    if (res_mode != CSK_RES_IDENTITY && res_mode != CSK_RES_CONV) CSK_FAIL("agcn_stage_framewise: res_mode must be identity or conv");
    if (res_mode == CSK_RES_IDENTITY && c_in != c_out) CSK_FAIL("agcn_stage_framewise: identity residual needs c_in == c_out");
    if ((V != 18 && V != 25) || (inter != 16 && inter != 32 && inter != 64) || c_out != 4 * inter) return 0;
    if (V % 2 == 0 && ((reinterpret_cast<uintptr_t>(x) & 7) || (x_seg_stride & 1) || (x_chan_stride & 1))) return 0;
    const int FT = 128 / V;
    if ((int64_t)((frames + FT - 1) / FT) * n_seg >= (1ll << 31) || (int64_t)frames * V >= (1ll << 31)) return 0;
    return inter * 1000 + V * 10 + (res_mode == CSK_RES_CONV ? 1 : 0);
}

extern "C" int csk_agcn_stage_framewise_f32_route(const float *x, int n_seg, int c_in, int c_out, int inter, int frames, int V,
                                                  int64_t x_seg_stride, int64_t x_chan_stride, int res_mode) {
    return framewise_route(x, n_seg, c_in, c_out, inter, frames, V, x_seg_stride, x_chan_stride, res_mode);
}

extern "C" int csk_agcn_stage_framewise_f32(const float *x, float *y, const float *w, const float *bias, const float *w_pairs,
                                            const float *b_pairs, const float *a_sum, int n_seg, int c_in, int c_out, int inter,
                                            int frames, int V, int64_t x_seg_stride, int64_t x_chan_stride, int64_t y_seg_stride,
                                            int64_t y_chan_stride, int res_mode, void *stream) {
    if (!x || !y || !w || !bias || !w_pairs || !b_pairs || !a_sum) CSK_FAIL("agcn_stage_framewise: null pointer");
    const int route = framewise_route(x, n_seg, c_in, c_out, inter, frames, V, x_seg_stride, x_chan_stride, res_mode);
    if (route < 0) return route;
    if (!route)
        CSK_FAIL("agcn_stage_framewise: built for V in {18, 25}, inter in {16, 32, 64}, c_out == 4 * inter and (even V) 8-byte "
                 "aligned rows (compose csk_agcn_embed_attention_f32 / csk_agcn_attention_f32 with csk_gcn_stage_f32)");
    FwParams p;
    p.x = x; p.y = y; p.w = w; p.bias = bias; p.we = w_pairs; p.be = b_pairs; p.a_sum = a_sum;
    p.x_seg_stride = x_seg_stride; p.x_chan_stride = x_chan_stride; p.y_seg_stride = y_seg_stride; p.y_chan_stride = y_chan_stride;
    p.Cin = c_in; p.CinPad = round_up(c_in, CSK_CPAD); p.Cout = c_out; p.Mpad = round_up(c_out, CSK_MT);
    p.EMpad = round_up(6 * inter, CSK_MT); p.frames = frames; p.ident = res_mode == CSK_RES_IDENTITY;
    const int FT = 128 / V;
    p.qtiles = (unsigned)((frames + FT - 1) / FT);
    hipStream_t s = (hipStream_t)stream;
    const bool cr = res_mode == CSK_RES_CONV;
#define CSK_FW(I_, V_) (cr ? launch_framewise<I_, V_, true>(p, n_seg, s) : launch_framewise<I_, V_, false>(p, n_seg, s))
#define CSK_FWV(I_) (V == 18 ? CSK_FW(I_, 18) : CSK_FW(I_, 25))
    return inter == 16 ? CSK_FWV(16) : inter == 32 ? CSK_FWV(32) : CSK_FWV(64);
#undef CSK_FWV
#undef CSK_FW
}
