// gcn.hip -- GCN stage of the ST-GCN / A-GCN forward path (gfx950 / MI355X):
//   y = ReLU( W' . agg(x) + b' + gcn_residual(x) )      models/base.py:260-270, models/a_gcn/a_gcn.py:48-69
// Four kernels and a reduction share GcnParams: gcn_stage_sparse2_kernel (skeleton graphs: the aggregated B operand is
// formed on the fly from register-resident adjacency entries; also the bare 1 x 1 conv and the split-K ranges),
// gcn_stage_dense_kernel (dense per-segment adjacency on 128-row tiles: aggregation on the matrix pipe), gcn_stage_kernel
// (general: any / dense / per-sample / per-frame adjacency, ELL tables in LDS, aggregation into an LDS operand tile) and
// gcn_reduce_kernel (sums the split-K ranges); the fourth, gcn_stage_dense2_kernel, lives in gcn_dense.hip.  GEMM core: mfma_core.h.
#include <type_traits>

#include "mfma_core.h"
#include "gcn_params.h"

// ------------------------------------------------------------------------------------------------
// GCN stage
// ------------------------------------------------------------------------------------------------

template <int MT, int NJ>
__global__ __launch_bounds__(NTHREADS, 2) void gcn_stage_kernel(const GcnParams p) {
    constexpr int NT = 16384 / MT;
    constexpr int WM = MT / 64;
    constexpr int TPC = NTHREADS / NT;   // threads per column in the aggregation pass (1 or 2)
    constexpr int KPT = KC / TPC;        // channels per thread there
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int V = p.V, R = p.R, EW = p.ell_w;
    float *Wl = smem;                          // [R][KC][MT]
    float *Xa = Wl + R * KC * MT;              // [R][KC][NT]   aggregated operand
    float *Bx = Xa + R * KC * NT;              // [KC][ldb]     raw x frames
    float *Lv = Bx + KC * p.ldb;               // [3][V][EW]    adjacency values
    int *Ls = reinterpret_cast<int *>(Lv + 3 * V * EW * (p.adj_per_frame ? p.lds_frames : 1));   // [3][V][EW] row indices

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int l31 = lane & 31, kh = lane >> 5;
    const unsigned wid = xcd_contiguous_id(blockIdx.x, gridDim.x);
    const int m0 = (int)(wid % p.mtiles) * MT, q0 = (int)((wid / p.mtiles) % p.qtiles) * NT;
    const int seg = (int)(wid / (p.mtiles * p.qtiles));
    const int Q = p.frames * V;
    const int qend = min(q0 + NT, Q);
    const int ta = div_magic(q0, p.vmagic), tb = div_magic(qend - 1, p.vmagic);
    const int span = (tb - ta + 1) * V;

    // adjacency -> LDS, once per workgroup: the fixed graph, this segment's attention matrices, or (per-frame
    // mode, continual A-GCN where every frame is another skeleton) the matrices of the frames this tile touches
    const int adj_n = 3 * V * EW;
    {
        const int nmat = p.adj_per_frame ? (tb - ta + 1) : 1;
        const int64_t first = p.adj_per_frame ? ((int64_t)seg * p.frames + ta) : (int64_t)seg;
        const float *gv = p.ell_val + first * p.adj_seg_stride;
        const int32_t *gs = p.ell_src;             // the index pattern is shared; only the values vary
        for (int e = tid; e < adj_n * nmat; e += NTHREADS) Lv[e] = gv[e];
        for (int e = tid; e < adj_n; e += NTHREADS) Ls[e] = gs[e];
    }
    // dense mode: every subset lists all V source joints in order (src[e] == e), as the A-GCN host code builds it
    const bool dense_all = p.dense;
    // aggregation-pass coordinates of this thread: one column, KPT channels
    const int aj = tid % NT, ak0 = (tid / NT) * KPT;
    const int aq = min(q0 + aj, Q - 1);
    const int at = div_magic(aq, p.vmagic);
    const int aw = aq - at * V;
    const int afb = (at - ta) * V;

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[a][b][g] = 0.f;

    const int offA = wm * 64 + l31;
    const int off0 = wn * 64 + l31, off1 = off0 + 32;
    const float *seg_base = p.x + (int64_t)seg * p.x_seg_stride;

    WStage<MT> ws;
    BStage<NJ> bs;
    const float *wbase = p.w + m0;
    ws.setup(R, p.CinPad, p.Mpad, tid);
    bs.setup(ta * V, span, Q, lane);
    ws.issue(wbase);
    bs.issue(seg_base, p.Cin, p.x_chan_stride, 0, wave);
    for (int c0 = 0; c0 < p.CinPad; c0 += KC) {
        __syncthreads();                           // previous chunk's MFMA reads of Wl / Xa are done
        ws.commit(Wl);
        bs.commit(Bx, p.ldb, wave);
        __syncthreads();
        if (c0 + KC < p.CinPad) {                  // prefetch the next chunk underneath aggregation + MFMA
            ws.issue(wbase + (size_t)(c0 + KC) * p.Mpad);
            bs.issue(seg_base, p.Cin, p.x_chan_stride, c0 + KC, wave);
        }
        // adjacency aggregation: Xa[r][kk][j] = sum_e val_r[e] * Bx[kk][frame(j) + src_r[e]]
        const float *bx = Bx + ak0 * p.ldb + afb;
        if (dense_all) {
            // dense adjacency (A-GCN): all three subsets share the index pattern src = e, so every x value is
            // loaded ONCE and feeds the three subsets' accumulators (11 LDS reads per 24 FMAs instead of 30)
            float s0[KPT], s1[KPT], s2[KPT];
#pragma unroll
            for (int kk = 0; kk < KPT; ++kk) s0[kk] = s1[kk] = s2[kk] = 0.f;
            const int fo = p.adj_per_frame ? (at - ta) * adj_n : 0;          // this column's frame matrix
            const int eb0 = fo + aw * EW, eb1 = fo + (V + aw) * EW, eb2 = fo + (2 * V + aw) * EW;
            int e = 0;
            if ((V & 1) == 0) {
                // even joint count (Kinetics V = 18): every row / adjacency column starts 8-byte aligned, so two source
                // joints are fetched per LDS instruction (the pass is LDS-issue bound: 3 + KPT reads per 3*KPT FMAs)
                typedef float f32x2 __attribute__((ext_vector_type(2)));
                for (; e < V; e += 2) {
                    const f32x2 v0 = *reinterpret_cast<const f32x2 *>(Lv + eb0 + e), v1 = *reinterpret_cast<const f32x2 *>(Lv + eb1 + e),
                                v2 = *reinterpret_cast<const f32x2 *>(Lv + eb2 + e);
#pragma unroll
                    for (int kk = 0; kk < KPT; ++kk) {
                        const f32x2 xv = *reinterpret_cast<const f32x2 *>(bx + kk * p.ldb + e);
                        s0[kk] = fmaf(v0[1], xv[1], fmaf(v0[0], xv[0], s0[kk]));
                        s1[kk] = fmaf(v1[1], xv[1], fmaf(v1[0], xv[0], s1[kk]));
                        s2[kk] = fmaf(v2[1], xv[1], fmaf(v2[0], xv[0], s2[kk]));
                    }
                }
            }
            for (; e < V; ++e) {
                const float v0 = Lv[eb0 + e], v1 = Lv[eb1 + e], v2 = Lv[eb2 + e];
#pragma unroll
                for (int kk = 0; kk < KPT; ++kk) {
                    const float xv = bx[kk * p.ldb + e];
                    s0[kk] = fmaf(v0, xv, s0[kk]);
                    s1[kk] = fmaf(v1, xv, s1[kk]);
                    s2[kk] = fmaf(v2, xv, s2[kk]);
                }
            }
#pragma unroll
            for (int kk = 0; kk < KPT; ++kk) {
                Xa[(0 * KC + ak0 + kk) * NT + aj] = s0[kk];
                Xa[(1 * KC + ak0 + kk) * NT + aj] = s1[kk];
                Xa[(2 * KC + ak0 + kk) * NT + aj] = s2[kk];
            }
        } else {
            for (int r = 0; r < 3; ++r) {
                float s[KPT];
#pragma unroll
                for (int kk = 0; kk < KPT; ++kk) s[kk] = 0.f;
                const int cnt = p.ell_cnt[r];
                const int eb = (r * V + aw) * EW;
                for (int e = 0; e < cnt; ++e) {
                    const int src = Ls[eb + e];
                    const float val = Lv[eb + e];
#pragma unroll
                    for (int kk = 0; kk < KPT; ++kk) s[kk] = fmaf(val, bx[kk * p.ldb + src], s[kk]);
                }
#pragma unroll
                for (int kk = 0; kk < KPT; ++kk) Xa[(r * KC + ak0 + kk) * NT + aj] = s[kk];
            }
        }
        if (R == 4) {   // conv gcn_residual rides the same GEMM as a 4th "subset" with identity adjacency
#pragma unroll
            for (int kk = 0; kk < KPT; ++kk) Xa[(3 * KC + ak0 + kk) * NT + aj] = bx[kk * p.ldb + aw];
        }
        __syncthreads();
        mfma_chunk<MT>(Wl, Xa, R, NT, KC * NT, offA, off0, off1, kh, acc);
    }

    // epilogue: ReLU(acc + bias + identity residual), same scheme as the sparse kernel below (scalar row bases +
    // 32-bit lane offsets on full tiles, permlane32_swap for 256-B row segments)
    float *oseg = p.y + (int64_t)seg * p.y_seg_stride;
    const bool ident = p.res_mode == CSK_RES_IDENTITY;
    const int rbase = m0 + wm * 64;
    const bool full = p.fast_epi && m0 + MT <= p.Cout;
    const unsigned kh4 = 4u * (unsigned)kh;
    float bb[2][16], rv[2][2][16];
    if (full) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int g = 0; g < 16; ++g) bb[mi][g] = ld_lane(p.bias + (rbase + mi * 32 + (g & 3) + 8 * (g >> 2)), kh4 * 4u);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const unsigned lo = 4u * (kh4 * (unsigned)p.x_chan_stride + (unsigned)min(q0 + wn * 64 + ni * 32 + l31, Q - 1));
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const float *rrow = seg_base + (int64_t)(rbase + mi * 32 + (g & 3) + 8 * (g >> 2)) * p.x_chan_stride;
                    rv[ni][mi][g] = ident ? ld_lane(rrow, lo) : 0.f;
                }
        }
    } else {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int g = 0; g < 16; ++g) bb[mi][g] = p.bias[rbase + mi * 32 + 4 * kh + (g & 3) + 8 * (g >> 2)];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int qc = min(q0 + wn * 64 + ni * 32 + l31, Q - 1);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int co = rbase + mi * 32 + 4 * kh + (g & 3) + 8 * (g >> 2);
                    rv[ni][mi][g] = ident ? seg_base[(int64_t)min(co, p.Cout - 1) * p.x_chan_stride + qc] : 0.f;
                }
        }
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const float v0 = relu_nan(acc[mi][0][g] + bb[mi][g] + rv[0][mi][g]);
            const float v1 = relu_nan(acc[mi][1][g] + bb[mi][g] + rv[1][mi][g]);
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(v0), __float_as_uint(v1), false, false);
            acc[mi][0][g] = __uint_as_float(sw[0]);
            acc[mi][1][g] = __uint_as_float(sw[1]);
        }
    const int qb = q0 + wn * 64 + lane;
    const bool qv = qb < Q;
    if (full) {
        if (qv) {
            const unsigned qo = 4u * (unsigned)qb;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    float *orow = oseg + (int64_t)(rbase + mi * 32 + (g & 3) + 8 * (g >> 2)) * p.y_chan_stride;
                    st_lane(orow, qo, acc[mi][0][g]);
                    st_lane(orow + 4 * p.y_chan_stride, qo, acc[mi][1][g]);
                }
        }
    } else {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row0 = rbase + mi * 32 + (g & 3) + 8 * (g >> 2);
                if (qv && row0 < p.Cout) oseg[(int64_t)row0 * p.y_chan_stride + qb] = acc[mi][0][g];
                if (qv && row0 + 4 < p.Cout) oseg[(int64_t)(row0 + 4) * p.y_chan_stride + qb] = acc[mi][1][g];
            }
    }
}

// ------------------------------------------------------------------------------------------------
// GCN stage, sparse-graph fast path: the aggregated B operand is formed ON THE FLY in the MFMA loop.
// For skeleton graphs A_eff has <= 1 / 1 / 4 non-zeros per column in the self / inward / outward subsets (NTU-25:
// 1/1/4, OpenPose-18: 1/1/3), so every lane keeps the <= 6 (LDS offset, weight) pairs of its two output columns in
// registers and builds   B_r[c][q] = sum_e val * x[c][frame(q), src_e]   with <= 6 LDS reads + FMAs per k-step, against
// 12-16 MFMAs (768-1024 cycles) that consume them: no aggregated tile, no aggregation phase.  Dense / per-sample
// adjacencies (A-GCN) use the general kernel above.  Chunk pipeline (history: profiles/HISTORY.md, round 2 item 14):
//   * PING-PONG LDS: chunk c+1 is committed (registers -> LDS[other]) at the START of iteration c, in front of chunk c's
//     MFMAs, so one barrier per chunk suffices (everybody done reading LDS[cur] and writing LDS[other]);
//   * TRICKLED loads: the loads of chunk c+2 are issued a few at a time between the first MFMA k-steps of chunk c
//     (register prefetch one chunk ahead of the commit), pinned there with sched_barrier;
//   * the epilogue operands (32 biases + 64 residual values per lane) are loaded after the K loop, one 32-row half at
//     a time: with 8-channel chunks the kernel fits 168 registers and <= 45 KB of LDS, i.e. THREE workgroups per CU --
//     a GCN k-step carries 18 LDS reads + 14 VALU per 12 MFMAs whose latency a third wave per SIMD covers.
// KCG_ = channels per chunk.
// ------------------------------------------------------------------------------------------------
// PLAIN: the same pipeline as a bare 1 x 1 conv (one "subset" with the identity adjacency, no residual, no ReLU) -- the six
// a_i / b_i embedding convs of A-GCN fused into one GEMM (models/a_gcn/a_gcn.py:53-59), csk_conv1x1_f32.
// SPLIT: one of p.ksplit channel ranges of a tile (raw partial sums, no epilogue arithmetic): csk_gcn_stage_splitk_f32.
template <int MT, bool CONVRES, int KCG_, bool PLAIN = false, bool SPLIT = false>
__global__ __launch_bounds__(NTHREADS, 3) void gcn_stage_sparse2_kernel(const GcnParams p) {
    constexpr int NT = 16384 / MT;
    constexpr int WM = MT / 64;
    constexpr int R = PLAIN ? 1 : (CONVRES ? 4 : 3);
    constexpr int M4 = MT / 4;
    constexpr int WB = (R * KCG_ * M4 + NTHREADS - 1) / NTHREADS;   // f32x4 of weights per thread per chunk
    constexpr int RPW = KCG_ / (NTHREADS / 64);            // activation rows per wave per chunk
    constexpr int NJ = MT == 128 ? 3 : 5;                  // 64-lane sweeps per activation row (span <= 192 / 320)
    constexpr int NS = KCG_ / 2;                           // MFMA k-steps per chunk
    constexpr int NH = NS / 2;                             // ... of which the first NH carry the next-next chunk's loads
    static_assert(KCG_ % 8 == 0, "a chunk is a whole number of rows per wave");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int V = p.V;
    const int wsz = R * KCG_ * MT, bsz = KCG_ * p.ldb, bufsz = wsz + bsz;     // one chunk buffer: Wl [R][KCG][MT], Bx [KCG][ldb]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int l31 = lane & 31, kh = lane >> 5;
    const unsigned wid = xcd_contiguous_id(blockIdx.x, gridDim.x);
    const int m0 = (int)(wid % p.mtiles) * MT, q0 = (int)((wid / p.mtiles) % p.qtiles) * NT;
    const int segks = (int)(wid / (p.mtiles * p.qtiles));
    const int seg = SPLIT ? segks / p.ksplit : segks, ks = SPLIT ? segks % p.ksplit : 0;
    const int cb = SPLIT ? ks * p.cper : 0;                // first channel of this split
    const int Q = p.frames * V;
    const int qend = min(q0 + NT, Q);
    const int ta = div_magic(q0, p.vmagic), tb = div_magic(qend - 1, p.vmagic);
    const int span = (tb - ta + 1) * V;
    // per-lane adjacency entries of the two output columns this lane feeds (B operand: column = lane & 31)
    int eoff[2][6];
    float eval[2][6];
    int ioff[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int q = min(q0 + wn * 64 + ni * 32 + l31, Q - 1);
        const int t = div_magic(q, p.vmagic);
        const int w = q - t * V, fb = (t - ta) * V;
        ioff[ni] = fb + w;
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            const int r = e < 2 ? e : 2, k = e < 2 ? 0 : e - 2;          // subsets 0,1: one entry; subset 2: four
            const bool have = !PLAIN && k < p.ell_cnt[r];
            const int idx = PLAIN ? 0 : (r * V + w) * p.ell_w + min(k, p.ell_w - 1);
            eoff[ni][e] = fb + (have ? p.ell_src[idx] : 0);
            eval[ni][e] = have ? p.ell_val[idx] : 0.f;
        }
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[a][b][g] = 0.f;

    const float *seg_base = p.x + (int64_t)seg * p.x_seg_stride;
    const float *wbase = p.w + m0 + (size_t)cb * p.Mpad;
    // staging registers + chunk-invariant offsets
    f32x4 wv[WB];
    unsigned wgo[WB], wlo[WB];
#pragma unroll
    for (int u = 0; u < WB; ++u) {
        const int e = min(u * NTHREADS + tid, R * KCG_ * M4 - 1);   // surplus threads re-stage the last vector
        const int row = e / M4, m4 = e % M4;
        wgo[u] = (unsigned)(((row / KCG_) * p.CinPad + (row % KCG_)) * p.Mpad + m4 * 4);
        wlo[u] = (unsigned)(e * 4);
    }
    // Activation staging, two forms chosen per workgroup (uniform): element-wise (NJ sweeps of 64 lanes per row), or --
    // when the row holds 4*ceil(span/4) positions from the tile's first frame on (every tile but the last of a
    // segment) -- 16-byte loads (4-byte aligned in global memory, aligned in LDS) and ds_write_b128: a quarter of the
    // load and LDS-write instructions.
    constexpr int NJ4 = (NJ + 3) / 4;
    float bv[RPW][NJ];
    f32x4 bv4[RPW][NJ4];
    unsigned bgo[NJ], blo[NJ];
#pragma unroll
    for (int u = 0; u < NJ; ++u) {
        const int j = min(u * 64 + lane, span - 1);
        bgo[u] = (unsigned)(ta * V + j);                   // always inside [0, Q): whole frames of this segment
        blo[u] = (unsigned)j;
    }
    const int nvec = (span + 3) / 4;
    const bool vec = ta * V + 4 * nvec <= Q && p.Cin >= KCG_;     // uniform (a 3-channel input: nothing to gain)
    unsigned bgo4[NJ4], blo4[NJ4];
#pragma unroll
    for (int u = 0; u < NJ4; ++u) {
        const int i = min(u * 64 + lane, nvec - 1);
        bgo4[u] = (unsigned)(ta * V + 4 * i);
        blo4[u] = (unsigned)(4 * i);
    }
    // staging load i of chunk c0 (i is a literal after unrolling): 0..WB-1 weights, then activation (row, sweep) pairs.
    // channels >= Cin: the row is CLAMPED, not zeroed -- the packed weights of padding channels are zero, so a finite
    // duplicate contributes nothing (and a NaN / Inf duplicate only reaches outputs the real row already poisons); a
    // select here would make the compiler wait for the load right behind its issue
    auto issue_one = [&](auto vtag, int i, int c0) {
        constexpr bool VEC = decltype(vtag)::value;
        constexpr int NX = VEC ? NJ4 : NJ;
        if (i < WB) {
            wv[i] = *reinterpret_cast<const f32x4 *>(wbase + (size_t)c0 * p.Mpad + wgo[i]);
        } else {
            const int rr = (i - WB) / NX, u = (i - WB) % NX;
            const int c = min(cb + c0 + wave + rr * (NTHREADS / 64), p.Cin - 1);
            const float *row = seg_base + (int64_t)c * p.x_chan_stride;
            if (VEC) bv4[rr][u] = *reinterpret_cast<const f32x4u *>(row + bgo4[u]);
            else bv[rr][u] = row[bgo[u]];
        }
    };
    auto commit = [&](auto vtag, float *buf) {
        constexpr bool VEC = decltype(vtag)::value;
        float *Wl = buf, *Bx = buf + wsz;
#pragma unroll
        for (int u = 0; u < WB; ++u) *reinterpret_cast<f32x4 *>(Wl + wlo[u]) = wv[u];
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            float *dst = Bx + (wave + rr * (NTHREADS / 64)) * p.ldb;
            if (VEC) {
#pragma unroll
                for (int u = 0; u < NJ4; ++u) *reinterpret_cast<f32x4 *>(dst + blo4[u]) = bv4[rr][u];
            } else {
#pragma unroll
                for (int u = 0; u < NJ; ++u) dst[blo[u]] = bv[rr][u];
            }
        }
    };
    const int offA = wm * 64 + l31;
    // one MFMA k-step pair of the chunk in `buf`: the aggregated B operand is formed on the fly (see the first form)
    auto mfma_step = [&](const float *buf, int s) {
        const float *Wl = buf, *Bx = buf + wsz;
        const int kk = 2 * s + kh;
        const float *bx = Bx + kk * p.ldb;
        float b[R][2];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            if constexpr (PLAIN) {
                b[0][ni] = bx[ioff[ni]];
            } else {
                const float x0 = bx[eoff[ni][0]];
                b[0][ni] = eval[ni][0] * x0;
                b[1][ni] = eval[ni][1] * bx[eoff[ni][1]];
                float s2 = eval[ni][2] * bx[eoff[ni][2]];
                s2 = fmaf(eval[ni][3], bx[eoff[ni][3]], s2);
                s2 = fmaf(eval[ni][4], bx[eoff[ni][4]], s2);
                s2 = fmaf(eval[ni][5], bx[eoff[ni][5]], s2);
                b[2][ni] = s2;
                if (CONVRES) b[R - 1][ni] = bx[ioff[ni]];
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float *wr = Wl + (r * KCG_ + kk) * MT + offA;
            const float a0 = wr[0], a1 = wr[32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b[r][0], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b[r][1], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b[r][0], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b[r][1], acc[1][1], 0, 0, 0);
        }
    };

    // CinPad is a multiple of CSK_CPAD = 16; a split covers cper (a multiple of KCG_) channels, the last one what is left
    const int nchunks = (SPLIT ? min(p.CinPad - cb, p.cper) : p.CinPad) / KCG_;
    auto k_loop = [&](auto vtag) {
        constexpr int NLX = WB + RPW * (decltype(vtag)::value ? NJ4 : NJ);     // staging loads per thread per chunk
#pragma unroll
        for (int i = 0; i < NLX; ++i) issue_one(vtag, i, 0);
        commit(vtag, smem);
        if (nchunks > 1) {
#pragma unroll
            for (int i = 0; i < NLX; ++i) issue_one(vtag, i, KCG_);
        }
        __syncthreads();
        for (int c = 0; c + 1 < nchunks; ++c) {
            float *cur = smem + (c & 1) * bufsz, *oth = smem + ((c & 1) ^ 1) * bufsz;
            commit(vtag, oth);                                 // chunk c+1: registers -> the other buffer
            // chunk c+2's loads; past the end the last chunk is re-loaded into the (then dead) staging registers, so that
            // the k-step sequence below stays ONE basic block (a uniform branch per load group would confine the
            // scheduler's LDS-read / MFMA interleave to single k-steps)
            const int cnext = min(c + 2, nchunks - 1) * KCG_;
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                // all loads go out in the FIRST half of the k-steps: the second half (and the barrier) is their latency
                // cover before the commit at the top of the next iteration
                if (s < NH) {
#pragma unroll
                    for (int i = s * NLX / NH; i < (s + 1) * NLX / NH; ++i) issue_one(vtag, i, cnext);
                    // pin the loads to this k-step: left alone, the machine scheduler sinks all of them to the end of the
                    // block, right in front of the barrier and the commit that needs them (a mask that only holds back
                    // vector-memory instructions does not help: the MFMAs are then hoisted over the loads instead)
                    __builtin_amdgcn_sched_barrier(0);
                }
                mfma_step(cur, s);
            }
            __builtin_amdgcn_s_setprio(0);
            __syncthreads();
        }
    };
    if (vec) k_loop(std::true_type{});
    else k_loop(std::false_type{});
    const float *last = smem + ((nchunks - 1) & 1) * bufsz;
    // Epilogue operands: loaded after the K loop, one 32-row half at a time (register budget of three workgroups / CU)
    const int rbase = m0 + wm * 64;
    const bool full = p.fast_epi && m0 + MT <= p.Cout;
    const unsigned kh4 = 4u * (unsigned)kh;
    float *oseg = SPLIT ? p.part + (int64_t)(seg * p.ksplit + ks) * p.Cout * p.y_chan_stride : p.y + (int64_t)seg * p.y_seg_stride;
    const int qb = q0 + wn * 64 + lane;
    const bool qv = qb < Q;
    float bb[2][16], rv[2][2][16];
    auto load_half = [&](int mi) {
        if (SPLIT) {                        // raw partial sums: bias, residual and ReLU belong to gcn_reduce_kernel
#pragma unroll
            for (int g = 0; g < 16; ++g) bb[mi][g] = rv[0][mi][g] = rv[1][mi][g] = 0.f;
        } else if (full) {
#pragma unroll
            for (int g = 0; g < 16; ++g) bb[mi][g] = ld_lane(p.bias + (rbase + mi * 32 + (g & 3) + 8 * (g >> 2)), kh4 * 4u);
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const unsigned lo = 4u * (kh4 * (unsigned)p.x_chan_stride + (unsigned)min(q0 + wn * 64 + ni * 32 + l31, Q - 1));
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const float *rrow = seg_base + (int64_t)(rbase + mi * 32 + (g & 3) + 8 * (g >> 2)) * p.x_chan_stride;
                    rv[ni][mi][g] = (CONVRES || PLAIN) ? 0.f : ld_lane(rrow, lo);
                }
            }
        } else {
#pragma unroll
            for (int g = 0; g < 16; ++g) bb[mi][g] = p.bias[rbase + mi * 32 + 4 * kh + (g & 3) + 8 * (g >> 2)];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int qc = min(q0 + wn * 64 + ni * 32 + l31, Q - 1);
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int co = rbase + mi * 32 + 4 * kh + (g & 3) + 8 * (g >> 2);
                    rv[ni][mi][g] = (CONVRES || PLAIN) ? 0.f : seg_base[(int64_t)min(co, p.Cout - 1) * p.x_chan_stride + qc];
                }
            }
        }
    };
    // ReLU(acc + bias + identity residual); permlane32_swap pairs the ni = 0/1 registers so that every store
    // instruction writes one 256-B contiguous row segment (see tcn_stage_kernel)
    auto finish_half = [&](int mi) {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            float v0 = acc[mi][0][g] + bb[mi][g] + rv[0][mi][g];
            float v1 = acc[mi][1][g] + bb[mi][g] + rv[1][mi][g];
            if (!PLAIN && !SPLIT) { v0 = relu_nan(v0); v1 = relu_nan(v1); }
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(v0), __float_as_uint(v1), false, false);
            acc[mi][0][g] = __uint_as_float(sw[0]);       // row (g & 3) + 8*(g >> 2), column qb
            acc[mi][1][g] = __uint_as_float(sw[1]);       // row + 4
        }
        if (full) {
            if (qv) {
                const unsigned qo = 4u * (unsigned)qb;
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    float *orow = oseg + (int64_t)(rbase + mi * 32 + (g & 3) + 8 * (g >> 2)) * p.y_chan_stride;
                    st_lane(orow, qo, acc[mi][0][g]);
                    st_lane(orow + 4 * p.y_chan_stride, qo, acc[mi][1][g]);
                }
            }
        } else {
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row0 = rbase + mi * 32 + (g & 3) + 8 * (g >> 2);
                if (qv && row0 < p.Cout) oseg[(int64_t)row0 * p.y_chan_stride + qb] = acc[mi][0][g];
                if (qv && row0 + 4 < p.Cout) oseg[(int64_t)(row0 + 4) * p.y_chan_stride + qb] = acc[mi][1][g];
            }
        }
    };
#pragma unroll
    for (int s = 0; s < NS; ++s) mfma_step(last, s);
    load_half(0);
    finish_half(0);
    load_half(1);
    finish_half(1);
}

// ------------------------------------------------------------------------------------------------
// GCN stage for a DENSE PER-SEGMENT adjacency (A-GCN clip form, models/a_gcn/a_gcn.py:62-65): the V x V aggregation itself
// runs on the matrix pipe.  Per chunk of KC2 channels the aggregation of a tile is the small GEMM
//     Xa[(frame, channel), (subset, w)] = sum_v  x[channel][frame, v] * adj[subset][v, w]
// with rows = (frames of the tile) x KC2 channels, columns = 3 V (two or three 32-column blocks), K = V: every (row block,
// column block) unit is one 32 x 32 accumulator and ceil(V / 2) v_mfma_f32_32x32x2_f32, the units are dealt to the four
// waves, and the results go to the LDS operand tile Xa of the channel-mixing GEMM.  Against the VALU form of
// gcn_stage_kernel (3 + KPT LDS reads per 3 KPT FMAs: LDS-issue bound, 1.6 x the sparse kernel's time) this costs
// +19 % MFMA cycles at V = 18 and frees the vector unit.  Tiles are FRAME-ALIGNED (FT = NT / V whole frames per tile: 126
// of 128 columns at V = 18) so that every tile has the same row blocks and the x tile starts at the tile's first position.
// Exact fp32 as everything else (the MFMA is an fmaf chain in k order); only the summation order over v differs from
// gcn_stage_kernel's (v = 0, 1, 2, ... there as here, but in chunks of two per instruction: the same order).
// ------------------------------------------------------------------------------------------------
template <int MT, bool CONVRES, int KC2, int OCC>
__global__ __launch_bounds__(NTHREADS, OCC) void gcn_stage_dense_kernel(const GcnParams p) {
    constexpr int NT = 16384 / MT;
    constexpr int WM = MT / 64;                          // KC2 = channels per chunk, OCC = workgroups per CU
    constexpr int R = CONVRES ? 4 : 3;
    constexpr int M4 = MT / 4;
    constexpr int WBU = (R * KC2 * M4 + NTHREADS - 1) / NTHREADS;   // f32x4 of weights per thread and chunk (surplus threads re-stage the last)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int V = p.V, FT = p.lds_frames, ldbx = p.ldb;  // frames per tile, padded x row length
    float *Wl = smem;                                    // [R][KC2][MT]
    float *Xa = Wl + R * KC2 * MT;                       // [3][KC2][NT]
    float *Bx = Xa + 3 * KC2 * NT;                       // [KC2][ldbx]
    float *Ladj = Bx + KC2 * ldbx;                       // [3 V][V]   adj[r][v, w] at (r V + w) V + v

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int l31 = lane & 31, kh = lane >> 5;
    const unsigned wid = xcd_contiguous_id(blockIdx.x, gridDim.x);
    const int m0 = (int)(wid % p.mtiles) * MT, qt = (int)((wid / p.mtiles) % p.qtiles);
    const int seg = (int)(wid / (p.mtiles * p.qtiles));
    const int Q = p.frames * V;
    const int ta = qt * FT, q0 = ta * V;
    const int fcnt = min(FT, p.frames - ta);             // frames of this tile
    const int ncol = fcnt * V;                           // valid columns of this tile

    {   // this segment's adjacency -> LDS (dense column-wise values, include/cskel.h)
        const float *gv = p.ell_val + (int64_t)seg * p.adj_seg_stride;
        for (int e = tid; e < 3 * V * V; e += NTHREADS) Ladj[e] = gv[e];
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[a][b][g] = 0.f;

    const float *seg_base = p.x + (int64_t)seg * p.x_seg_stride;
    const float *wbase = p.w + m0;
    // staging: weights [R][KC2][MT] as 16-byte vectors; x rows as 4-byte-aligned 16-byte vectors, each clamped into its row
    // (a clamped vector lands at its own -- clamped -- LDS offset, so a partial last vector overlaps its neighbour with
    // the same values instead of shifting data)
    f32x4 wv[WBU];
    constexpr int XV = 2;                                // x vectors per thread and chunk: KC2 rows x <= 256 / 4 ... 
    const int xrow = tid / 32, xv0 = tid % 32;           // 8 rows x 32 vectors per sweep of 256 threads
    f32x4 xv[XV][2];
    auto issue = [&](int c0) {
#pragma unroll
        for (int u = 0; u < WBU; ++u) {
            const int e = min(u * NTHREADS + tid, R * KC2 * M4 - 1);
            const int row = e / M4, m4 = e % M4;
            wv[u] = *reinterpret_cast<const f32x4 *>(wbase + (size_t)((row / KC2) * p.CinPad + c0 + (row % KC2)) * p.Mpad + m4 * 4);
        }
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int kk = xrow + 8 * u;
            if (kk < KC2) {
                const float *src = seg_base + (int64_t)min(c0 + kk, p.Cin - 1) * p.x_chan_stride;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int o = min(4 * (xv0 + 32 * h), max(ncol - 4, 0));
                    xv[u][h] = *reinterpret_cast<const f32x4u *>(src + min(q0 + o, Q - 4));
                }
            }
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int u = 0; u < WBU; ++u) *reinterpret_cast<f32x4 *>(Wl + 4 * min(u * NTHREADS + tid, R * KC2 * M4 - 1)) = wv[u];
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int kk = xrow + 8 * u;
            if (kk < KC2) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int o = min(4 * (xv0 + 32 * h), max(ncol - 4, 0));
                    const int oo = min(q0 + o, Q - 4) - q0;                  // (a tile shorter than 4 positions: Q - 4 < q0 never
                    *reinterpret_cast<f32x4u *>(Bx + kk * ldbx + max(oo, 0)) = xv[u][h];   //  happens for V >= 4 frames)
                }
            }
        }
    };
    // aggregation units of this wave
    const int RT = (fcnt * KC2 + 31) / 32, CT = (3 * V + 31) / 32, KS2 = (V + 1) / 2;
    const int offA = wm * 64 + l31;
    const int off0 = wn * 64 + l31, off1 = off0 + 32;

    issue(0);
    for (int c0 = 0; c0 < p.CinPad; c0 += KC2) {
        __syncthreads();                               // previous chunk's reads of Wl / Xa / Bx are done
        commit();
        __syncthreads();
        if (c0 + KC2 < p.CinPad) issue(c0 + KC2);
        // ---- aggregation on the matrix pipe: unit u = (row block, column block)
        for (int u = wave; u < RT * CT; u += NTHREADS / 64) {
            const int rt = u / CT, ct = u - rt * CT;
            const int row = rt * 32 + l31, col = ct * 32 + l31;          // A operand: row, B operand: column of this lane
            const int tl = row / KC2, kk = row % KC2;
            const bool rok = tl < fcnt, cok = col < 3 * V;
            const float *ax = Bx + kk * ldbx + min(tl, fcnt - 1) * V;
            const float *bj = Ladj + min(col, 3 * V - 1) * V;
            f32x16 d;
#pragma unroll
            for (int g = 0; g < 16; ++g) d[g] = 0.f;
            // operands of four k-steps are fetched together, then their MFMAs issue back to back (a rolled one-step loop
            // exposes the LDS latency of every step: the chain has a single accumulator)
            for (int s2 = 0; s2 < KS2; s2 += 4) {
                float a[4], b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int v = 2 * (s2 + j) + kh;
                    const bool vok = v < V;
                    const float av = ax[min(v, V - 1)], bv = bj[min(v, V - 1)];
                    a[j] = (rok && vok) ? av : 0.f;
                    b[j] = (cok && vok) ? bv : 0.f;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) d = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], d, 0, 0, 0);
            }
            // D[row][col]: col = this lane, rows (g & 3) + 8 (g >> 2) + 4 kh -> Xa[subset][channel][frame V + w]
            const int r = col / V, w = col - r * V;
            if (cok) {
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int ro = rt * 32 + (g & 3) + 8 * (g >> 2) + 4 * kh;
                    const int tlo = ro / KC2, kko = ro % KC2;
                    if (tlo < fcnt) Xa[(r * KC2 + kko) * NT + tlo * V + w] = d[g];
                }
            }
        }
        __syncthreads();
        // ---- channel mixing: acc += W[r][kk][rows] x Xa[r][kk][cols]  (+ conv gcn_residual: 4th subset straight from x)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float *wr = Wl + (r * KC2 + kh) * MT + offA;
            const float *br = (CONVRES && r == 3) ? Bx + kh * ldbx : Xa + (r * KC2 + kh) * NT;
            const int ldr = (CONVRES && r == 3) ? ldbx : NT;
#pragma unroll
            for (int s = 0; s < KC2 / 2; ++s) {
                const float a0 = wr[2 * s * MT], a1 = wr[2 * s * MT + 32];
                const float b0 = br[2 * s * ldr + off0], b1 = br[2 * s * ldr + off1];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }

    // epilogue: ReLU(acc + bias + identity residual), scheme of gcn_stage_kernel; columns beyond the tile's frames are dropped
    float *oseg = p.y + (int64_t)seg * p.y_seg_stride;
    const bool ident = p.res_mode == CSK_RES_IDENTITY;
    const int rbase = m0 + wm * 64;
    const bool full = p.fast_epi && m0 + MT <= p.Cout;
    const unsigned kh4 = 4u * (unsigned)kh;
    const int jb = wn * 64 + lane, qb = q0 + jb;
    const bool qv = jb < ncol;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        float bb[16], rv[2][16];
        if (full) {
#pragma unroll
            for (int g = 0; g < 16; ++g) bb[g] = ld_lane(p.bias + (rbase + mi * 32 + (g & 3) + 8 * (g >> 2)), kh4 * 4u);
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const unsigned lo = 4u * (kh4 * (unsigned)p.x_chan_stride + (unsigned)min(q0 + wn * 64 + ni * 32 + l31, Q - 1));
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const float *rrow = seg_base + (int64_t)(rbase + mi * 32 + (g & 3) + 8 * (g >> 2)) * p.x_chan_stride;
                    rv[ni][g] = ident ? ld_lane(rrow, lo) : 0.f;
                }
            }
        } else {
#pragma unroll
            for (int g = 0; g < 16; ++g) bb[g] = p.bias[rbase + mi * 32 + 4 * kh + (g & 3) + 8 * (g >> 2)];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int qc = min(q0 + wn * 64 + ni * 32 + l31, Q - 1);
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int co = rbase + mi * 32 + 4 * kh + (g & 3) + 8 * (g >> 2);
                    rv[ni][g] = ident ? seg_base[(int64_t)min(co, p.Cout - 1) * p.x_chan_stride + qc] : 0.f;
                }
            }
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const float v0 = relu_nan(acc[mi][0][g] + bb[g] + rv[0][g]);
            const float v1 = relu_nan(acc[mi][1][g] + bb[g] + rv[1][g]);
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(v0), __float_as_uint(v1), false, false);
            acc[mi][0][g] = __uint_as_float(sw[0]);
            acc[mi][1][g] = __uint_as_float(sw[1]);
        }
        if (full) {
            if (qv) {
                const unsigned qo = 4u * (unsigned)qb;
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    float *orow = oseg + (int64_t)(rbase + mi * 32 + (g & 3) + 8 * (g >> 2)) * p.y_chan_stride;
                    st_lane(orow, qo, acc[mi][0][g]);
                    st_lane(orow + 4 * p.y_chan_stride, qo, acc[mi][1][g]);
                }
            }
        } else {
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row0 = rbase + mi * 32 + (g & 3) + 8 * (g >> 2);
                if (qv && row0 < p.Cout) oseg[(int64_t)row0 * p.y_chan_stride + qb] = acc[mi][0][g];
                if (qv && row0 + 4 < p.Cout) oseg[(int64_t)(row0 + 4) * p.y_chan_stride + qb] = acc[mi][1][g];
            }
        }
    }
}

// split-K reduction of the GCN stage: y[seg][co][q] = ReLU( sum_ks part[seg * ksplit + ks][co][q] (split order) + bias[co]
// + identity gcn_residual x[seg][co][q] ); one thread per (co, q), q < Q = frames * V
__global__ __launch_bounds__(256) void gcn_reduce_kernel(const GcnParams p) {
    const int Q = p.frames * p.V;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)p.Cout * Q) return;
    const int co = (int)(i / Q), q = (int)(i - (int64_t)co * Q), seg = blockIdx.y;
    float s = 0.f;
    for (int ks = 0; ks < p.ksplit; ++ks) s += p.part[((int64_t)(seg * p.ksplit + ks) * p.Cout + co) * p.y_chan_stride + q];
    s += p.bias[co];
    if (p.res_mode == CSK_RES_IDENTITY) s += p.x[(int64_t)seg * p.x_seg_stride + (int64_t)co * p.x_chan_stride + q];
    p.y[(int64_t)seg * p.y_seg_stride + (int64_t)co * p.y_chan_stride + q] = relu_nan(s);
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// The workgroup tile of gcn_stage_kernel and gcn_stage_sparse2_kernel for p's shape: MT x NT outputs (128 rows where Mpad allows),
// activation rows of whole frames.  Fills p.ldb / p.lds_frames / p.qtiles / p.mtiles.  The two guards of that arithmetic speak
// under the caller's name; a caller runs each at its own place among its checks (gcn_stage_setup, csk_conv1x1_f32).
struct GcnTile {
    int MT, NT;
    explicit GcnTile(GcnParams &p) : MT((p.Mpad % 128) == 0 ? 128 : 64), NT(16384 / MT) {
        const int max_dt = (NT + p.V - 2) / p.V;
        p.lds_frames = max_dt + 1;
        p.ldb = round_up(p.lds_frames * p.V, 4);
        p.qtiles = (unsigned)(((int64_t)p.frames * p.V + NT - 1) / NT); p.mtiles = p.Mpad / MT;
    }
    static int positions_guard(const GcnParams &p, const char *who) {
        if ((int64_t)p.frames * p.V >= (1 << 26)) CSK_FAIL("%s: frames*V too large for 32-bit position arithmetic", who);
        return 0;
    }
    static int grid_guard(const GcnParams &p, int n_seg, const char *who) {
        if ((int64_t)p.qtiles * p.mtiles * n_seg >= (1ll << 31)) CSK_FAIL("%s: grid too large", who);
        return 0;
    }
};

// What every launch of the stage starts from: the argument checks that need no operand (0, or -1 with the message set), the launch
// parameters with the geometry of the 32x32x2 tiles, *lds_out = the general kernel's LDS tile, *sparse_out = the skeleton-sparse
// fast path applies.  No pointer but ell_cnt is dereferenced: csk_gcn_stage_f32_tile calls it without operands.
static int gcn_stage_setup(const GcnCall &c, GcnParams *out, int *MT_out, size_t *lds_out, bool *sparse_out) {
    const int V = c.V, ell_w = c.ell_w;
    const int32_t *ell_cnt = c.ell_cnt;
    if (c.n_seg <= 0 || c.c_in <= 0 || c.c_out <= 0 || c.frames <= 0 || V < 2 || V > 64) CSK_FAIL("gcn_stage: bad dims");
    if (ell_w < 1 || ell_w > V) CSK_FAIL("gcn_stage: ell_w must be in [1, V]");
    if (c.res_mode != CSK_RES_IDENTITY && c.res_mode != CSK_RES_CONV) CSK_FAIL("gcn_stage: res_mode must be identity or conv");
    if (c.res_mode == CSK_RES_IDENTITY && c.c_in != c.c_out) CSK_FAIL("gcn_stage: identity residual needs c_in == c_out");
    for (int i = 0; i < 3; ++i)
        if (ell_cnt[i] < 0 || ell_cnt[i] > ell_w) CSK_FAIL("gcn_stage: ell_cnt[%d] out of range", i);
    GcnParams &p = *out;
    p = gcn_params(c);
    // per-segment adjacencies are dense by contract (include/cskel.h): ell_w == V, ell_cnt == {V,V,V}, src[e] == e
    p.dense = c.adj_seg_stride != 0 && ell_w == V && ell_cnt[0] == V && ell_cnt[1] == V && ell_cnt[2] == V;
    p.adj_per_frame = c.adj_per_frame != 0;
    if (p.adj_per_frame && !p.dense) CSK_FAIL("gcn_stage: per-frame adjacency must be dense (ell_w == V, ell_cnt == V)");
    const GcnTile tile(p);
    const bool big = tile.MT == 128;
    const size_t lds = (size_t)(p.R * KC * tile.MT + p.R * KC * tile.NT + KC * p.ldb + 3 * V * ell_w * (1 + (p.adj_per_frame ? p.lds_frames : 1))) * sizeof(float);
    if (lds > 160 * 1024) CSK_FAIL("gcn_stage: LDS tile %zu B exceeds 160 KiB", lds);
    if (const int rc = GcnTile::positions_guard(p, "gcn_stage")) return rc;
    if (const int rc = GcnTile::grid_guard(p, c.n_seg, "gcn_stage")) return rc;
    // sparse-graph fast path: shared adjacency with <= 1/1/4 non-zeros per column, activation tile <= 320 positions
    const bool sparse = c.adj_seg_stride == 0 && ell_cnt[0] <= 1 && ell_cnt[1] <= 1 && ell_cnt[2] <= 4 && p.ldb <= (big ? 192 : 320) &&
                        !csk_diag_flag("CSK_GCN_GENERAL");
    // split-K (latency mode)
    if (c.ksplit > 1 && !sparse) CSK_FAIL("gcn_stage_splitk: split-K is built for the skeleton-sparse kernel (shared adjacency, <= 1/1/4 non-zeros per column)");
    p.ksplit = split_ranges(p.CinPad, c.c_in, c.ksplit, 8, &p.cper);
    *MT_out = tile.MT; *lds_out = lds; *sparse_out = sparse;
    return 0;
}

// The ONE decision of a launch: the kernel it runs and what that launch takes beyond GcnParams.  gcn_stage_route fills it,
// gcn_stage_impl switches on it, gcn_route_code turns it into the integers the route queries report (include/cskel.h).
enum { ROUTE_SPARSE2 = 1, ROUTE_TILE16 = 2, ROUTE_DENSE2 = 3, ROUTE_DENSE128 = 4, ROUTE_GENERAL = 5 };
// the bit fields csk_gcn_stage_splitk_f32_route reports for a split launch
enum { ROUTE_SPLIT = 1 << 30, ROUTE_SPLIT_MT128 = 1 << 29, ROUTE_SPLIT_CONVRES = 1 << 28, ROUTE_SPLIT_RANGES_SHIFT = 23, ROUTE_SPLIT_CPER_MASK = (1 << 23) - 1 };
struct GcnRoute {
    int family;           // ROUTE_*
    int MT;               // rows of a workgroup tile, 128 or 64
    bool convres;         // conv gcn_residual: a fourth operand subset
    int NJ;               // ROUTE_GENERAL: gcn_stage_kernel<MT, NJ>
    int tile16;           // ROUTE_TILE16: csk_gcn16_tile's value (0 in every other family)
    int dense2;           // ROUTE_DENSE2: csk_gcn_dense2_route's value
    int ranges, cper;     // ROUTE_SPARSE2: channel ranges of cper channels; > 1 range = the split launch and its reduction
    // what the launch takes that is not in GcnParams (ROUTE_TILE16 / ROUTE_DENSE2: their launchers own it, nothing below is set)
    unsigned grid;
    size_t lds;
    int lds_frames, ldb;  // ROUTE_DENSE128: the frame-aligned tiles, in place of the fields gcn_stage_setup gave p
    unsigned qtiles;
};

// Sets up the launch parameters of a call (gcn_stage_setup) and decides its route: 0, or -1 with the message set where a check
// fails or no kernel takes the shape.  The one path of the two launch entries and the three queries.  Host arithmetic: of the
// operands only the alignment is read (csk_gcn16_tile, csk_gcn_dense2_route), each of those rules asked once.
static int gcn_stage_route(const GcnCall &c, GcnParams *out, GcnRoute *route) {
    GcnParams &p = *out;
    size_t lds;
    bool sparse;
    GcnRoute r = {};
    if (const int rc = gcn_stage_setup(c, &p, &r.MT, &lds, &sparse)) return rc;
    const bool big = r.MT == 128;
    const int NT = 16384 / r.MT, V = p.V, n_seg = c.n_seg;
    r.convres = p.R == 4;
    r.ranges = p.ksplit; r.cper = p.cper;
    r.grid = p.qtiles * p.mtiles * n_seg;
    if (p.ksplit > 1) {   // a split launch: gcn_stage_setup has refused everything but the sparse family
        if (p.cper / 8 > ROUTE_SPLIT_CPER_MASK) CSK_FAIL("gcn_stage_splitk: %d channels per range exceed the split launch", p.cper);
        if ((int64_t)r.grid * r.ranges >= (1ll << 31)) CSK_FAIL("gcn_stage: grid too large");
        r.family = ROUTE_SPARSE2;
        r.grid *= r.ranges;
    } else if (sparse && (r.tile16 = csk_gcn16_tile(p, n_seg)) != 0) {
        r.family = ROUTE_TILE16;   // slot-balanced 16x16x4 tiles where they pack the chip better (step16.hip; same sums)
    } else if (sparse) {
        r.family = ROUTE_SPARSE2;
    } else if (p.dense && (r.dense2 = csk_gcn_dense2_route(p, n_seg)) != 0) {
        // dense per-sample / per-frame adjacency at V = 18 / 25: on-the-fly aggregation from register-resident adjacency
        // columns (gcn_dense.hip); every other dense shape continues below
        r.family = ROUTE_DENSE2;
    } else if (big && p.dense && !p.adj_per_frame && V >= 4 && V <= 32 && NT / V >= 1 && p.frames * (int64_t)V >= 4) {
        // dense per-segment adjacency (A-GCN clip form): aggregation on the matrix pipe, frame-aligned tiles
        // (128-row tiles only: on the 64-row tiles of the C_out = 64 layers the VALU aggregation of the general kernel measured
        // 0.31 ms per launch against 0.34 ms for this form -- profiles/r03a_agcn_clip_layers.md vs r03b)
        r.family = ROUTE_DENSE128;
        r.lds_frames = NT / V;                                  // FT: whole frames per tile
        r.ldb = round_up(r.lds_frames * V, 4);
        if ((r.ldb / 4) % 2 == 0) r.ldb += 4;                   // row stride = 4 (mod 8) words: the row-block reads are at most 2-way conflicted
        r.qtiles = (p.frames + r.lds_frames - 1) / r.lds_frames;
        if ((int64_t)r.qtiles * p.mtiles * n_seg >= (1ll << 31)) CSK_FAIL("gcn_stage: grid too large");
        r.grid = r.qtiles * p.mtiles * n_seg;
        r.lds = (size_t)(p.R * 8 * r.MT + 3 * 8 * NT + 8 * r.ldb + 3 * V * V) * sizeof(float);
    } else {
        // activation staging sweeps per row: whole frames of the tile only (no temporal halo), i.e. < NT + 2 V positions:
        // <= 256 for 128-wide and <= 384 for 256-wide tiles at V <= 64 -- 3-4 / 5-6 sweeps of 64 lanes (all spill-free)
        const int nj = (p.ldb + 63) / 64;
        if (nj > (big ? 4 : 6)) CSK_FAIL("gcn_stage: activation tile of %d positions per channel exceeds the staged maximum", p.ldb);
        r.family = ROUTE_GENERAL;
        r.NJ = big ? (nj <= 3 ? 3 : 4) : (nj <= 5 ? 5 : 6);
        r.lds = lds;
    }
    // ping-pong LDS, trickled loads, 3 workgroups / CU
    if (r.family == ROUTE_SPARSE2) r.lds = 2 * (size_t)(p.R * 8 * r.MT + 8 * p.ldb) * sizeof(float);
    *route = r;
    return 0;
}

// What the queries report for a route (include/cskel.h): family * 1000000 + template arguments (csk_gcn_stage_f32_route), the bit
// fields of a split launch (csk_gcn_stage_splitk_f32_route).  Nothing in the library reads these integers back.
static int gcn_route_code(const GcnRoute &r) {
    if (r.ranges > 1)
        return ROUTE_SPLIT | (r.MT == 128 ? ROUTE_SPLIT_MT128 : 0) | (r.convres ? ROUTE_SPLIT_CONVRES : 0) | ((r.ranges - 1) << ROUTE_SPLIT_RANGES_SHIFT) |
               (r.cper / 8);
    const int args = r.family == ROUTE_TILE16 ? r.tile16 : r.family == ROUTE_DENSE2 ? r.dense2 : r.family == ROUTE_DENSE128 ? (int)r.convres :
                     r.MT * 10 + (r.family == ROUTE_GENERAL ? r.NJ : (int)r.convres);
    return r.family * 1000000 + args;
}

template <bool SPLIT>
static auto gcn_sparse2_kernel_of(const GcnRoute &r) -> void (*)(GcnParams) {
    if (r.MT == 128) return r.convres ? gcn_stage_sparse2_kernel<128, true, 8, false, SPLIT> : gcn_stage_sparse2_kernel<128, false, 8, false, SPLIT>;
    return r.convres ? gcn_stage_sparse2_kernel<64, true, 8, false, SPLIT> : gcn_stage_sparse2_kernel<64, false, 8, false, SPLIT>;
}

static int gcn_stage_impl(const GcnCall &c, void *stream) {
    if (!c.x || !c.y || !c.w || !c.bias || !c.ell_src || !c.ell_val || !c.ell_cnt) CSK_FAIL("gcn_stage: null pointer");
    GcnParams p;
    GcnRoute r;
    if (const int rc = gcn_stage_route(c, &p, &r)) return rc;
    hipStream_t s = (hipStream_t)stream;
    void (*kern)(GcnParams);
    switch (r.family) {
        case ROUTE_TILE16: return csk_launch_gcn16(p, c.n_seg, r.tile16, stream);
        case ROUTE_DENSE2: return csk_launch_gcn_dense2(p, c.n_seg, r.dense2, stream);
        case ROUTE_SPARSE2: kern = r.ranges > 1 ? gcn_sparse2_kernel_of<true>(r) : gcn_sparse2_kernel_of<false>(r); break;
        case ROUTE_DENSE128:
            p.lds_frames = r.lds_frames; p.ldb = r.ldb; p.qtiles = r.qtiles;
            kern = r.convres ? gcn_stage_dense_kernel<128, true, 8, 3> : gcn_stage_dense_kernel<128, false, 8, 3>;
            break;
        default:
            kern = r.MT == 128 ? (r.NJ == 3 ? gcn_stage_kernel<128, 3> : gcn_stage_kernel<128, 4>)
                               : (r.NJ == 5 ? gcn_stage_kernel<64, 5> : gcn_stage_kernel<64, 6>);
    }
    if (const int e = csk_ensure_lds((const void *)kern, r.lds)) return e;
    hipLaunchKernelGGL(kern, dim3(r.grid), dim3(NTHREADS), r.lds, s, p);
    if (r.ranges > 1) {
        if (const int e = (int)hipGetLastError()) return e;
        const int64_t work = (int64_t)c.c_out * c.frames * c.V;
        hipLaunchKernelGGL(gcn_reduce_kernel, dim3((unsigned)((work + 255) / 256), c.n_seg), dim3(256), 0, s, p);
    }
    return (int)hipGetLastError();
}

// the three queries: no operand but ell_cnt is dereferenced, so only that one is refused when null
static int gcn_stage_query(const GcnCall &c, GcnRoute *r) {
    if (!c.ell_cnt) CSK_FAIL("gcn_stage: null pointer");
    GcnParams p;
    return gcn_stage_route(c, &p, r);
}

extern "C" int csk_gcn_stage_f32(const float *x, float *y, const float *w, const float *bias, const int32_t *ell_src,
                                 const float *ell_val, const int32_t *ell_cnt, int ell_w, int64_t adj_seg_stride,
                                 int adj_per_frame,
                                 int n_seg, int c_in, int c_out, int frames, int V, int64_t x_seg_stride,
                                 int64_t x_chan_stride, int64_t y_seg_stride, int64_t y_chan_stride, int res_mode,
                                 void *stream) {
    const GcnCall c = {x, y, w, bias, ell_src, ell_val, ell_cnt, ell_w, adj_seg_stride, adj_per_frame, n_seg, c_in, c_out, frames, V,
                       x_seg_stride, x_chan_stride, y_seg_stride, y_chan_stride, res_mode, 1, nullptr};
    return gcn_stage_impl(c, stream);
}

extern "C" int csk_gcn_stage_f32_tile(const float *x, const float *y, const int32_t *ell_cnt, int ell_w, int64_t adj_seg_stride,
                                      int adj_per_frame, int n_seg, int c_in, int c_out, int frames, int V, int64_t x_seg_stride,
                                      int64_t x_chan_stride, int64_t y_seg_stride, int64_t y_chan_stride, int res_mode) {
    const GcnCall c = {x, const_cast<float *>(y), nullptr, nullptr, nullptr, nullptr, ell_cnt, ell_w, adj_seg_stride, adj_per_frame, n_seg, c_in,
                       c_out, frames, V, x_seg_stride, x_chan_stride, y_seg_stride, y_chan_stride, res_mode, 1, nullptr};
    GcnRoute r;
    if (const int rc = gcn_stage_query(c, &r)) return rc;
    return r.tile16;
}

extern "C" int csk_gcn_stage_f32_route(const float *x, const float *y, const float *ell_val, const int32_t *ell_cnt, int ell_w,
                                       int64_t adj_seg_stride, int adj_per_frame, int n_seg, int c_in, int c_out, int frames, int V,
                                       int64_t x_seg_stride, int64_t x_chan_stride, int64_t y_seg_stride, int64_t y_chan_stride,
                                       int res_mode) {
    const GcnCall c = {x, const_cast<float *>(y), nullptr, nullptr, nullptr, ell_val, ell_cnt, ell_w, adj_seg_stride, adj_per_frame, n_seg, c_in,
                       c_out, frames, V, x_seg_stride, x_chan_stride, y_seg_stride, y_chan_stride, res_mode, 1, nullptr};
    GcnRoute r;
    if (const int rc = gcn_stage_query(c, &r)) return rc;
    return gcn_route_code(r);
}

// what the split entry and its route query refuse before anything else
static int gcn_splitk_args(int ksplit, const float *partial) {
    if (ksplit < 1 || ksplit > 32 || (ksplit > 1 && !partial)) CSK_FAIL("gcn_stage_splitk: ksplit must be in [1, 32] and needs a partial-sum buffer");
    return 0;
}

extern "C" int csk_gcn_stage_splitk_f32_route(const float *x, const float *y, const float *ell_val, const int32_t *ell_cnt, int ell_w, int n_seg,
                                              int c_in, int c_out, int frames, int V, int64_t x_seg_stride, int64_t x_chan_stride,
                                              int64_t y_seg_stride, int64_t y_chan_stride, int res_mode, int ksplit, const float *partial) {
    if (const int rc = gcn_splitk_args(ksplit, partial)) return rc;
    const GcnCall c = {x, const_cast<float *>(y), nullptr, nullptr, nullptr, ell_val, ell_cnt, ell_w, 0, 0, n_seg, c_in, c_out, frames, V,
                       x_seg_stride, x_chan_stride, y_seg_stride, y_chan_stride, res_mode, ksplit, const_cast<float *>(partial)};
    GcnRoute r;
    if (const int rc = gcn_stage_query(c, &r)) return rc;
    return gcn_route_code(r);
}

extern "C" int csk_gcn_stage_splitk_f32(const float *x, float *y, const float *w, const float *bias, const int32_t *ell_src,
                                        const float *ell_val, const int32_t *ell_cnt, int ell_w, int n_seg, int c_in, int c_out,
                                        int frames, int V, int64_t x_seg_stride, int64_t x_chan_stride, int64_t y_seg_stride,
                                        int64_t y_chan_stride, int res_mode, int ksplit, float *partial, void *stream) {
    if (const int rc = gcn_splitk_args(ksplit, partial)) return rc;
    const GcnCall c = {x, y, w, bias, ell_src, ell_val, ell_cnt, ell_w, 0, 0, n_seg, c_in, c_out, frames, V,
                       x_seg_stride, x_chan_stride, y_seg_stride, y_chan_stride, res_mode, ksplit, partial};
    return gcn_stage_impl(c, stream);
}


// ------------------------------------------------------------------------------------------------
// Bare 1 x 1 conv + bias on the GCN-stage layouts (no adjacency, no residual, no ReLU): the fused a_i / b_i embedding convs
// of A-GCN (models/a_gcn/a_gcn.py:27-28, 53-59): one GEMM [c_out x c_in] . [c_in x positions] per segment.
// ------------------------------------------------------------------------------------------------
extern "C" int csk_conv1x1_f32(const float *x, float *y, const float *w, const float *bias, int n_seg, int c_in, int c_out,
                               int frames, int V, int64_t x_seg_stride, int64_t x_chan_stride, int64_t y_seg_stride,
                               int64_t y_chan_stride, void *stream) {
    if (!x || !y || !w || !bias) CSK_FAIL("conv1x1: null pointer");
    if (n_seg <= 0 || c_in <= 0 || c_out <= 0 || frames <= 0 || V < 2 || V > 64) CSK_FAIL("conv1x1: bad dims");
    const int32_t no_adjacency[3] = {0, 0, 0};
    const GcnCall c = {x, y, w, bias, nullptr, nullptr, no_adjacency, 1, 0, 0, n_seg, c_in, c_out, frames, V,
                       x_seg_stride, x_chan_stride, y_seg_stride, y_chan_stride, CSK_RES_NONE, 1, nullptr};
    GcnParams p = gcn_params(c);
    p.R = 1;                                               // one operand subset: the conv itself
    if (const int rc = GcnTile::positions_guard(p, "conv1x1")) return rc;
    const GcnTile tile(p);
    const bool big = tile.MT == 128;
    if (p.ldb > (big ? 192 : 320)) CSK_FAIL("conv1x1: activation tile of %d positions exceeds the staged maximum", p.ldb);
    if (const int rc = GcnTile::grid_guard(p, n_seg, "conv1x1")) return rc;
    constexpr int KCP = 16;                                // channels per chunk: 32 MFMAs per wave and barrier
    const size_t lds = 2 * (size_t)(KCP * tile.MT + KCP * p.ldb) * sizeof(float);
    void (*k)(GcnParams) = big ? gcn_stage_sparse2_kernel<128, false, KCP, true> : gcn_stage_sparse2_kernel<64, false, KCP, true>;
    if (const int e = csk_ensure_lds((const void *)k, lds)) return e;
    hipLaunchKernelGGL(k, dim3(p.qtiles * p.mtiles * n_seg), dim3(NTHREADS), lds, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}
