// step.hip -- gfx950 kernels for the CoST-GCN continual (frame-by-frame) path.
//
// State lives in a persistent HBM slab in CHANNEL-MAJOR layout: one frame of activations for all streams is
// a (C, P) matrix, P = n_streams * M * V positions (padded to a multiple of 4), position = (skeleton, joint)
// with the joint innermost.  Per block (depths per layer, from the frames max_in ONE launch can bring it: CSK_CO_Y_SLOTS /
// CSK_CO_IN_SLOTS in include/cskel.h, 16 / 12 for the default 8-frame cycles):
//     y ring   [8 + max_in][C_out][P]   post-GCN frames  (the (k-1) = 8-frame window of co.Conv2d + the new frames of a
//                                        launch cycle)
//     out ring [4 + max_in][C_out][P]   block outputs    (doubles as the next block's input / residual history,
//                                        co.Delay(4), plus the frames of a cycle in flight)
// A cycle of a block = gcn_stage on the new frames (gcn.hip, frames == skeletons) writing ring slots s % depth ..., then
// tcn_step below for the emitting steps: the 9 taps of the temporal conv are 9 consecutive ring slots at the SAME
// positions, so the GEMM is  D[co, p] = sum_r sum_c W[r][c][co] * ring[(head - 8 + r) % slots][c][p].
// Zero-initialised slots reproduce the zero left-padding of the clip conv (models/base.py:307-334 semantics).
// (A bare CoTemporalConvolution uses the same kernel on a ring of exactly k slots.)
// The kernels here are the 32x32x2 tiles, for the launches csk_tcn_step16_tile does not take: split-K (latency mode), k != 9,
// P < 8, rings >= 4 GB.  Every other temporal step, and the fused block / stack step (csk_co_block_step_f32,
// csk_co_stack_step_f32), runs on the tiles of step16.hip.
#include <type_traits>

#include "mfma_core.h"
#include "step_params.h"

// ------------------------------------------------------------------------------------------------
// ring staging: NS ring slots x KC channel rows x NP positions -> Bl [slot][KC][NP]
// ------------------------------------------------------------------------------------------------
// A workgroup tile of NT = 16384/MT columns is E emissions x NP = NT/E positions: the E emissions of a launch cycle
// at the same positions share all but (E-1)*head_step of their 9 ring slots, so one staged window of
//     S = K-1 + (E-1)*head_step + 1   slots
// serves E*K taps (E = 4: 12 slots instead of 36 -- the step analogue of the clip kernel's temporal halo), and a tap
// of emission j is the LDS row block  j*head_step + r.
// Staging sweep u of a thread covers row u*RPU + tid/N4 of the [slot][kk] row space (RPU = 256/N4 rows per sweep).
// A wave covers whole rows of ONE slot in every sweep (N4 <= 64, rows per wave divide KC), so the slot of a sweep is
// wave-uniform: slot bases stay on the scalar unit.  Rows past the window (sweep padding, K < 9) re-stage its last
// slot into LDS rows that are never read.
template <int NP, int NS>
struct RingStage {
    static constexpr int N4 = NP / 4;
    static constexpr int RPU = NTHREADS / N4;                       // rows per sweep: 4 (NP=256) .. 16 (NP=64)
    // window() makes a sweep's ring-slot offset wave-uniform with readfirstlane: legal only if a wave's rows of a sweep
    // (64 / N4 of them) never straddle two slots, i.e. they divide the KC rows of a slot
    static_assert(NP <= 256 && N4 <= 64 && KC % (64 / N4) == 0, "a wave's rows of a sweep must lie inside one ring slot");
    static constexpr int NB = (NS * KC + RPU - 1) / RPU;            // f32x4 per thread per chunk
    static constexpr int LDS_FLOATS = NB * RPU * NP;
    unsigned poff;                                                  // clamped position offset inside the tile
    int krow;                                                       // tid / N4: row inside a sweep
    int64_t soff[NB];                                               // element offset of this wave's ring slot per sweep (uniform)
    f32x4 v[NB];
    __device__ __forceinline__ void setup(int p0, int64_t P, int tid) {
        krow = tid / N4;
        poff = (unsigned)min((tid % N4) * 4, (int)(P - 4 - p0));    // last legal f32x4 start relative to p0
    }
    // window slot w lives in ring slot (first + w*step) mod slots of Cs channel rows each (computed once per phase)
    __device__ __forceinline__ void window(int first, int step, int slots, int nwin, int Cs, int64_t P) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int w = min((u * RPU + krow) / KC, nwin - 1);
            const int64_t o = (int64_t)((first + w * step) % slots) * Cs * P;
            soff[u] = ((int64_t)__builtin_amdgcn_readfirstlane((int)(o >> 32)) << 32) |
                      (unsigned)__builtin_amdgcn_readfirstlane((int)o);
        }
    }
    // base = ring + p0 (uniform); rows c0 + kk, channels >= C read as zero
    template <int U0, int U1>
    __device__ __forceinline__ void issue_range(const float *__restrict__ base, int C, int64_t P, int c0) {
#pragma unroll
        for (int u = U0; u < U1; ++u) {
            const int c = c0 + (u * RPU + krow) % KC;
            const f32x4 x = *reinterpret_cast<const f32x4 *>(base + soff[u] + (int64_t)min(c, C - 1) * P + poff);
            v[u] = x * (c < C ? 1.f : 0.f);
        }
    }
    // NU = sweeps actually needed (compile-time: ceil(window_slots*KC / RPU))
    template <int NU = NB>
    __device__ __forceinline__ void issue(const float *__restrict__ base, int C, int64_t P, int c0) {
        issue_range<0, (NU < NB ? NU : NB)>(base, C, P, c0);
    }
    // one third of the chunk's sweeps (G is a literal so that register indices are static)
    template <int G>
    __device__ __forceinline__ void issue_third(const float *__restrict__ base, int C, int64_t P, int c0) {
        issue_range<G * NB / 3, (G + 1) * NB / 3>(base, C, P, c0);
    }
    template <int NU = NB>
    __device__ __forceinline__ void commit(float *__restrict__ Bl) const {
#pragma unroll
        for (int u = 0; u < (NU < NB ? NU : NB); ++u) *reinterpret_cast<f32x4 *>(Bl + (u * RPU + krow) * NP + poff) = v[u];
    }
};


// E = emissions per workgroup tile (folded into the tile's column axis, see RingStage), HS = head_step of the launch
// (1, or 2 for a stride-2 block; only meaningful for E > 1).  SPLIT = false is the throughput kernel; the split-K form
// is a separate instantiation (E = 1) so that its extra index arithmetic costs the default path nothing.
template <int MT, int E, int HS, bool SPLIT, bool K9 = true, bool HALVES = false>
__device__ __forceinline__ void tcn_step_tile(const StepParams &p, const int bx, const int by, const int bz, float *smem) {
    constexpr int NT = 16384 / MT;
    constexpr int NP = NT / E;                      // positions per tile
    constexpr int NS = 8 + (E - 1) * HS + 1;        // window slots staged per chunk (K = 9)
    constexpr int WM = MT / 64;
    static_assert(NP >= 64, "a wave's 64 columns must belong to one emission");
    typedef RingStage<NP, NS> Stage;
    constexpr int NU_RES = (E * KC + Stage::RPU - 1) / Stage::RPU;      // sweeps of the residual-conv phase (E slots)
    float *Wl = smem;                       // [K][KC][MT]
    float *Bl = smem + 9 * KC * MT;         // [NS (+ sweep padding)][KC][NP]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int l31 = lane & 31, kh = lane >> 5;
    const int m0 = by * MT, p0 = bx * NP;
    const int64_t P = p.P;
    // emission group of this workgroup (bz = blockIdx.z): emissions j0 .. j0+E-1 of the launch; emission j has its newest
    // frame in slot head + j*head_step, its residual frame in xres slot xres_slot0 + j*xres_step and goes to out slot
    // out_slot0 + j (all modulo their ring depths)
    constexpr bool split = SPLIT;
    const int ks = split ? bz % p.ksplit : 0;
    const int j0 = (split ? bz / p.ksplit : bz) * E;
    const int jw = j0 + (wn * 64) / NP;                       // emission of this wave's 64 columns (wave-uniform)
    const int cb = ks * p.cper;                               // first channel of this split
    const int Cl = split ? min(p.C - cb, p.cper) : p.C;       // its channels (<= 0: padding-only split, sums stay zero)
    const int CpadL = split ? min(p.Cpad - cb, p.cper) : p.Cpad;
    const int nwin = p.K + (E - 1) * HS;                      // window slots actually used
    int first = (p.head + j0 * p.head_step - (p.K - 1)) % p.slots;     // ring slot of window slot 0
    if (first < 0) first += p.slots;
    const float *xres = p.xres + (int64_t)((p.xres_slot0 + jw * p.xres_step) % p.xres_slots) * p.Cres * P;
    float *out = split ? p.part + (int64_t)(jw * p.ksplit + ks) * p.Cout * P
                       : p.out + (int64_t)((p.out_slot0 + jw) % p.out_slots) * p.Cout * P;

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[a][b][g] = 0.f;

    const int offA = wm * 64 + l31;
    // B operand of (tap r, channel kk, this lane's column): Bl[((jl*HS + r)*KC + kk)*NP + column inside the emission]
    const int jl = (wn * 64) / NP, cw = (wn * 64) % NP;
    const int off0 = jl * HS * KC * NP + cw + l31, off1 = off0 + 32;
    WStage<MT> ws;
    Stage rs;
    // ---- phase 1: temporal conv over the ring window
    {
        const float *wbase = p.w + m0 + (size_t)cb * p.Mpad;
        const float *rbase = p.ring + (int64_t)cb * P + p0;
        // 9-tap chunks: the compact weight staging of mfma_core.h (one offset register instead of 2 x WB)
        using WS9 = typename std::conditional<MT == 128, WStage9x128, WStage9x64>::type;
        typename std::conditional<K9, WS9, WStage<MT> &>::type ws1 = [&]() -> decltype(auto) {
            if constexpr (K9) { WS9 w9; w9.setup(p.Cpad, p.Mpad, tid); return w9; }
            else { ws.setup(p.K, p.Cpad, p.Mpad, tid); return (ws); }
        }();
        rs.setup(p0, P, tid);
        ws1.issue(wbase);
        rs.window(first, 1, p.slots, nwin, p.C, P);
        rs.issue(rbase, Cl, P, 0);
        const int t1 = (p.K + 2) / 3, t2 = min(p.K, 2 * t1);
        constexpr bool k9 = K9;                          // 9 taps: straight-line 3-tap MFMA segments (mfma_taps_ct; spill-free at 155-236 VGPRs, kernel_resources.txt)
        int c0 = 0;
        for (; c0 + KC < CpadL; c0 += KC) {
            __syncthreads();
            ws1.commit(Wl);
            rs.commit(Bl);
            __syncthreads();
            // next chunk's loads in three bursts between three tap segments (see mfma_taps in mfma_core.h)
            const float *wnext = wbase + (size_t)(c0 + KC) * p.Mpad;
#pragma unroll
            for (int j = 0; j < 3; ++j) ws1.issue_slot(j, wnext);
            rs.template issue_third<0>(rbase, Cl, P, c0 + KC);
            __builtin_amdgcn_s_setprio(1);
            if (k9) mfma_taps_ct<MT, 3>(Wl, Bl, 0, NP, KC * NP, offA, off0, off1, kh, acc);
            else mfma_taps<MT>(Wl, Bl, 0, t1, NP, KC * NP, offA, off0, off1, kh, acc);
            __builtin_amdgcn_s_setprio(0);
#pragma unroll
            for (int j = 3; j < 6; ++j) ws1.issue_slot(j, wnext);
            rs.template issue_third<1>(rbase, Cl, P, c0 + KC);
            __builtin_amdgcn_s_setprio(1);
            if (k9) mfma_taps_ct<MT, 3>(Wl, Bl, 3, NP, KC * NP, offA, off0, off1, kh, acc);
            else if (t1 < t2) mfma_taps<MT>(Wl, Bl, t1, t2, NP, KC * NP, offA, off0, off1, kh, acc);
            __builtin_amdgcn_s_setprio(0);
#pragma unroll
            for (int j = 6; j < 9; ++j) ws1.issue_slot(j, wnext);
            rs.template issue_third<2>(rbase, Cl, P, c0 + KC);
            __builtin_amdgcn_s_setprio(1);
            if (k9) mfma_taps_ct<MT, 3>(Wl, Bl, 6, NP, KC * NP, offA, off0, off1, kh, acc);
            else if (t2 < p.K) mfma_taps<MT>(Wl, Bl, t2, p.K, NP, KC * NP, offA, off0, off1, kh, acc);
            __builtin_amdgcn_s_setprio(0);
        }
        __syncthreads();
        ws1.commit(Wl);
        rs.commit(Bl);
        __syncthreads();
        mfma_chunk<MT>(Wl, Bl, p.K, NP, KC * NP, offA, off0, off1, kh, acc);
    }
    // ---- phase 2: 1x1 residual conv on the delayed block input (CoTempConv k=1 + co.Delay, base.py:424-441): the
    // window is the E residual frames of the tile's emissions, one "tap" each
    if (p.res_mode == CSK_RES_CONV && ks == 0) {
        const float *wbase = p.wres + m0;
        const float *xbase = p.xres + p0;
        const int xfirst = (p.xres_slot0 + j0 * p.xres_step) % p.xres_slots;
        const int offr0 = jl * KC * NP + cw + l31, offr1 = offr0 + 32;
        ws.setup(1, p.CresPad, p.Mpad, tid);
        ws.issue(wbase);
        rs.window(xfirst, p.xres_step, p.xres_slots, E, p.Cres, P);
        rs.template issue<NU_RES>(xbase, p.Cres, P, 0);
        for (int c0 = 0; c0 < p.CresPad; c0 += KC) {
            __syncthreads();
            ws.commit(Wl);
            rs.template commit<NU_RES>(Bl);
            __syncthreads();
            if (c0 + KC < p.CresPad) {
                ws.issue(wbase + (size_t)(c0 + KC) * p.Mpad);
                rs.template issue<NU_RES>(xbase, p.Cres, P, c0 + KC);
            }
            mfma_chunk<MT>(Wl, Bl, 1, NP, KC * NP, offA, offr0, offr1, kh, acc);
        }
    }
    // ---- epilogue: + bias (+ identity residual), ReLU, stores.  Same scheme as tcn_stage_kernel: on full tiles the row
    // base pointers are wave-uniform (scalar unit) and every access carries one 32-bit lane byte offset;
    // v_permlane32_swap pairs the ni = 0 / 1 registers so that a store instruction writes one 256-B row segment.
    // (split-K: raw partial sums -- bias, identity residual and ReLU are applied by step_reduce_kernel)
    const bool ident = !split && p.res_mode == CSK_RES_IDENTITY;
    const bool relu = !split && p.relu;
    const int rbase = m0 + wm * 64;
    const bool full = p.fast_epi && m0 + MT <= p.Cout;
    const unsigned kh4 = 4u * (unsigned)kh;
    const int pw = p0 + cw;                                   // first position of this wave's columns
    // Operands are loaded and consumed one 32-row half (mi) at a time when HALVES (the 168-register instantiation: 64
    // accumulators + 2 x 48 operands would not fit), else both halves up front (all loads in flight together).
    float bv[2][16], rv[2][2][16];
    auto load_half = [&](int mi) {
        if (full) {
#pragma unroll
            for (int g = 0; g < 16; ++g)
                bv[mi][g] = split ? 0.f : ld_lane(p.bias + (rbase + mi * 32 + (g & 3) + 8 * (g >> 2)), kh4 * 4u);
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const unsigned lo = 4u * (kh4 * (unsigned)P + (unsigned)min((int64_t)(pw + ni * 32 + l31), P - 1));
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const float *rrow = xres + (int64_t)(rbase + mi * 32 + (g & 3) + 8 * (g >> 2)) * P;
                    rv[ni][mi][g] = ident ? ld_lane(rrow, lo) : 0.f;
                }
            }
        } else {
#pragma unroll
            for (int g = 0; g < 16; ++g) bv[mi][g] = split ? 0.f : p.bias[rbase + mi * 32 + 4 * kh + (g & 3) + 8 * (g >> 2)];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int64_t qc = min((int64_t)(pw + ni * 32 + l31), P - 1);
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int co = rbase + mi * 32 + 4 * kh + (g & 3) + 8 * (g >> 2);
                    rv[ni][mi][g] = ident ? xres[(int64_t)min(co, p.Cout - 1) * P + qc] : 0.f;
                }
            }
        }
    };
    const int64_t qb = (int64_t)pw + lane;
    const bool qv = qb < P;
    auto finish_half = [&](int mi) {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            float v0 = acc[mi][0][g] + bv[mi][g] + rv[0][mi][g];
            float v1 = acc[mi][1][g] + bv[mi][g] + rv[1][mi][g];
            if (relu) { v0 = relu_nan(v0); v1 = relu_nan(v1); }
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(v0), __float_as_uint(v1), false, false);
            acc[mi][0][g] = __uint_as_float(sw[0]);            // row rbase + mi*32 + (g&3) + 8(g>>2), column qb
            acc[mi][1][g] = __uint_as_float(sw[1]);            // row + 4
        }
        if (full) {
            if (qv) {
                const unsigned qo = 4u * (unsigned)qb;
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    float *orow = out + (int64_t)(rbase + mi * 32 + (g & 3) + 8 * (g >> 2)) * P;
                    st_lane(orow, qo, acc[mi][0][g]);
                    st_lane(orow + 4 * P, qo, acc[mi][1][g]);
                }
            }
        } else {
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row0 = rbase + mi * 32 + (g & 3) + 8 * (g >> 2);
                if (qv && row0 < p.Cout) out[(int64_t)row0 * P + qb] = acc[mi][0][g];
                if (qv && row0 + 4 < p.Cout) out[(int64_t)(row0 + 4) * P + qb] = acc[mi][1][g];
            }
        }
    };
    if (HALVES) {
        load_half(0);
        finish_half(0);
        __builtin_amdgcn_sched_barrier(0);
        load_half(1);
        finish_half(1);
    } else {
        load_half(0);
        load_half(1);
        finish_half(0);
        finish_half(1);
    }
}

// OCC = 3: the same kernel within 168 registers (three workgroups per CU), for launches whose workgroup count fits 768 resident
// slots in fewer rounds than 512 (CoAGCN at the Kinetics shape: 576 tiles per 64-channel block)
template <int MT, int E, int HS, bool SPLIT, bool K9, int OCC = 2>
__global__ __launch_bounds__(NTHREADS, OCC) void tcn_step_kernel(const StepParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // XCD-aware work-item order (mfma_core.h): every XCD walks a contiguous range of items; m-tile fastest, then emission
    // group, then position tile -- the m-tiles of a position tile read the SAME ring window (and emission groups at the
    // same positions all but a few slots of it); with a plain (x, y, z) grid they sat gridDim.x dispatches apart, by when
    // the window had left the 4 MB L2 (C = 256 launches fetched 966 MB for 525 MB of operands)
    const unsigned wid = xcd_contiguous_id(blockIdx.x, gridDim.x);
    tcn_step_tile<MT, E, HS, SPLIT, K9, OCC == 3>(p, (int)(wid / (p.gy * p.gz)), (int)(wid % p.gy), (int)((wid / p.gy) % p.gz), smem);
}

// split-K reduction: out_j[co][p] = ReLU?( sum_ks part[j*ksplit + ks][co][p] (fixed order) + bias[co] + identity residual )
__global__ __launch_bounds__(256) void step_reduce_kernel(const StepParams p) {
    const int64_t P = p.P, P4 = P / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;            // (co, p4)
    if (i >= (int64_t)p.Cout * P4) return;
    const int co = (int)(i / P4);
    const int64_t q = (i - (int64_t)co * P4) * 4;
    const int j = blockIdx.y;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < p.ksplit; ++ks)
        s += *reinterpret_cast<const f32x4 *>(p.part + ((int64_t)(j * p.ksplit + ks) * p.Cout + co) * P + q);
    s += p.bias[co];
    if (p.res_mode == CSK_RES_IDENTITY) {
        const float *xres = p.xres + (int64_t)((p.xres_slot0 + j * p.xres_step) % p.xres_slots) * p.Cres * P;
        s += *reinterpret_cast<const f32x4 *>(xres + (int64_t)co * P + q);
    }
    if (p.relu) { s[0] = relu_nan(s[0]); s[1] = relu_nan(s[1]); s[2] = relu_nan(s[2]); s[3] = relu_nan(s[3]); }
    float *out = p.out + (int64_t)((p.out_slot0 + j) % p.out_slots) * p.Cout * P;
    *reinterpret_cast<f32x4 *>(out + (int64_t)co * P + q) = s;
}

// feat[n, c] = mean over the M*V positions of stream n in a channel-major frame h (C, P): one wave per (n, c)
__global__ __launch_bounds__(256) void co_spatial_pool_kernel(const float *__restrict__ h, float *__restrict__ feat,
                                                              int N, int C, int MV, int64_t P) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= (int64_t)N * C) return;
    const int n = row / C, c = row % C;
    const float *src = h + (int64_t)c * P + (int64_t)n * MV;
    float s = 0.f;
    for (int j = lane; j < MV; j += 64) s += src[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) feat[row] = s / (float)MV;
}

// pooled[i] = (1/window) * sum over `count` valid ring entries (zero-initialised window, fixed divisor:
// AvgPool1d count_include_pad semantics); entries are visited oldest -> newest so the sum order is fixed
__global__ void co_window_mean_kernel(const float *__restrict__ ring, float *__restrict__ pooled, int64_t n_elem,
                                      int window, int head, int count) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n_elem) return;
    float s = 0.f;
    for (int j = count - 1; j >= 0; --j) {
        int slot = (head - j) % window;
        if (slot < 0) slot += window;
        s += ring[(int64_t)slot * n_elem + i];
    }
    pooled[i] = s / (float)window;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// The ONE decision of a launch, asked once: step_route makes it, csk_tcn_step_f32 launches from it, csk_tcn_step_f32_route reports it.
enum { STEP_TILE16 = 1, STEP_TILE32 = 2 };      // family: tcn_step16_kernel (step16.hip), code = csk_tcn_step16_tile's value | tcn_step_kernel, code = step_code
struct StepRoute { int family, code; unsigned gx, gy, gz; int64_t grid; };     // STEP_TILE32: position tiles, m-tiles, emission groups * ranges; their product
constexpr int step_code(int MT, int E, int HS, bool SPLIT, bool K9, int OCC) { return MT * 100000 + E * 10000 + HS * 1000 + SPLIT * 100 + K9 * 10 + OCC; }

// Every k = 9, unsplit launch whose rings fit 32-bit byte offsets runs on the slot-balanced 16x16x4 tiles (step16.hip), whatever its size: that
// family has its own fp32 summation order.  The others run tcn_step_kernel<MT, E, HS, SPLIT, K9, OCC>: the ONE copy of that rule.  Host arithmetic.
static StepRoute step_route(const StepParams &p, int n_emit) {
    if (const int tile = csk_tcn_step16_tile(p, n_emit)) return {STEP_TILE16, tile};
    const bool big = (p.Mpad % 128) == 0, split = p.ksplit > 1, k9 = p.K == 9;
    const int MT = big ? 128 : 64;
    // emissions folded into a workgroup tile: the largest E in {4, 2, 1} that divides n_emit and leaves >= 64 positions
    // per emission (a wave's 64 columns must belong to one emission); stride-2 launches only as 128-row tiles of two
    // emissions (the only stride-2 shapes of the ST-GCN stack); k != 9, and split-K on the 64-row tiles, use the plain tile.
    int E = 1;
    if (k9 && !big && p.head_step == 1 && !split) E = (n_emit % 4 == 0) ? 4 : (n_emit % 2 == 0) ? 2 : 1;
    if (k9 && big && p.head_step >= 1 && p.head_step <= 2) E = (n_emit % 2 == 0) ? 2 : 1;      // also with split-K
    const int HS = big && E == 2 ? p.head_step : 1, NP = 16384 / MT / E;
    const unsigned gx = (unsigned)((p.P + NP - 1) / NP), gy = (unsigned)(p.Mpad / MT), gz = (unsigned)((n_emit / E) * p.ksplit);
    const int64_t g = (int64_t)gx * gy * gz;
    // The 64-row, four-emission form also exists within 168 registers (three workgroups per CU, 43 KB of LDS each): taken when
    // the launch needs fewer rounds of 768 resident workgroups than of 512 (256 CUs) -- CoAGCN at the Kinetics shape is 576
    // tiles per 64-channel block: one round instead of a full one plus an eighth.  A function of the launch size only.
    const int OCC = !big && E == 4 && (g + 767) / 768 < (g + 511) / 512 ? 3 : 2;       // (E == 4: unsplit, k == 9)
    return {STEP_TILE32, step_code(MT, E, HS, split, k9, OCC), gx, gy, gz, g};
}

struct StepKernel { void (*kern)(StepParams); size_t lds; };        // code -> kernel and LDS bytes of the 15 instantiations step_route can name
static StepKernel step_kernel_of(int code) {
    switch (code) {
#define CSK_STEP32(MT, E, HS, ...) case step_code(MT, E, HS, __VA_ARGS__): return {tcn_step_kernel<MT, E, HS, __VA_ARGS__>, (9 * KC * MT + RingStage<16384 / MT / E, 8 + (E - 1) * HS + 1>::LDS_FLOATS) * sizeof(float)};
        CSK_STEP32(128, 2, 2, true, true, 2) CSK_STEP32(128, 2, 1, true, true, 2) CSK_STEP32(128, 1, 1, true, true, 2) CSK_STEP32(128, 1, 1, true, false, 2)
        CSK_STEP32(64, 1, 1, true, true, 2) CSK_STEP32(64, 1, 1, true, false, 2) CSK_STEP32(128, 2, 2, false, true, 2) CSK_STEP32(128, 2, 1, false, true, 2)
        CSK_STEP32(128, 1, 1, false, true, 2) CSK_STEP32(128, 1, 1, false, false, 2) CSK_STEP32(64, 4, 1, false, true, 2) CSK_STEP32(64, 2, 1, false, true, 2)
        CSK_STEP32(64, 1, 1, false, true, 2) CSK_STEP32(64, 1, 1, false, false, 2) CSK_STEP32(64, 4, 1, false, true, 3)
#undef CSK_STEP32
    }
    return {nullptr, 0};
}

// what only csk_tcn_step_f32 requires: the limits of its step_check (step_params.h)
static int step_limits_f32(const StepCall &c, bool operands) {
    if (c.ksplit < 1 || c.ksplit > 32 || (operands && c.ksplit > 1 && !c.partial)) CSK_FAIL("tcn_step: ksplit must be in [1, 32] and needs a partial-sum buffer");
    if (c.k < 1 || c.k > 9) CSK_FAIL("tcn_step: bad k/slots/head");
    if (c.head_step < 0) CSK_FAIL("tcn_step: bad emission geometry");
    if (c.P >= (1ll << 31) - 256) CSK_FAIL("tcn_step: P too large");
    return 0;
}

extern "C" int csk_tcn_step_f32(const float *ring, int slots, int head, int head_step, int n_emit, const float *w,
                                const float *x_res, int x_res_slots, int x_res_slot0, int x_res_step,
                                const float *w_res, const float *bias, float *out, int out_slots, int out_slot0,
                                int c, int c_out, int64_t P, int k, int res_mode, int c_res, int relu, int ksplit,
                                float *partial, void *stream) {
    const StepCall call = {ring, slots, head, head_step, n_emit, w, x_res, x_res_slots, x_res_slot0, x_res_step, w_res, bias, out,
                           out_slots, out_slot0, c, c_out, P, k, res_mode, c_res, relu, ksplit, partial};
    if (const int rc = step_check("tcn_step", "k/slots/head", call, true, [&] { return step_limits_f32(call, true); })) return rc;
    StepParams p = step_params(call);
    const StepRoute r = step_route(p, n_emit);
    if (p.ksplit > 1 && ((uintptr_t)partial & 15)) CSK_FAIL("tcn_step: partial-sum buffer must be 16-byte aligned");
    if (r.family == STEP_TILE16) return csk_launch_tcn_step16(p, n_emit, r.code, stream);
    if (r.grid >= (1ll << 31)) CSK_FAIL("tcn_step: grid too large");
    p.gx = r.gx; p.gy = r.gy; p.gz = r.gz;
    const StepKernel sk = step_kernel_of(r.code);
    hipStream_t s = (hipStream_t)stream;
    if (const int e = csk_ensure_lds((const void *)sk.kern, sk.lds)) return e;
    hipLaunchKernelGGL(sk.kern, dim3((unsigned)r.grid), dim3(NTHREADS), sk.lds, s, p);
    if (p.ksplit > 1) {
        if (const int e = (int)hipGetLastError()) return e;
        const int64_t work = (int64_t)c_out * (P / 4);
        hipLaunchKernelGGL(step_reduce_kernel, dim3((unsigned)((work + 255) / 256), n_emit), dim3(256), 0, s, p);
    }
    return (int)hipGetLastError();
}

// The query: the shape arguments of the entry as a call without operands (x_res_slots <= 0: no x_res; otherwise an x_res that is
// there and never read), checked at the shape level and routed as the entry routes it
extern "C" int csk_tcn_step_f32_route(int slots, int head_step, int n_emit, int x_res_slots, int out_slots, int c, int c_out, int64_t P,
                                      int k, int res_mode, int c_res, int ksplit, int32_t *route) {
    if (!route) CSK_FAIL("tcn_step_route: null route");
    static const float there = 0.f;
    const StepCall call = {nullptr, slots, 0, head_step, n_emit, nullptr, x_res_slots > 0 ? &there : nullptr, x_res_slots, 0, 0,
                           nullptr, nullptr, nullptr, out_slots, 0, c, c_out, P, k, res_mode, c_res, 1, ksplit, nullptr};
    if (const int rc = step_check("tcn_step", "k/slots/head", call, false, [&] { return step_limits_f32(call, false); })) return rc;
    const StepRoute r = step_route(step_params(call), n_emit);
    route[0] = r.family; route[1] = r.code; route[2] = r.grid < (1ll << 31) ? (int32_t)r.grid : -1;
    return 0;
}

extern "C" int csk_tcn_step_f32_tile(int slots, int head_step, int n_emit, int x_res_slots, int out_slots, int c, int c_out, int64_t P,
                                     int k, int res_mode, int c_res, int ksplit) {
    int32_t route[CSK_STEP_ROUTE_WORDS];
    if (const int rc = csk_tcn_step_f32_route(slots, head_step, n_emit, x_res_slots, out_slots, c, c_out, P, k, res_mode, c_res, ksplit, route)) return rc;
    return route[0] == STEP_TILE16 ? route[1] : 0;
}

extern "C" int csk_co_spatial_pool_f32(const float *h, float *feat, int N, int C, int MV, int64_t P, void *stream) {
    if (!h || !feat) CSK_FAIL("co_spatial_pool: null pointer");
    if (N <= 0 || C <= 0 || MV <= 0 || (int64_t)N * MV > P) CSK_FAIL("co_spatial_pool: bad dims");
    const int64_t rows = (int64_t)N * C;
    hipLaunchKernelGGL(co_spatial_pool_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, h,
                       feat, N, C, MV, P);
    return (int)hipGetLastError();
}

extern "C" int csk_co_window_mean_f32(const float *ring, float *pooled, int64_t n_elem, int window, int head,
                                      int count, void *stream) {
    if (!ring || !pooled) CSK_FAIL("co_window_mean: null pointer");
    if (n_elem <= 0 || window <= 0 || head < 0 || head >= window || count < 0 || count > window)
        CSK_FAIL("co_window_mean: bad dims");
    hipLaunchKernelGGL(co_window_mean_kernel, dim3((unsigned)((n_elem + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, ring, pooled, n_elem, window, head, count);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Multi-stream logit fusion + top-k (scripts/multi_stream_eval.py:33-60): fused = left fold of add / maximum over
// up to 4 prediction arrays (N, classes); rank[n] = number of classes scoring strictly higher than the target
// class (top-k hit <=> rank < k).  One wave per sample.
// ------------------------------------------------------------------------------------------------
struct FuseParams {
    const float *preds[4];
    int n_streams, use_max, N, classes;
    int64_t sample_stride, class_stride;    // element strides of the (N, classes[, steps]) arrays
};

__global__ __launch_bounds__(256) void fuse_rank_kernel(const FuseParams p, const int64_t *__restrict__ targets,
                                                        float *__restrict__ fused, int *__restrict__ rank) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + wave;
    if (n >= p.N) return;
    const int64_t tgt = targets ? targets[n] : -1;
    float tv = 0.f;
    if (tgt >= 0 && tgt < p.classes) {                     // fused score of the target class (same fold order)
        tv = p.preds[0][n * p.sample_stride + tgt * p.class_stride];
        for (int s = 1; s < p.n_streams; ++s) {
            const float v = p.preds[s][n * p.sample_stride + tgt * p.class_stride];
            tv = p.use_max ? __builtin_elementwise_maximum(tv, v) : tv + v;   // NaN-propagating, as np.maximum
        }
    }
    int higher = 0;
    for (int c = lane; c < p.classes; c += 64) {
        float f = p.preds[0][n * p.sample_stride + c * p.class_stride];
        for (int s = 1; s < p.n_streams; ++s) {
            const float v = p.preds[s][n * p.sample_stride + c * p.class_stride];
            f = p.use_max ? __builtin_elementwise_maximum(f, v) : f + v;
        }
        if (fused) fused[n * p.classes + c] = f;
        higher += (f > tv) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) higher += __shfl_xor(higher, o);
    if (rank && lane == 0) rank[n] = (tgt >= 0 && tgt < p.classes) ? higher : p.classes;
}

extern "C" int csk_fuse_rank_f32(const float *const *preds, int n_streams, int use_max, int N, int classes,
                                 int64_t sample_stride, int64_t class_stride, const int64_t *targets, float *fused,
                                 int *rank, void *stream) {
    if (!preds || n_streams < 1 || n_streams > 4) CSK_FAIL("fuse_rank: 1..4 prediction arrays expected");
    if (N <= 0 || classes <= 0 || (!fused && !rank)) CSK_FAIL("fuse_rank: bad dims / no output requested");
    if (rank && !targets) CSK_FAIL("fuse_rank: rank requested without targets");
    FuseParams p;
    for (int s = 0; s < 4; ++s) {
        p.preds[s] = s < n_streams ? preds[s] : nullptr;
        if (s < n_streams && !preds[s]) CSK_FAIL("fuse_rank: null prediction array");
    }
    p.n_streams = n_streams; p.use_max = use_max; p.N = N; p.classes = classes;
    p.sample_stride = sample_stride; p.class_stride = class_stride;
    hipLaunchKernelGGL(fuse_rank_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p, targets,
                       fused, rank);
    return (int)hipGetLastError();
}
