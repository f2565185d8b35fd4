// step_split.hip -- OPT-IN step precision "bf16x3" of the continual temporal step (gfx950 / MI355X): the GEMM of tcn16_tile
// (step16.hip) on the bf16 matrix pipe.
//
//     out[slot(j)][co][p] = ReLU( sum_c sum_r W[r][c][co] * y_ring[(head + j head_step - 8 + r) mod slots][c][p] + bias[co] + residual )
//
// Arithmetic: that of tcn_split.hip -- every fp32 operand is three bf16 pieces x = h + m + l (split_core.h: split8), a product
// is the six piece products of order <= 2 (hl, lh, mm, mh, hm, hh in that order), each one v_mfma_f32_16x16x32_bf16 with fp32
// accumulation.  The identity residual stays exact fp32 (epilogue16, the epilogue of the exact step kernels); a 1 x 1 conv
// residual runs in split arithmetic.  It is NOT fp32 and never selected implicitly (continual.set_step_precision).
//
// Tile: 64 output channels x E emissions x 16 NBE positions; wave w owns channels 16 w .. 16 w + 15 and ALL column blocks, the
// MFMA issued "transposed" as in step16.hip (A = activations: 16 positions x 32 channels, B = weights: 32 channels x 16 output
// channels), so a lane holds 4 consecutive positions of one output channel and the epilogue is epilogue16's.
//
// K loop: a bf16 k-step is 32 channels of one tap -- the 9-slot window of a 32-channel chunk (6 B per element) does not fit
// the LDS the way the fp32 kernel's 4-channel window does.  The loop therefore walks (32-channel chunk, WINDOW SLOT): one ring
// slot of the chunk is staged (split at staging: a lane loads the 8 channels of its position, coalesced along positions,
// splits them and writes 3 x 16 B) and serves every emission of the tile that reads it -- emission j reads window slot w as
// tap r = w - j head_step.  A ring slot is loaded and split once per chunk whatever E is.  An output's summation order is
// (chunk ascending, tap ascending, the six products) for every E, tile width and launch size: a stream's results do not depend
// on how many streams share the slab nor on how many frames a launch carries.
//   Bl [piece][k-quarter][NP positions][8 ch]     one staged ring slot, K-contiguous: an A fragment is one ds_read_b128
// The weights are not staged: a wave's B fragment of (tap, chunk, piece) is 16 output channels x 32 channels = one 16-byte
// vector per lane of the host image (fold.pack_conv_weight_split, the image of csk_tcn_stage_bf16x3), loaded from L2 at the
// top of a stage -- in front of the barriers and the split of the stage's activations -- and feeds 6 NBE MFMAs.
// Two barriers per stage (the activation tile is single-buffered: two tiles of 400 positions do not fit twice per CU); the
// next stage's ring loads are in flight in registers under the stage's MFMAs.
#include "split_core.h"
#include "step_params.h"
#include "tile16.h"

namespace {

struct StepSplitParams {
    const float *ring, *xres, *bias;
    const u32x4 *w, *wres;          // split images: [C_pad / 16][9 | 3 tap slots][3 pieces][2 halves][Mpad] vectors of 8 bf16
    float *out;
    int C, nch16, Cout, Mpad, slots, head, head_step;
    int res_mode, Cres, nch16_res, relu;
    int xres_slots, xres_slot0, xres_step, out_slots, out_slot0;
    unsigned gx, gy, gz;
    int64_t P;
};

// one stage of the K loop (wave-uniform): the ring slot that is staged and, per emission of the tile, the image slot of
// the tap that reads it (-1: none)
template <int E>
struct Stage {
    const float *base;              // first channel row of the slot
    const u32x4 *img;               // image of the chunk's first 16 channels
    int C, c0, nch16_left, islot[E];
};

template <int NBE, int E, int HS>
__global__ __launch_bounds__(NTHREADS, 2) void tcn_step_split_kernel(const StepSplitParams p) {
    constexpr int NP = 16 * NBE, NB = E * NBE, U = 4 * NP, NSW = (U + NTHREADS - 1) / NTHREADS;
    constexpr int NS = 8 + (E - 1) * HS + 1;                    // window slots (K = 9)
    extern __shared__ __attribute__((aligned(16))) u32x4 smem4[];
    u32x4 *Bl = smem4;                                          // [3][4][NP]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kq = lane >> 4;
    const unsigned wid = xcd_contiguous_id(blockIdx.x, gridDim.x);
    const int bx = (int)(wid / (p.gy * p.gz)), by = (int)(wid % p.gy), bz = (int)((wid / p.gy) % p.gz);
    const int m0 = by * 64, p0 = bx * NP, j0 = bz * E;
    const int64_t P = p.P;
    int first = (p.head + j0 * p.head_step - 8) % p.slots;      // ring slot of window slot 0
    if (first < 0) first += p.slots;
    const int pmax = (int)(P - 1 - p0);                         // last position of the channel row, relative to the tile

    f32x4 acc[NB];
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nch32 = (p.nch16 + 1) / 2, nch32_res = p.res_mode == CSK_RES_CONV ? (p.nch16_res + 1) / 2 : 0;
    const int S1 = nch32 * NS, S = S1 + nch32_res * E;
    const int Mpad = p.Mpad;
    auto stage_of = [&](int s) {
        Stage<E> st;
        if (s < S1) {           // phase 1: chunk s / NS, window slot s % NS of the temporal conv
            const int c = s / NS, w = s - c * NS;
            st.base = p.ring + (int64_t)((first + w) % p.slots) * p.C * P;
            st.C = p.C; st.c0 = 32 * c; st.nch16_left = p.nch16 - 2 * c;
            st.img = p.w + (int64_t)(2 * c) * 9 * 6 * Mpad;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int r = w - j * HS;
                // class-major tap slots of the image: taps 0, 2, 4, 6, 8, 1, 3, 5, 7 for stride 2
                st.islot[j] = (r < 0 || r > 8) ? -1 : p.head_step == 2 ? ((r & 1) ? 5 + (r >> 1) : r >> 1) : r;
            }
        } else {                // phase 2: chunk t / E of the 1 x 1 residual conv on the delayed input of emission t % E
            const int t = s - S1, c = t / E, jj = t - c * E;
            st.base = p.xres + (int64_t)((p.xres_slot0 + (j0 + jj) * p.xres_step) % p.xres_slots) * p.Cres * P;
            st.C = p.Cres; st.c0 = 32 * c; st.nch16_left = p.nch16_res - 2 * c;
            st.img = p.wres + (int64_t)(2 * c) * 3 * 6 * Mpad;
#pragma unroll
            for (int j = 0; j < E; ++j) st.islot[j] = j == jj ? 0 : -1;
        }
        return st;
    };

    // ring loads of a stage: unit e = sweep * 256 + tid -> (k-quarter e / NP, position e % NP), the 8 channels of the unit.
    // Unconditional: the position is clamped into the channel row, the channel into [0, C) (rows past C meet zero weights;
    // the value only has to be what the ring holds), surplus threads redo the last unit.
    float v[NSW][8];
    auto issue = [&](const Stage<E> &st) {
#pragma unroll
        for (int u = 0; u < NSW; ++u) {
            const int e = min(u * NTHREADS + tid, U - 1);
            const int q = e / NP, pos = e - q * NP;
            const unsigned po = (unsigned)(p0 + min(pos, pmax));
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const unsigned c = (unsigned)min(st.c0 + 8 * q + i, st.C - 1);
                v[u][i] = ld_lane(st.base, (c * (unsigned)P + po) * 4u);
            }
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int u = 0; u < NSW; ++u) {
            const int e = min(u * NTHREADS + tid, U - 1);
            const int q = e / NP, pos = e - q * NP;
            bf16x8 ph, pm, pl;
            split8(v[u], ph, pm, pl);
            u32x4 *dst = Bl + q * NP + pos;
            dst[0] = __builtin_bit_cast(u32x4, ph);
            dst[4 * NP] = __builtin_bit_cast(u32x4, pm);
            dst[8 * NP] = __builtin_bit_cast(u32x4, pl);
        }
    };

    const int co = m0 + wave * 16 + l15;                        // < Mpad
    issue(stage_of(0));
    for (int s = 0; s < S; ++s) {
        const Stage<E> st = stage_of(s);
        const int nsl = s < S1 ? 9 : 3;                          // tap slots of the image
        // B fragments of the stage's taps: lane (l15, kq) holds channels 8 kq .. 8 kq + 7 of the chunk = half kq & 1 of
        // 16-channel image chunk kq >> 1; a chunk past the image (odd count of 16-channel chunks) reads as zero
        u32x4 wf[E][3];
        const bool have = (kq >> 1) < st.nch16_left;
        const int wo = ((kq >> 1) < st.nch16_left ? (kq >> 1) : 0) * nsl * 6 * Mpad + (kq & 1) * Mpad + co;
#pragma unroll
        for (int j = 0; j < E; ++j)
            if (st.islot[j] >= 0) {                             // (uniform)
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) {
                    const u32x4 x = st.img[wo + (st.islot[j] * 3 + pc) * 2 * Mpad];
                    wf[j][pc] = have ? x : u32x4{0u, 0u, 0u, 0u};
                }
            }
        __syncthreads();                                        // the previous stage's fragment reads are done
        commit();
        __syncthreads();
        if (s + 1 < S) issue(stage_of(s + 1));
#pragma unroll
        for (int j = 0; j < E; ++j)
            if (st.islot[j] >= 0) {
                const u32x4 *bl = Bl + kq * NP + l15;
#pragma unroll
                for (int cb = 0; cb < NBE; ++cb) {
                    bf16x8 a[3];
#pragma unroll
                    for (int pc = 0; pc < 3; ++pc) a[pc] = __builtin_bit_cast(bf16x8, bl[pc * 4 * NP + 16 * cb]);
                    constexpr int PW[6] = {0, 2, 1, 1, 0, 0}, PA[6] = {2, 0, 1, 0, 1, 0};   // (weight, activation) pieces: hl, lh, mm, mh, hm, hh
#pragma unroll
                    for (int t6 = 0; t6 < 6; ++t6)
                        acc[j * NBE + cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            a[PA[t6]], __builtin_bit_cast(bf16x8, wf[j][PW[t6]]), acc[j * NBE + cb], 0, 0, 0);
                }
            }
    }
    // ---- epilogue: + bias (+ identity residual, exact fp32), ReLU (tile16.h)
    unsigned oslot[E], xslot[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        oslot[j] = (unsigned)((int64_t)((p.out_slot0 + j0 + j) % p.out_slots) * p.Cout * P * 4);
        xslot[j] = (unsigned)((int64_t)((p.xres_slot0 + (j0 + j) * p.xres_step) % p.xres_slots) * p.Cres * P * 4);
    }
    const int nval = (int)min((int64_t)NP, P - p0);             // positions of the tile inside the row (a multiple of 4)
    epilogue16<NB, E, NP>(acc, p.bias, p.Cout, co, kq, p.res_mode == CSK_RES_IDENTITY, p.relu != 0, p.xres, p.out, xslot, oslot, P, P,
                          p0, nval, nval);
}

template <int NBE, int E, int HS>
int launch_split(StepSplitParams p, int n_emit, hipStream_t s) {
    constexpr int NP = 16 * NBE;
    p.gx = (unsigned)((p.P + NP - 1) / NP); p.gy = (unsigned)(p.Mpad / 64); p.gz = (unsigned)(n_emit / E);
    if ((int64_t)p.gx * p.gy * p.gz >= (1ll << 31)) CSK_FAIL("tcn_step_bf16x3: grid too large");
    void (*kern)(StepSplitParams) = tcn_step_split_kernel<NBE, E, HS>;
    const size_t lds = (size_t)12 * NP * 16;
    if (const int e = csk_ensure_lds((const void *)kern, lds)) return e;
    hipLaunchKernelGGL(kern, dim3(p.gx * p.gy * p.gz), dim3(NTHREADS), lds, s, p);
    return (int)hipGetLastError();
}

// The tile of a launch -- the ONE copy of the rule.  E, emissions per tile: 2 when the launch carries an even number (a staged ring
// slot then serves two taps), else 1; NBE, the tile width in 16-position column blocks (NTU: 25 / 13, Kinetics: 18 / 9), follows the
// launch shape by the cost model of the exact step kernels.  Neither changes an output's summation order.
struct SplitTile { int NBE, E; };
SplitTile split_tile(int n_emit, int Mpad, int64_t P) {
    const int E = n_emit % 2 == 0 ? 2 : 1;
    const int64_t mt = Mpad / 64;
    const int wide = E == 2 ? 13 : 25, narrow = E == 2 ? 9 : 18;
    const double cw = cost_model(((P + 16 * wide - 1) / (16 * wide)) * mt * (n_emit / E), 16.0 * wide * E);
    const double cn = cost_model(((P + 16 * narrow - 1) / (16 * narrow)) * mt * (n_emit / E), 16.0 * narrow * E);
    return {cw <= cn ? wide : narrow, E};
}

}  // namespace

extern "C" int csk_tcn_step_bf16x3(const float *ring, int slots, int head, int head_step, int n_emit, const void *w_split,
                                   const float *x_res, int x_res_slots, int x_res_slot0, int x_res_step,
                                   const void *w_res_split, const float *bias, float *out, int out_slots, int out_slot0,
                                   int c, int c_out, int64_t P, int k, int res_mode, int c_res, int relu, void *stream) {
    const StepCall call = {ring, slots, head, head_step, n_emit, w_split, x_res, x_res_slots, x_res_slot0, x_res_step, w_res_split, bias, out,
                           out_slots, out_slot0, c, c_out, P, k, res_mode, c_res, relu, 1, nullptr};
    const StepParams q = step_params(call);         // for Mpad and the residual ring, stood in for where the call has no x_res
    const int Cres = res_mode != CSK_RES_NONE ? c_res : 1;
    const int rc = step_check("tcn_step_bf16x3", "slots/head", call, true, [&]() -> int {      // (step_params.h) with what only this entry requires
        if (k != 9) CSK_FAIL("tcn_step_bf16x3: the split kernel is built for the 9 x 1 temporal conv (k = %d); use csk_tcn_step_f32", k);
        if (head_step < 1 || head_step > 2) CSK_FAIL("tcn_step_bf16x3: head_step must be 1 or 2 (the stride the weight image was packed for)");
        if (res_mode != CSK_RES_NONE && res_mode != CSK_RES_IDENTITY && res_mode != CSK_RES_CONV) CSK_FAIL("tcn_step_bf16x3: bad res_mode");
        if ((uintptr_t)out & 15) CSK_FAIL("tcn_step_bf16x3: state pointers must be 16-byte aligned");
        if (((uintptr_t)w_split | (uintptr_t)w_res_split) & 15) CSK_FAIL("tcn_step_bf16x3: packed weights must be 16-byte aligned");
        if ((int64_t)slots * c * P * 4 >= (1ll << 32) || (int64_t)q.xres_slots * Cres * P * 4 >= (1ll << 32) || (int64_t)out_slots * c_out * P * 4 >= (1ll << 32))
            CSK_FAIL("tcn_step_bf16x3: a ring of 4 GB or more (32-bit byte offsets inside the rings)");
        return 0;
    });
    if (rc) return rc;
    if (res_mode != CSK_RES_NONE && c_res <= 0) CSK_FAIL("tcn_step_bf16x3: bad residual ring geometry");
    StepSplitParams p;
    p.ring = ring; p.w = (const u32x4 *)w_split; p.xres = q.xres; p.wres = (const u32x4 *)w_res_split; p.bias = bias; p.out = out;
    p.C = c; p.nch16 = round_up(c, KS) / KS; p.Cout = c_out; p.Mpad = q.Mpad;
    p.slots = slots; p.head = head; p.head_step = head_step; p.res_mode = res_mode;
    p.Cres = Cres; p.nch16_res = round_up(p.Cres, KS) / KS; p.relu = relu; p.P = P;
    p.xres_slots = q.xres_slots; p.xres_slot0 = q.xres_slot0; p.xres_step = x_res_step; p.out_slots = out_slots; p.out_slot0 = out_slot0;
    const SplitTile t = split_tile(n_emit, p.Mpad, P);
    hipStream_t s = (hipStream_t)stream;
    if (t.E == 1) return t.NBE == 25 ? launch_split<25, 1, 1>(p, n_emit, s) : launch_split<18, 1, 1>(p, n_emit, s);
    if (head_step == 2) return t.NBE == 13 ? launch_split<13, 2, 2>(p, n_emit, s) : launch_split<9, 2, 2>(p, n_emit, s);
    return t.NBE == 13 ? launch_split<13, 2, 1>(p, n_emit, s) : launch_split<9, 2, 1>(p, n_emit, s);
}

extern "C" int csk_tcn_step_bf16x3_tile(int n_emit, int c_out, int64_t P) {
    if (n_emit < 1 || n_emit > 64 || c_out <= 0 || P < 4 || (P & 3)) CSK_FAIL("tcn_step_bf16x3_tile: bad dims");
    return split_tile(n_emit, round_up(c_out, CSK_MT), P).NBE;
}
