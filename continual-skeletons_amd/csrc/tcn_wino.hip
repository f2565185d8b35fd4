// tcn_wino.hip -- the clip temporal conv of the identity-residual blocks (csk_tcn_stage_wino_f32) by Winograd minimal filtering:
// the 9 x 1 conv (stride 1, pad 4) as three 3-tap groups, each computed with F(2, 3) -- two output frames from four input frames,
// interpolation points 0, 1, -1, inf -- and the groups summed in the transformed domain, so that one output transform serves all
// three.  Per output frame pair and channel the matrix pipe runs 12 K-blocks instead of 18: 1.5x fewer fp32 MFMA FLOPs for the
// same conv, all arithmetic still fp32 (no reduced-precision operand anywhere).
//
//   weights (host, fold.pack_conv_weight_wino):  U[4 g + i][c][co] = (G . w[3 g .. 3 g + 2][c][co])[i], fp64, rounded once
//            G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1]
//   input  (per K step, in registers):  d = y[c][2 j + 3 g - 4 .. 2 j + 3 g - 1][v]  ->  (d0 - d2, d1 + d2, d2 - d1, d1 - d3)
//   GEMMs:  M_i[co][(j, v)] = sum_g sum_c U[4 g + i][c][co] * B_{g,i}[c][(j, v)]          four accumulator sets, i = 0..3
//   output (epilogue, lane-local):  out(2 j) = M0 + M1 + M2,  out(2 j + 1) = M1 - M2 - M3;  + bias + identity residual, ReLU
//
// GEMM view: the columns are (output frame pair j, joint v) flattened, V innermost -- the address arithmetic of a stride-2 conv:
// column (j, v) reads raw frame 2 j + s - 4 at LDS offset 2 (j - ja) V + v + s V, s = 0..9 (s = 3 g + f, f = 0..3).  One raw
// activation chunk in LDS serves the 12 (group, point) products; the transform is 4 VALU ops per 8 MFMAs.
// Tiling: 256 threads = 4 waves, workgroup tile 64 output channels x 128 pair columns; a wave owns all 64 channels x 32 pair
// columns per point (2 x 1 MFMA 32x32x2 accumulators per point, 8 in all = 128 registers), two workgroups per CU.
// Second workgroup shape (MW = 2, "tall"): 128 output channels x 64 pair columns, waves 2 x 2 with the same wave tile and the
// same MFMA order per accumulator element, so both shapes give the same bits.  Tiles do not cross sequences, so a sequence of
// 950 pair columns (T = 75, V = 25) issues 1024 columns in wide tiles and 960 in tall ones; the host takes per layer the shape
// that measures faster (wino_pick_mw: stride 2 the tall one, stride 1 the tall one where it saves 1/16 of the columns; the wide
// one where c_out % 128 != 0).  Tall: 12 (13) weight rows x 8 x 128 staged per chunk, 48 (52) prefetch registers per thread,
// up to 256 VGPRs, 60.5 KB (70 KB stride 2) LDS at V = 25.
// K loop: 8-channel chunks as in tcn_stage_kernel (tcn.hip), the next chunk's loads trickled in three thirds in front of the
// three group segments.  Inside a chunk the LDS operands run ahead of the MFMAs in registers (wino_chunk): A fragments two
// MFMA pairs ahead, raw samples half a K step ahead, across the group segments.  The weights stream from the host-transformed
// image, the staging types are those of mfma_core.h.
// T odd: the last pair's second frame (t = T) is computed from zero padding and not stored.
//
// csk_tcn_stage_wino_ext_f32 adds two forms for the blocks the entry above leaves to the direct kernels:
//   form A  stride 1, no residual: the kernel above without the residual load (RES = false).  Offered by the entry; the host
//           layer's blocks keep the direct kernels for this shape (blocks.py: bitwise pin against csk_block_few_channels_f32).
//   form B  stride 2 (pad 4), conv residual or none: with the phase streams e[n] = y[2 n], o[n] = y[2 n + 1]
//              out[t] = sum_{a=0..4} w[2 a] e[t + a - 2] + sum_{a=0..3} w[2 a + 1] o[t + a - 2]
//           a 5-tap and a 4-tap stride-1 conv, cut into four groups for F(2, 3) (same points, accumulator sets and output
//           transform): E0 = even taps a = 0..2 (4 products), E1 = even taps a = 3, 4, O0 = odd taps a = 0, 1, O1 = odd taps
//           a = 2, 3 -- the 2-tap groups have a zero third tap, so their point-inf product is skipped and d3 never read (3
//           products each): 13 K-blocks per output pair and channel instead of 18.  No de-interleaving: in the raw staged row
//           column (pair j, joint v) reads phase sample i of a group at raw frame 4 j - 4 + F + 2 i (F = 0, 6, 1, 5 for E0, E1,
//           O0, O1) -- column stride 4 V, tap stride 2 V.  The 1 x 1 stride-2 conv residual res[t] = wres . x[2 t] runs as extra
//           chunks over x after the main loop, a 1-tap group with d2 := d1: acc0 += wres (d0 - d1), acc1 += wres d1 (d0 = x[4 j],
//           d1 = x[4 j + 2]), which the output transform turns into out(2 j) += wres d0, out(2 j + 1) += wres d1.
//   weights (host, fold.pack_conv_weight_wino_s2): 13 rows E0 (4), E1 (3), O0 (3), O1 (3); the residual streams the direct w_res.
//
// csk_tcn_stage_wino_valid_res_f32: the valid (pad 0) stride-1 form with the 1 x 1 conv residual on the centred shrink, res[u] =
// wres . x[u + 4] -- extra chunks over x behind the main loop that add wres x[2 j + 4] to M0 and wres (-x[2 j + 5]) to M3, which the
// output transform turns into the residual of both frames of the pair (wino_valid_res_chunk; RESCONV of tcn_stage_wino_kernel).
#include <type_traits>

#include "mfma_core.h"
#include "tcn_params.h"

namespace {

constexpr int WMT = 64;        // output channels per wave, and per workgroup tile of the wide shape
constexpr int WNT = 128;       // pair columns per workgroup tile of the wide shape (32 per wave)
constexpr int WTAPS = 12;      // (group, point) products per channel
// Workgroup shapes, MW = waves along the channels: MW = 1 wide, 64 channels x 128 pair columns (waves 1 x 4); MW = 2 tall, 128
// channels x 64 pair columns (waves 2 x 2: wave w owns channel half w / 2, column half w % 2).  A wave's tile and code are the
// same in both, so both give the same bits; the host picks by layer (wino_pick_mw).

// LDS row of one staged channel: the raw frames 2 ja - 4 .. 2 jb + 5 of a tile whose pair columns span pairs ja .. jb
template <int VT, int MW = 1>
constexpr int wino_ldb() { return ((2 * ((WNT / MW + VT - 2) / VT) + 10) * VT + 3) / 4 * 4; }

// Weight staging of a 12-tap chunk of the 64-row tile: 12 * KC * 16 = 1536 f32x4 = 6 per thread; slot u of a thread is tap
// 2 u + tid / 128, channel row (tid / 16) % 8, rows 4 (tid % 16) .. -- the offsets of the slots differ by wave-uniform constants
// (the layout of WStage9x64 in mfma_core.h, all six slots whole)
struct WStage12x64 {
    unsigned goff0, loff0, gstride;
    f32x4 v[6];
    __device__ __forceinline__ void setup(int Cpad, int Mpad, int tid) {
        goff0 = (unsigned)(((tid >> 7) * Cpad + ((tid >> 4) & 7)) * Mpad + (tid & 15) * 4);
        loff0 = (unsigned)(tid * 4);
        gstride = (unsigned)(2 * Cpad * Mpad);
    }
    __device__ __forceinline__ void issue_slot(int u, const float *__restrict__ chunk_base) {
        v[u] = *reinterpret_cast<const f32x4 *>(chunk_base + (size_t)u * gstride + goff0);
    }
    __device__ __forceinline__ void issue(const float *__restrict__ chunk_base) {
#pragma unroll
        for (int u = 0; u < 6; ++u) issue_slot(u, chunk_base);
    }
    // the part of the next chunk's loads issued in front of group segment G
    template <int G>
    __device__ __forceinline__ void issue_part(const float *__restrict__ chunk_base) {
        issue_slot(2 * G, chunk_base);
        issue_slot(2 * G + 1, chunk_base);
    }
    __device__ __forceinline__ void commit(float *__restrict__ Wl) const {
#pragma unroll
        for (int u = 0; u < 6; ++u) *reinterpret_cast<f32x4 *>(Wl + u * (NTHREADS * 4) + loff0) = v[u];
    }
};

// Weight staging of an NT-row chunk of the 128-row tile: NT * KC * 32 f32x4 = NT per thread; slot u of a thread is image row u,
// channel row tid / 32, rows 4 (tid % 32) .. (the layout of WStage9x128 in mfma_core.h).  issue_part<G>: the rows of group G
// (four groups of 4, 3, 3, 3 rows for NT = 13, three of 4 for NT = 12).
template <int NT>
struct WStageNx128 {
    unsigned goff0, loff0, gstride;
    f32x4 v[NT];
    __device__ __forceinline__ void setup(int Cpad, int Mpad, int tid) {
        goff0 = 4u * (unsigned)((tid >> 5) * Mpad + (tid & 31) * 4);          // bytes
        loff0 = (unsigned)(tid * 4);
        gstride = (unsigned)(Cpad * Mpad);
    }
    // wave-uniform row base + one 32-bit per-lane byte offset (ld_lane in mfma_core.h): NT 64-bit per-lane addresses would
    // not fit the register budget
    __device__ __forceinline__ void issue_slot(int u, const float *__restrict__ chunk_base) {
        v[u] = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const char *>(chunk_base + (size_t)u * gstride) + goff0);
    }
    __device__ __forceinline__ void issue(const float *__restrict__ chunk_base) {
#pragma unroll
        for (int u = 0; u < NT; ++u) issue_slot(u, chunk_base);
    }
    template <int G>
    __device__ __forceinline__ void issue_part(const float *__restrict__ chunk_base) {
        constexpr int lo = NT == 13 ? (G == 0 ? 0 : 3 * G + 1) : 4 * G, hi = NT == 13 ? 3 * G + 4 : 4 * G + 4;
#pragma unroll
        for (int u = lo; u < hi; ++u) issue_slot(u, chunk_base);
    }
    __device__ __forceinline__ void commit(float *__restrict__ Wl) const {
#pragma unroll
        for (int u = 0; u < NT; ++u) *reinterpret_cast<f32x4 *>(Wl + u * (KC * 128) + loff0) = v[u];
    }
};

// Residual weights: one 8-channel chunk of the direct w_res image for the 64-row tile = 128 f32x4, one per thread of the lower
// half; the upper half repeats it (same value to the same address)
struct WStageRes64 {
    unsigned goff0, loff0;
    f32x4 v;
    __device__ __forceinline__ void setup(int Mpad, int tid) {
        goff0 = (unsigned)(((tid >> 4) & 7) * Mpad + (tid & 15) * 4);
        loff0 = (unsigned)((tid & 127) * 4);
    }
    __device__ __forceinline__ void issue(const float *__restrict__ chunk_base) {
        v = *reinterpret_cast<const f32x4 *>(chunk_base + goff0);
    }
    __device__ __forceinline__ void commit(float *__restrict__ Wl) const { *reinterpret_cast<f32x4 *>(Wl + loff0) = v; }
};

// The same for the 128-row tile: 256 f32x4, one per thread (channel row tid / 32, rows 4 (tid % 32) ..)
struct WStageRes128 {
    unsigned goff0, loff0;
    f32x4 v;
    __device__ __forceinline__ void setup(int Mpad, int tid) {
        goff0 = (unsigned)((tid >> 5) * Mpad + (tid & 31) * 4);
        loff0 = (unsigned)(tid * 4);
    }
    __device__ __forceinline__ void issue(const float *__restrict__ chunk_base) {
        v = *reinterpret_cast<const f32x4 *>(chunk_base + goff0);
    }
    __device__ __forceinline__ void commit(float *__restrict__ Wl) const { *reinterpret_cast<f32x4 *>(Wl + loff0) = v; }
};

// The groups of a chunk: image row of a group's first point, raw frame of its first sample (samples FS frames apart), its points
// (= the samples it reads: a 3-point group has a zero third tap and no d3), and which sample of the group in front is this
// group's d0 (-1: none) -- that frame is read once and kept in a register from one group to the next.
struct WinoGroupsS1 {          // stride 1: three 3-tap groups, sample f of group g at raw frame 3 g + f; 10 distinct frames
    static constexpr int NG = 3, FS = 1;
    static constexpr int row0(int g) { return 4 * g; }
    static constexpr int frame0(int g) { return 3 * g; }
    static constexpr int np(int) { return 4; }
    static constexpr int carry(int g) { return g > 0 ? 3 : -1; }
};
struct WinoGroupsS2 {          // stride 2: E0, E1, O0, O1 (form B of the header comment); 11 distinct frames
    static constexpr int NG = 4, FS = 2;
    static constexpr int row0(int g) { return g == 0 ? 0 : 3 * g + 1; }
    static constexpr int frame0(int g) { return g == 0 ? 0 : g == 1 ? 6 : g == 2 ? 1 : 5; }
    static constexpr int np(int g) { return g == 0 ? 4 : 3; }
    static constexpr int carry(int g) { return g == 1 ? 3 : g == 3 ? 2 : -1; }
};

template <int G>
using group_c = std::integral_constant<int, G>;

// One chunk for one wave, all groups: acc[i][mi] += U[row0(g) + i][kk][rows mi] x B_{g,i}[kk][this lane's column], groups in
// ascending order, K steps s = 0 .. KC / 2 - 1 inside a group, points inside a step -- the order per accumulator element that
// both workgroup shapes share.  (Wl: the staged weights at this wave's first row; MT = rows of the staged tile.)
// Operands run ahead in registers: the A fragments AD MFMA pairs ahead of their own pair (1 <= AD <= 3; pairs counted through
// the steps of the chunk), the raw samples of step (g, s) + 1 from the middle of step (g, s), across the group boundary too --
// between(group_c<g + 1>) (the loads of the next chunk that go in front of group g + 1, between s_setprio 0 / 1) is called
// behind the last MFMA of group g with the first operands of group g + 1 already on their way.  Only the chunk's first pairs
// wait for LDS.  CARRY: a frame that two neighbouring groups share is read once (10 instead of 12 reads per K step at stride
// 1, 11 instead of 13 at stride 2) at the price of KC / 2 registers across the group boundary.
template <class GR, int VT, int LDB, int MT, int AD, bool CARRY, class Between>
__device__ __forceinline__ void wino_chunk(const float *__restrict__ Wl, const float *__restrict__ Bl, int off, int l31, int kh,
                                           f32x16 (&acc)[4][2], Between between) {
    static_assert(AD >= 1 && AD <= 3, "a pair's fragment is read inside its own step or the one in front");
    constexpr int NS = KC / 2, NSTEP = GR::NG * NS;
    const float *br = Bl + kh * LDB + off;
    const float *wr = Wl + kh * MT + l31;
    float d[NSTEP][4], a[NSTEP][4][2], keep[NS];       // every index is a constant once unrolled: registers, live only briefly
    auto read_d = [&](int t) {
        const int g = t / NS, s = t % NS;
        const float *p = br + 2 * s * LDB + GR::frame0(g) * VT;
#pragma unroll
        for (int f = 0; f < 4; ++f)
            d[t][f] = CARRY && f == 0 && GR::carry(g) >= 0 ? keep[s] : f < GR::np(g) ? p[f * GR::FS * VT] : 0.f;
        if (CARRY && g + 1 < GR::NG && GR::carry(g + 1) >= 0) keep[s] = d[t][GR::carry(g + 1)];
    };
    // the A pair that stands j pairs behind pair 0 of step t (in its own step or the next one)
    auto read_a = [&](int t, int j) {
        const int n = GR::np(t / NS), tt = j < n ? t : t + 1, i = j < n ? j : j - n;
        if (tt < NSTEP) {
            const float *p = wr + (GR::row0(tt / NS) + i) * (KC * MT) + 2 * (tt % NS) * MT;
            a[tt][i][0] = p[0];
            a[tt][i][1] = p[32];
        }
    };
    read_d(0);
#pragma unroll
    for (int j = 0; j < AD; ++j) read_a(0, j);
#pragma unroll
    for (int t = 0; t < NSTEP; ++t) {
        const int g = t / NS;
        // A step is a scheduling region of its own, its order pinned (left to itself the scheduler sinks every read back in
        // front of its MFMA pair, and hoists the next step's transform up to the reads it then waits for): the transform of
        // samples read half a step ago; behind each MFMA pair one ds_read2 for the pair AD further on, behind the second pair
        // also the next step's samples (one or two instructions).  The chunk's first reads stand in front of its first step.
        if (t > 0) __builtin_amdgcn_sched_barrier(0);
        const float b[4] = {d[t][0] - d[t][2], d[t][1] + d[t][2], d[t][2] - d[t][1], d[t][1] - d[t][3]};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < GR::np(g)) {
                acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][i][0], b[i], acc[i][0], 0, 0, 0);
                acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][i][1], b[i], acc[i][1], 0, 0, 0);
                read_a(t, i + AD);
                if (i == 1 && t + 1 < NSTEP) read_d(t + 1);
            }
        }
        if (t == 0) __builtin_amdgcn_sched_group_barrier(0x100, AD + 2, 0);
#pragma unroll
        for (int i = 0; i < GR::np(g); ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            if (i == 1) __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
            else __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        if (t + 1 < NSTEP && (t + 1) % NS == 0) {
            if (g == 0) between(group_c<1>{});
            else if (g == 1) between(group_c<2>{});
            else if constexpr (GR::NG > 3) between(group_c<3>{});
        }
    }
}

// One chunk of a 1 x 1 conv residual for one wave: per K step two samples d0, d1 of the lane's column (FS frames apart) and one
// A pair; SIGN-transformed into two accumulator sets (below).  Operands one step ahead, as in wino_chunk.
template <int VT, int LDB, int MT, int FS, class Products>
__device__ __forceinline__ void wino_res_steps(const float *__restrict__ Wl, const float *__restrict__ Bl, int off, int l31, int kh,
                                               Products products) {
    constexpr int NS = KC / 2;
    const float *br = Bl + kh * LDB + off;
    const float *wr = Wl + kh * MT + l31;
    float d[2][2], a[2][2];
    auto read = [&](int s, float (&dd)[2], float (&aa)[2]) {
        dd[0] = br[2 * s * LDB];
        dd[1] = br[2 * s * LDB + FS * VT];
        aa[0] = wr[2 * s * MT];
        aa[1] = wr[2 * s * MT + 32];
    };
    read(0, d[0], a[0]);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s + 1 < NS) read(s + 1, d[(s + 1) & 1], a[(s + 1) & 1]);
        products(a[s & 1][0], a[s & 1][1], d[s & 1][0], d[s & 1][1]);
    }
}

// One chunk of the valid form's conv residual res[u] = w_res . x[u + 4]: the staged row starts at raw frame 2 ja + 4 of x, so the
// lane's column reads d0 = x[2 j + 4] and d1 = x[2 j + 5].  No accumulator set of its own: acc0 += w_res d0 and acc3 += w_res (-d1),
// which the output transform out(2 j) = M0 + M1 + M2, out(2 j + 1) = M1 - M2 - M3 turns into out(2 j) += w_res d0 and
// out(2 j + 1) += w_res d1.  The sign sits in the staged operand: the weights are the direct w_res image as it is.
template <int VT, int MW>
__device__ __forceinline__ void wino_valid_res_chunk(const float *__restrict__ Wl, const float *__restrict__ Bl, int off, int l31,
                                                     int kh, f32x16 (&acc)[4][2]) {
    wino_res_steps<VT, wino_ldb<VT, MW>(), WMT * MW, 1>(Wl, Bl, off, l31, kh, [&](float a0, float a1, float d0, float d1) {
        const float nd1 = -d1;
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, d0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, d0, acc[0][1], 0, 0, 0);
        acc[3][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, nd1, acc[3][0], 0, 0, 0);
        acc[3][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, nd1, acc[3][1], 0, 0, 0);
    });
}

// ---- epilogue: output transform, + bias (+ identity residual, RES), ReLU.  C/D map: column = lane & 31 (this lane's pair column),
// row = (g & 3) + 8 (g >> 2) + 4 (lane >> 5).  Row base pointers are wave-uniform (64-bit); a lane adds one 32-bit byte offset
// (4 kh rows + its position; T V < 2^26 keeps it below 2^32).  Every wave has all 64 rows (c_out a multiple of the tile's rows,
// host gate).  p.Tout = output frames; m0 = the wave's first row, wn = its column quarter / half; (jc, vc) = this lane's pair column.
// VALID (csk_tcn_stage_wino_valid_f32): the output has p.Tout = p.Tin - 8 frames, the residual is the block input of p.Tin
// frames read 4 frames further on (the centred shrink) -- its own row length and lane offsets.
template <int VT, bool RES, bool VALID = false>
__device__ __forceinline__ void wino_epilogue(const TcnParams &p, const f32x16 (&acc)[4][2], int m0, int q0, int qend, int seg,
                                              int wn, int l31, int kh, int jc, int vc) {
    const int T = p.Tout, TV = T * VT;
    const int TVR = VALID ? p.Tin * VT : TV;                         // row length of the residual
    const bool qv = q0 + wn * 32 + l31 < qend;
    const bool odd_ok = 2 * jc + 1 < T;                              // the pair's second frame exists (T odd: not the last pair)
    const unsigned p0 = (unsigned)(2 * jc * VT + vc);
    const unsigned b0 = 4u * (4u * (unsigned)kh * (unsigned)TV + p0);
    const unsigned b1 = odd_ok ? b0 + 4u * VT : b0;                  // phantom frame: re-read frame 2 j (value unused)
    const unsigned kh16 = 16u * (unsigned)kh;
    const unsigned r0 = VALID ? 4u * (4u * (unsigned)kh * (unsigned)TVR + p0 + 4u * VT) : b0;
    const unsigned r1 = VALID ? (odd_ok ? r0 + 4u * VT : r0) : b1;
    const float *rseg = RES ? p.xres + (int64_t)seg * p.Cout * TVR : nullptr;
    float *oseg = p.out + (int64_t)seg * p.Cout * TV;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        const int rb = m0 + mi * 32;
        float o0[16], o1[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = rb + (g & 3) + 8 * (g >> 2);
            const float bias = ld_lane(p.bias + row, kh16);
            const float m1 = acc[1][mi][g], m2 = acc[2][mi][g];
            float v0 = acc[0][mi][g] + m1 + m2 + bias;
            float v1 = m1 - m2 - acc[3][mi][g] + bias;
            if (RES) {
                const float *rrow = rseg + (int64_t)row * TVR;
                v0 += ld_lane(rrow, r0);
                v1 += ld_lane(rrow, r1);
            }
            if (p.relu) { v0 = relu_nan(v0); v1 = relu_nan(v1); }
            o0[g] = v0;
            o1[g] = v1;
        }
        if (qv) {
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                float *orow = oseg + (int64_t)(rb + (g & 3) + 8 * (g >> 2)) * TV;
                st_lane(orow, b0, o0[g]);
                if (odd_ok) st_lane(orow, b1, o1[g]);
            }
        }
    }
}

}  // namespace

// p.Tout = T (frames in and out), p.nt = pair columns per segment ((T + 1) / 2 * V), p.w = the transformed weight image.
// VALID: the unpadded conv (pad 0) -- the padded conv's output frames [4, T - 4) stored at t - 4.  Pair column (j, v) is the
// padded form's pair j + 2, so it reads the raw frames 2 j .. 2 j + 9 (the staged span starts at frame 2 ja instead of 2 ja - 4)
// and stores the frames 2 j, 2 j + 1 of an output of p.Tout = p.Tin - 8 frames; p.nt = (p.Tout + 1) / 2 * V.  Same products in the
// same order per accumulator element: bit for bit the padded form's frames.
// RESCONV (VALID only, csk_tcn_stage_wino_valid_res_f32): the 1 x 1 conv residual on the centred shrink, res[u] = p.wres . p.xres[u + 4]
// (p.xres: p.Cres channels, a multiple of 16, x p.Tres == p.Tin frames), as a second K phase behind the main loop.
template <int VT, bool RES = true, int MW = 1, bool VALID = false, bool RESCONV = false>
__global__ __launch_bounds__(NTHREADS, 2) void tcn_stage_wino_kernel(const TcnParams p) {
    static_assert(!RESCONV || (VALID && !RES), "the conv-residual phase is built for the valid form");
    constexpr int LDB = wino_ldb<VT, MW>(), MT = WMT * MW, NT = WNT / MW;
    constexpr int NJ = (LDB + 63) / 64;
    constexpr int AD = 2;                  // wino_chunk: A fragments two MFMA pairs ahead (three would spill in the tall shape)
    constexpr bool CARRY = true;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *Wl = smem;
    float *Bl = smem + WTAPS * KC * MT;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kh = lane >> 5;
    const int wm = MW == 2 ? wave >> 1 : 0, wn = MW == 2 ? wave & 1 : wave;     // this wave's channel half / column part
    // work item -> (m-tile fastest: shares the activation tile; then column tile; then segment)
    const unsigned wid = xcd_contiguous_id(blockIdx.x, gridDim.x);
    const int m0 = (int)(wid % p.mtiles) * MT, q0 = (int)((wid / p.mtiles) % p.qtiles) * NT;
    const int seg = (int)(wid / (p.mtiles * p.qtiles));
    const int T = VALID ? p.Tin : p.Tout, TV = T * VT, QP = p.nt;    // T: input frames
    const int qend = min(q0 + NT, QP);
    const int ja = div_magic(q0, p.vmagic), jb = div_magic(qend - 1, p.vmagic);

    // this lane's pair column (clamped into the tile; lanes past its end compute a copy of the last column and store nothing)
    const int qc = min(q0 + wn * 32 + l31, qend - 1);
    const int jc = div_magic(qc, p.vmagic), vc = qc - jc * VT;
    const int off = 2 * (jc - ja) * VT + vc;

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[i][mi][g] = 0.f;

    {
        const int fa = VALID ? 2 * ja : 2 * ja - 4;                  // first raw frame of the tile (pad 4; VALID: pad 0)
        const int span = (2 * (jb - ja) + 10) * VT;
        const int64_t cs = (int64_t)TV;
        const float *seg_base = p.y + (int64_t)seg * p.C * cs;       // 64-bit segment base; 32-bit offsets inside it
        const float *wbase = p.w + m0;
        const float *Ww = Wl + wm * WMT;                             // this wave's rows of the staged weights
        std::conditional_t<MW == 2, WStageNx128<WTAPS>, WStage12x64> ws;
        ws.setup(p.Cpad, p.Mpad, tid);
        auto kloop = [&](auto &bx) {
            ws.issue(wbase);
            bx.issue(seg_base, p.C, cs, 0, wave);
            for (int c0 = 0; c0 + KC < p.Cpad; c0 += KC) {
                __syncthreads();                     // previous chunk's LDS reads are done
                ws.commit(Wl);
                bx.commit(Bl, LDB, wave);
                __syncthreads();
                const float *wnext = wbase + (size_t)(c0 + KC) * p.Mpad;
                const int cn = c0 + KC;
                ws.template issue_part<0>(wnext);
                bx.template issue_third<0>(seg_base, p.C, cs, cn, wave);
                __builtin_amdgcn_s_setprio(1);
                wino_chunk<WinoGroupsS1, VT, LDB, MT, AD, CARRY>(Ww, Bl, off, l31, kh, acc, [&](auto g) {
                    __builtin_amdgcn_s_setprio(0);
                    ws.template issue_part<g()>(wnext);
                    bx.template issue_third<g()>(seg_base, p.C, cs, cn, wave);
                    __builtin_amdgcn_s_setprio(1);
                });
                __builtin_amdgcn_s_setprio(0);
            }
            __syncthreads();                         // peeled last chunk
            ws.commit(Wl);
            bx.commit(Bl, LDB, wave);
            __syncthreads();
            wino_chunk<WinoGroupsS1, VT, LDB, MT, AD, CARRY>(Ww, Bl, off, l31, kh, acc, [](auto) {});
        };
        // tiles whose staged span lies inside the sequence: 16-byte staging; the others (zero padding at either end) element-wise
        const bool interior = fa >= 0 && fa * VT + 4 * ((span + 3) / 4) <= TV;     // uniform
        if (interior) {
            BStage4<(NJ + 3) / 4> b4;
            b4.setup(fa * VT, span, lane);
            kloop(b4);
        } else {
            BStage<NJ> bs;
            bs.setup(fa * VT, span, TV, lane);
            kloop(bs);
        }
    }

    if (RESCONV) {
        // conv residual: 8-channel chunks of x, frames 2 ja + 4 .. 2 jb + 5 -- inside the sequence for every tile (the last pair's
        // second frame is at most frame Tin - 4), so 16-byte staging throughout; the next chunk's loads are issued in front of the
        // current chunk's products
        constexpr int NJ4R = (((2 * ((NT + VT - 2) / VT) + 2) * VT + 3) / 4 + 63) / 64;
        const int span = (2 * (jb - ja) + 2) * VT;
        const int64_t cs = (int64_t)p.Tres * VT;
        const float *seg_base = p.xres + (int64_t)seg * p.Cres * cs;
        const float *wbase = p.wres + m0;
        const float *Ww = Wl + wm * WMT;                             // this wave's rows of the staged weights
        std::conditional_t<MW == 2, WStageRes128, WStageRes64> wr;
        wr.setup(p.Mpad, tid);
        BStage4<NJ4R> b4;
        b4.setup((2 * ja + 4) * VT, span, lane);
        wr.issue(wbase);
        b4.issue(seg_base, p.Cres, cs, 0, wave);
        for (int c0 = 0; c0 + KC < p.Cres; c0 += KC) {
            __syncthreads();
            wr.commit(Wl);
            b4.commit(Bl, LDB, wave);
            __syncthreads();
            wr.issue(wbase + (size_t)(c0 + KC) * p.Mpad);
            b4.issue(seg_base, p.Cres, cs, c0 + KC, wave);
            wino_valid_res_chunk<VT, MW>(Ww, Bl, off, l31, kh, acc);
        }
        __syncthreads();
        wr.commit(Wl);
        b4.commit(Bl, LDB, wave);
        __syncthreads();
        wino_valid_res_chunk<VT, MW>(Ww, Bl, off, l31, kh, acc);
    }

    wino_epilogue<VT, RES, VALID>(p, acc, m0 + wm * WMT, q0, qend, seg, wn, l31, kh, jc, vc);
}

// ------------------------------------------------------------------------------------------------
// form B: stride 2 by polyphase F(2, 3) groups (header comment)
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int W2TAPS = 13;     // (group, point) products per channel: E0 4, E1 3, O0 3, O1 3

// LDS row of one staged channel: the raw frames 4 ja - 4 .. 4 jb + 6 of a tile whose pair columns span pairs ja .. jb
template <int VT, int MW = 1>
constexpr int wino2_ldb() { return ((4 * ((WNT / MW + VT - 2) / VT) + 11) * VT + 3) / 4 * 4; }

// Weight staging of a 13-row chunk of the 64-row tile: 13 * KC * 16 = 1664 f32x4 = 6.5 per thread; slot u of a thread is image
// row 2 u + tid / 128 (WStage12x64); the upper half of the threads has no slot 6 and repeats its slot 5 (same value to the
// same address, as WStage9x64 does)
struct WStage13x64 {
    unsigned goff0, loff0, gstride, u6;
    f32x4 v[7];
    __device__ __forceinline__ void setup(int Cpad, int Mpad, int tid) {
        goff0 = (unsigned)(((tid >> 7) * Cpad + ((tid >> 4) & 7)) * Mpad + (tid & 15) * 4);
        loff0 = (unsigned)(tid * 4);
        gstride = (unsigned)(2 * Cpad * Mpad);
        u6 = tid >= 128 ? 5u : 6u;
    }
    __device__ __forceinline__ void issue_slot(int u, const float *__restrict__ chunk_base) {
        if (u < 6) v[u] = *reinterpret_cast<const f32x4 *>(chunk_base + (size_t)u * gstride + goff0);
        else v[6] = *reinterpret_cast<const f32x4 *>(chunk_base + (size_t)u6 * gstride + goff0);
    }
    __device__ __forceinline__ void issue(const float *__restrict__ chunk_base) {
#pragma unroll
        for (int u = 0; u < 7; ++u) issue_slot(u, chunk_base);
    }
    template <int G>
    __device__ __forceinline__ void issue_part(const float *__restrict__ chunk_base) {
        if (G < 3) {
            issue_slot(2 * G, chunk_base);
            issue_slot(2 * G + 1, chunk_base);
        } else {
            issue_slot(6, chunk_base);
        }
    }
    __device__ __forceinline__ void commit(float *__restrict__ Wl) const {
#pragma unroll
        for (int u = 0; u < 6; ++u) *reinterpret_cast<f32x4 *>(Wl + u * (NTHREADS * 4) + loff0) = v[u];
        *reinterpret_cast<f32x4 *>(Wl + u6 * (NTHREADS * 4) + loff0) = v[6];
    }
};

// BStage4 (mfma_core.h) for the tall shape, whose weight stage holds 13 registers-of-four per thread: a row of LDB floats as NV
// whole 16-byte sweeps (256 floats each) and, where the rest is short, NS 4-byte sweeps (64 floats each) in place of one more
// 16-byte sweep that three quarters of the lanes would only repeat.  One offset per sweep serves the global and the LDS side
// (the tile's first position goes into the wave-uniform row base).
template <int LDB>
struct BStage4Tail {
    static constexpr int RPW = KC / (NTHREADS / 64);   // rows per wave
    static constexpr int REST = LDB % 256;
    static constexpr int NV = LDB / 256 + (REST > 128 ? 1 : 0), NS = REST > 128 ? 0 : (REST + 63) / 64;
    static_assert(NV >= 1 && NV <= 2 && NS <= 2, "issue_third: 16-byte sweeps with thirds 0 and 1, 4-byte sweeps with third 2");
    unsigned off4[NV], off1[NS > 0 ? NS : 1];
    int pbase_;
    f32x4 v[RPW][NV];
    float t[RPW][NS > 0 ? NS : 1];
    __device__ __forceinline__ void setup(int pbase, int span, int lane) {
        const int nvec = (span + 3) / 4;
        pbase_ = pbase;
#pragma unroll
        for (int u = 0; u < NV; ++u) off4[u] = (unsigned)(4 * min(u * 64 + lane, nvec - 1));
#pragma unroll
        for (int u = 0; u < NS; ++u) off1[u] = (unsigned)min(NV * 256 + u * 64 + lane, span - 1);
    }
    __device__ __forceinline__ const float *row(const float *__restrict__ seg_base, int C, int64_t chan_stride, int c0, int wave,
                                                int rr) const {
        const int c = min(c0 + wave + rr * (NTHREADS / 64), C - 1);         // clamped: padding channels carry zero weights
        return seg_base + (int64_t)c * chan_stride + pbase_;
    }
    template <int G>
    __device__ __forceinline__ void issue_third(const float *__restrict__ seg_base, int C, int64_t chan_stride, int c0, int wave) {
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const float *src = row(seg_base, C, chan_stride, c0, wave, rr);
            if (G < NV) v[rr][G < NV ? G : 0] = *reinterpret_cast<const f32x4u *>(src + off4[G < NV ? G : 0]);
            if (G == 2) {
#pragma unroll
                for (int u = 0; u < NS; ++u) t[rr][u] = src[off1[u]];
            }
        }
    }
    __device__ __forceinline__ void issue(const float *__restrict__ seg_base, int C, int64_t chan_stride, int c0, int wave) {
        issue_third<0>(seg_base, C, chan_stride, c0, wave);
        issue_third<1>(seg_base, C, chan_stride, c0, wave);
        issue_third<2>(seg_base, C, chan_stride, c0, wave);
    }
    __device__ __forceinline__ void commit(float *__restrict__ Bl, int ldb, int wave) const {
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            float *dst = Bl + (wave + rr * (NTHREADS / 64)) * ldb;
#pragma unroll
            for (int u = 0; u < NV; ++u) *reinterpret_cast<f32x4 *>(dst + off4[u]) = v[rr][u];
#pragma unroll
            for (int u = 0; u < NS; ++u) dst[off1[u]] = t[rr][u];
        }
    }
};

// One residual chunk: the staged row starts at raw frame 4 ja of x; d0 = x[4 j], d1 = x[4 j + 2]
template <int VT, int MW>
__device__ __forceinline__ void wino2_res_chunk(const float *__restrict__ Wl, const float *__restrict__ Bl, int off, int l31, int kh,
                                                f32x16 (&acc)[4][2]) {
    wino_res_steps<VT, wino2_ldb<VT, MW>(), WMT * MW, 2>(Wl, Bl, off, l31, kh, [&](float a0, float a1, float d0, float d1) {
        const float b0 = d0 - d1;
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, d1, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, d1, acc[1][1], 0, 0, 0);
    });
}

}  // namespace

// p.Tin = input frames, p.Tout = output frames ((Tin - 1) / 2 + 1), p.nt = pair columns per segment ((Tout + 1) / 2 * V),
// p.w = the 13-row image, p.wres / p.xres = direct residual image and block input (RESCONV) with p.Tres == p.Tin
template <int VT, bool RESCONV, int MW = 1>
__global__ __launch_bounds__(NTHREADS, 2) void tcn_stage_wino_s2_kernel(const TcnParams p) {
    constexpr int LDB = wino2_ldb<VT, MW>(), MT = WMT * MW, NT = WNT / MW;
    constexpr int NJ = (LDB + 63) / 64;
    constexpr int AD = 2;                  // wino_chunk: A fragments two MFMA pairs ahead (three would spill in the tall shape)
    constexpr bool CARRY = true;
    constexpr int NJR = ((4 * ((NT + VT - 2) / VT) + 3) * VT + 63) / 64;      // residual rows: raw frames 4 ja .. 4 jb + 2
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *Wl = smem;
    float *Bl = smem + W2TAPS * KC * MT;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kh = lane >> 5;
    const int wm = MW == 2 ? wave >> 1 : 0, wn = MW == 2 ? wave & 1 : wave;     // this wave's channel half / column part
    const unsigned wid = xcd_contiguous_id(blockIdx.x, gridDim.x);
    const int m0 = (int)(wid % p.mtiles) * MT, q0 = (int)((wid / p.mtiles) % p.qtiles) * NT;
    const int seg = (int)(wid / (p.mtiles * p.qtiles));
    const int TVin = p.Tin * VT, QP = p.nt;
    const int qend = min(q0 + NT, QP);
    const int ja = div_magic(q0, p.vmagic), jb = div_magic(qend - 1, p.vmagic);
    const float *Ww = Wl + wm * WMT;                                 // this wave's rows of the staged weights

    // this lane's pair column (clamped into the tile; lanes past its end compute a copy of the last column and store nothing)
    const int qc = min(q0 + wn * 32 + l31, qend - 1);
    const int jc = div_magic(qc, p.vmagic), vc = qc - jc * VT;
    const int off = 4 * (jc - ja) * VT + vc;

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[i][mi][g] = 0.f;

    {
        const int fa = 4 * ja - 4;                                   // first raw frame of the tile (pad 4)
        const int span = (4 * (jb - ja) + 11) * VT;
        const int64_t cs = (int64_t)TVin;
        const float *seg_base = p.y + (int64_t)seg * p.C * cs;       // 64-bit segment base; 32-bit offsets inside it
        const float *wbase = p.w + m0;
        std::conditional_t<MW == 2, WStageNx128<W2TAPS>, WStage13x64> ws;
        ws.setup(p.Cpad, p.Mpad, tid);
        auto kloop = [&](auto &bx) {
            ws.issue(wbase);
            bx.issue(seg_base, p.C, cs, 0, wave);
            for (int c0 = 0; c0 + KC < p.Cpad; c0 += KC) {
                __syncthreads();                     // previous chunk's LDS reads are done
                ws.commit(Wl);
                bx.commit(Bl, LDB, wave);
                __syncthreads();
                const float *wnext = wbase + (size_t)(c0 + KC) * p.Mpad;
                const int cn = c0 + KC;
                ws.template issue_part<0>(wnext);
                bx.template issue_third<0>(seg_base, p.C, cs, cn, wave);
                __builtin_amdgcn_s_setprio(1);
                wino_chunk<WinoGroupsS2, VT, LDB, MT, AD, CARRY>(Ww, Bl, off, l31, kh, acc, [&](auto g) {
                    __builtin_amdgcn_s_setprio(0);
                    ws.template issue_part<g()>(wnext);
                    if constexpr (g() < 3) bx.template issue_third<g()>(seg_base, p.C, cs, cn, wave);
                    __builtin_amdgcn_s_setprio(1);
                });
                __builtin_amdgcn_s_setprio(0);
            }
            __syncthreads();                         // peeled last chunk
            ws.commit(Wl);
            bx.commit(Bl, LDB, wave);
            __syncthreads();
            wino_chunk<WinoGroupsS2, VT, LDB, MT, AD, CARRY>(Ww, Bl, off, l31, kh, acc, [](auto) {});
        };
        // tiles whose staged span lies inside the sequence: 16-byte staging; the others (zero padding at either end) element-wise
        const bool interior = fa >= 0 && fa * VT + 4 * ((span + 3) / 4) <= TVin;   // uniform
        if (interior) {
            std::conditional_t<MW == 2, BStage4Tail<LDB>, BStage4<(NJ + 3) / 4>> b4;
            b4.setup(fa * VT, span, lane);
            kloop(b4);
        } else {
            BStage<NJ> bs;
            bs.setup(fa * VT, span, TVin, lane);
            kloop(bs);
        }
    }

    if (RESCONV) {
        // conv residual: 8-channel chunks of x (element-wise staging: frames past the end read as zero), the next chunk's
        // loads issued in front of the current chunk's products
        const int span = (4 * (jb - ja) + 3) * VT;
        const int64_t cs = (int64_t)p.Tres * VT;
        const float *seg_base = p.xres + (int64_t)seg * p.Cres * cs;
        const float *wbase = p.wres + m0;
        const int cend = (p.Cres + KC - 1) / KC * KC;                // <= CresPad: rows of the image
        std::conditional_t<MW == 2, WStageRes128, WStageRes64> wr;
        wr.setup(p.Mpad, tid);
        BStage<NJR> bs;
        bs.setup(4 * ja * VT, span, p.Tres * VT, lane);
        wr.issue(wbase);
        bs.issue(seg_base, p.Cres, cs, 0, wave);
        for (int c0 = 0; c0 + KC < cend; c0 += KC) {
            __syncthreads();
            wr.commit(Wl);
            bs.commit(Bl, LDB, wave);
            __syncthreads();
            wr.issue(wbase + (size_t)(c0 + KC) * p.Mpad);
            bs.issue(seg_base, p.Cres, cs, c0 + KC, wave);
            wino2_res_chunk<VT, MW>(Ww, Bl, off, l31, kh, acc);
        }
        __syncthreads();
        wr.commit(Wl);
        bs.commit(Bl, LDB, wave);
        __syncthreads();
        wino2_res_chunk<VT, MW>(Ww, Bl, off, l31, kh, acc);
    }

    wino_epilogue<VT, false>(p, acc, m0 + wm * WMT, q0, qend, seg, wn, l31, kh, jc, vc);
}

// Workgroup shape of a launch with qp pair columns per sequence -- a function of the layer alone, never of the batch.  Both
// shapes need c_out a multiple of their rows, so the tall one never issues more columns x rows than the wide one.  Measured at
// batch 256 (profiles/HISTORY.md round 16): at equal issued columns the tall stride-2 kernel is 2 % faster than the wide one (it
// stages less per chunk), the tall stride-1 kernel 2 - 5 % slower (twice the weight traffic per column).  So stride 2 takes the
// tall shape wherever c_out allows it, stride 1 where it issues at least 1/16 fewer columns (T = 75: 960 against 1024 at V = 25,
// 704 against 768 at V = 18; not T = 300: 3776 against 3840, measured 2 % slower).
// CSK_TCN_WINO=2 / =3 (diagnostic, under CSK_DIAG) takes the wide / the tall shape wherever c_out allows both.
static int wino_pick_mw(int qp, int c_out, int stride) {
    if (c_out % (2 * WMT) != 0) return 1;
    const int force = csk_diag_int("CSK_TCN_WINO");
    if (force == 2 || force == 3) return force - 1;
    if (stride == 2) return 2;
    const int64_t wide = round_up(qp, WNT), tall = round_up(qp, WNT / 2);
    return 16 * tall <= 15 * wide ? 2 : 1;
}

// The forms of the Winograd kernels: the 9-tap conv each computes and the residuals it takes with it.  Everything else -- V, the
// channel counts, the workgroup shape, the LDS tile, the launch -- is common to them (tcn_stage_wino_launch).
enum WinoFormId { WINO_PADDED_IDENT, WINO_PADDED_NONE, WINO_VALID, WINO_VALID_RES, WINO_S2 };
struct WinoForm {
    int stride, pad, t_min;   // the conv, and the fewest input frames the form takes
    unsigned res_modes;       // bit m: residual mode m (CSK_RES_*) is a shape of the form
    int res_off;              // a residual is read from this frame of x_res on (t_res == t_in frames, always)
    int none_off;             // the res_off a call WITHOUT residual must come with; -1: any, it is not read
    int cres_unit;            // conv residual: c_res a positive multiple of this (16: whole chunks of the direct w_res image)
};
constexpr unsigned WR_NONE = 1u << CSK_RES_NONE, WR_IDENT = 1u << CSK_RES_IDENTITY, WR_CONV = 1u << CSK_RES_CONV;
constexpr WinoForm WINO_FORMS[] = {
    /* WINO_PADDED_IDENT csk_tcn_stage_wino_f32               */ {1, 4, 1, WR_IDENT, 0, -1, 0},
    /* WINO_PADDED_NONE  csk_tcn_stage_wino_ext_f32, form A   */ {1, 4, 1, WR_NONE, 0, -1, 0},
    /* WINO_VALID        csk_tcn_stage_wino_valid_f32         */ {1, 0, 9, WR_IDENT | WR_NONE, 4, -1, 0},
    /* WINO_VALID_RES    csk_tcn_stage_wino_valid_res_f32     */ {1, 0, 9, WR_CONV, 4, -1, 16},
    /* WINO_S2           csk_tcn_stage_wino_ext_f32, form B   */ {2, 4, 1, WR_CONV | WR_NONE, 0, 0, 1},
};

// the kernel of (V, MW, form, residual), its LDS row and its (group, point) products per channel: every instantiation that exists
struct WinoKernel {
    void (*kern)(TcnParams);
    int ldb, taps;
};
template <int VT, int MW>
static WinoKernel wino_kernel_of(WinoFormId form, int res_mode) {
    const bool ident = res_mode == CSK_RES_IDENTITY, conv = res_mode == CSK_RES_CONV;
    switch (form) {
        case WINO_PADDED_IDENT: return {tcn_stage_wino_kernel<VT, true, MW>, wino_ldb<VT, MW>(), WTAPS};
        case WINO_PADDED_NONE: return {tcn_stage_wino_kernel<VT, false, MW>, wino_ldb<VT, MW>(), WTAPS};
        case WINO_VALID:
            return {ident ? tcn_stage_wino_kernel<VT, true, MW, true> : tcn_stage_wino_kernel<VT, false, MW, true>, wino_ldb<VT, MW>(), WTAPS};
        case WINO_VALID_RES: return {tcn_stage_wino_kernel<VT, false, MW, true, true>, wino_ldb<VT, MW>(), WTAPS};
        default: return {conv ? tcn_stage_wino_s2_kernel<VT, true, MW> : tcn_stage_wino_s2_kernel<VT, false, MW>, wino2_ldb<VT, MW>(), W2TAPS};
    }
}

// -2: the shape is not one the form's kernel is built for (nothing launched; the caller runs the direct kernels); 0 / error code
// otherwise.  w_img: the form's weight image (fold.pack_conv_weight_wino, stride 2: fold.pack_conv_weight_wino_s2).  The workgroup
// shape is picked by the form's own column count ((t_out + 1) / 2 pairs per sequence).
static int tcn_stage_wino_launch(WinoFormId form, const float *y, const float *w_img, const float *x_res, const float *w_res,
                                 const float *bias, float *out, int n_seg, int c, int c_out, int t_in, int V, int k, int stride, int pad,
                                 int res_mode, int c_res, int t_res, int res_off, int relu, void *stream) {
    const WinoForm &f = WINO_FORMS[form];
    if (!w_img || !y || !bias || !out) return -2;
    if (k != 9 || stride != f.stride || pad != f.pad || t_in < f.t_min) return -2;
    if (res_mode < 0 || res_mode > CSK_RES_CONV || !((f.res_modes >> res_mode) & 1)) return -2;
    const bool res = res_mode != CSK_RES_NONE;
    if (res ? (res_off != f.res_off || !x_res || t_res != t_in) : (f.none_off >= 0 && res_off != f.none_off)) return -2;
    if (res_mode == CSK_RES_IDENTITY && c_res != c_out) return -2;
    if (res_mode == CSK_RES_CONV && (!w_res || c_res < f.cres_unit || c_res % f.cres_unit != 0)) return -2;
    if ((V != 25 && V != 18) || c_out % WMT != 0 || c < 1 || n_seg < 1) return -2;
    if ((int64_t)t_in * V >= (1 << 26)) return -2;                    // 32-bit position / lane byte offsets inside a segment
    if (csk_diag_flag("CSK_TCN_WINO") && csk_diag_int("CSK_TCN_WINO") < 2) return -2;   // diagnostic A/B switch: the direct kernels
    const int t_out = (t_in + 2 * pad - k) / stride + 1;
    const int qp = (t_out + 1) / 2 * V;
    const int mw = wino_pick_mw(qp, c_out, stride);
    const int qtiles = (qp + WNT / mw - 1) / (WNT / mw), mtiles = c_out / (WMT * mw);
    if ((int64_t)qtiles * mtiles * n_seg >= (1ll << 31)) return -2;
    // a form without residual has always passed nullptr / 0 for the residual fields
    TcnParams p = tcn_params(y, w_img, res ? x_res : nullptr, res_mode == CSK_RES_CONV ? w_res : nullptr, bias, out, c, c_out, t_in, t_out,
                             V, k, stride, pad, res_mode, res ? c_res : 0, res ? t_res : 0, res ? f.res_off : 0, relu);
    p.mtiles = (unsigned)mtiles; p.qtiles = (unsigned)qtiles; p.nt = qp;
    const WinoKernel wk = V == 25 ? (mw == 2 ? wino_kernel_of<25, 2>(form, res_mode) : wino_kernel_of<25, 1>(form, res_mode))
                                  : (mw == 2 ? wino_kernel_of<18, 2>(form, res_mode) : wino_kernel_of<18, 1>(form, res_mode));
    p.ldb = wk.ldb;
    const size_t lds = (size_t)(wk.taps * KC * WMT * mw + KC * wk.ldb) * sizeof(float);
    if (const int e = csk_ensure_lds((const void *)wk.kern, lds)) return e;
    hipLaunchKernelGGL(wk.kern, dim3((unsigned)(qtiles * mtiles * n_seg)), dim3(NTHREADS), lds, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

// the entries that fall back themselves: the form's kernel, else (-2) the direct kernels on the direct image w
static int tcn_stage_wino_or_direct(int form, const float *y, const float *w, const float *x_res, const float *w_res, const float *bias,
                                    float *out, int n_seg, int c, int c_out, int t_in, int V, int k, int stride, int pad, int res_mode,
                                    int c_res, int t_res, int res_off, int relu, const float *w_img, void *stream) {
    const int rc = form < 0 ? -2
                            : tcn_stage_wino_launch((WinoFormId)form, y, w_img, x_res, w_res, bias, out, n_seg, c, c_out, t_in, V, k, stride,
                                                    pad, res_mode, c_res, t_res, res_off, relu, stream);
    if (rc != -2) return rc;
    return csk_tcn_stage_f32(y, w, x_res, w_res, bias, out, n_seg, c, c_out, t_in, V, k, stride, pad, res_mode, c_res, t_res,
                             res_off, relu, stream);
}

extern "C" int csk_tcn_stage_wino_f32(const float *y, const float *w, const float *x_res, const float *w_res, const float *bias,
                                      float *out, int n_seg, int c, int c_out, int t_in, int V, int k, int stride, int pad,
                                      int res_mode, int c_res, int t_res, int res_off, int relu, const float *w_wino, void *stream) {
    return tcn_stage_wino_or_direct(WINO_PADDED_IDENT, y, w, x_res, w_res, bias, out, n_seg, c, c_out, t_in, V, k, stride, pad, res_mode,
                                    c_res, t_res, res_off, relu, w_wino, stream);
}

extern "C" int csk_tcn_stage_wino_ext_f32(const float *y, const float *w, const float *x_res, const float *w_res, const float *bias,
                                          float *out, int n_seg, int c, int c_out, int t_in, int V, int k, int stride, int pad,
                                          int res_mode, int c_res, int t_res, int res_off, int relu, const float *w_wino_ext,
                                          void *stream) {
    // form A at stride 1, form B at stride 2, the direct kernels at any other
    return tcn_stage_wino_or_direct(stride == 1 ? WINO_PADDED_NONE : stride == 2 ? WINO_S2 : -1, y, w, x_res, w_res, bias, out, n_seg, c,
                                    c_out, t_in, V, k, stride, pad, res_mode, c_res, t_res, res_off, relu, w_wino_ext, stream);
}

extern "C" int csk_tcn_stage_wino_valid_f32(const float *y, const float *w, const float *x_res, const float *w_res, const float *bias,
                                            float *out, int n_seg, int c, int c_out, int t_in, int V, int k, int stride, int pad,
                                            int res_mode, int c_res, int t_res, int res_off, int relu, const float *w_wino,
                                            void *stream) {
    return tcn_stage_wino_or_direct(WINO_VALID, y, w, x_res, w_res, bias, out, n_seg, c, c_out, t_in, V, k, stride, pad, res_mode, c_res,
                                    t_res, res_off, relu, w_wino, stream);
}

// -2 where the shape is not the kernel's: no launch, the caller runs csk_tcn_stage_f32 (include/cskel.h)
extern "C" int csk_tcn_stage_wino_valid_res_f32(const float *y, const float *x_res, const float *w_res, const float *bias, float *out,
                                                int n_seg, int c, int c_out, int t_in, int V, int k, int stride, int pad,
                                                int res_mode, int c_res, int t_res, int res_off, int relu, const float *w_wino,
                                                void *stream) {
    return tcn_stage_wino_launch(WINO_VALID_RES, y, w_wino, x_res, w_res, bias, out, n_seg, c, c_out, t_in, V, k, stride, pad, res_mode,
                                 c_res, t_res, res_off, relu, stream);
}

