// step_params.h -- launch parameters shared by the continual-step kernels (step.hip: 32x32x2 tiles; step16.hip: the
// slot-balanced 16x16x4 tiles)
#pragma once
#include <stdint.h>

#include "mfma_core.h"

struct StepParams {
    const float *ring, *w, *xres, *wres, *bias;     // xres / out are RING bases; slots are picked per emission
    float *out;
    int C, Cpad, Cout, Mpad, K, slots, head, head_step;
    int res_mode, Cres, CresPad, relu;
    int xres_slots, xres_slot0, xres_step, out_slots, out_slot0;
    int fast_epi;      // P fits the 32-bit lane byte offsets of the scalar-base epilogue addressing
    unsigned gx, gy, gz;   // position tiles, m-tiles, emission groups [* ksplit] of the launch (the grid is 1-D)
    int ksplit, cper;  // split-K (latency mode): emission groups * ksplit slices, split ks covers channels [ks*cper, ..+cper)
    float *part;       // and writes raw partial sums to part[(emission*ksplit + ks)][Cout][P]; 1 = off
    int64_t P;
};

// The fields both launchers (step.hip, step16.hip) derive from the operands, in the argument order of csk_tcn_step_f32, unsplit.
// xres / xres_slots / xres_slot0 are taken as given: a launch without a residual still forms slot offsets from them, and each
// launcher keeps the stand-ins it has always passed.  The launcher adds the grid and a split.
inline StepParams step_params(const float *ring, int slots, int head, int head_step, const float *w, const float *xres, int xres_slots,
                              int xres_slot0, int xres_step, const float *wres, const float *bias, float *out, int out_slots,
                              int out_slot0, int c, int c_out, int64_t P, int k, int res_mode, int c_res, int relu) {
    StepParams p = {};
    p.ring = ring; p.w = w; p.xres = xres; p.wres = wres; p.bias = bias; p.out = out;
    p.C = c; p.Cpad = round_up(c, CSK_CPAD); p.Cout = c_out; p.Mpad = round_up(c_out, CSK_MT);
    p.K = k; p.slots = slots; p.head = head; p.head_step = head_step; p.res_mode = res_mode;
    p.Cres = c_res > 0 ? c_res : 1; p.CresPad = round_up(p.Cres, CSK_CPAD); p.relu = relu; p.P = P;
    // 32-bit lane byte offsets: 4 * (4 * row_stride + position) must stay below 2^32
    p.fast_epi = P < (1ll << 27);
    p.xres_slots = xres_slots; p.xres_slot0 = xres_slot0; p.xres_step = xres_step; p.out_slots = out_slots; p.out_slot0 = out_slot0;
    p.ksplit = 1; p.cper = p.Cpad; p.part = nullptr;
    return p;
}

// step16.hip: the slot-balanced tile family (64 channels x 16*NB columns, v_mfma_f32_16x16x4_f32).  Both return -2 when the
// launch is not one they take (the caller then launches the 32x32x2 kernels / the per-stage launches); otherwise the launch
// status.  Of the 16x16x4 kernels, gcn16_kernel equals gcn_stage_sparse2_kernel bit for bit (as the stride-1 tcn_stage16_kernel
// equals tcn_stage_kernel); tcn_step16_kernel differs from tcn_step_kernel by its fp32 summation order (4-channel chunks where
// the 32x32x2 kernel walks 8; so does the stride-2 tcn_stage16_kernel), so it takes a launch by (k, ksplit, ring size) only,
// never by the launch size.
int csk_launch_tcn_step16(StepParams p, int n_emit, void *stream);
// the instantiation that launch runs, NB * 1000 + E * 100 + HS * 10 + TAIL of tcn_step16_kernel; 0 where it returns -2.  Host
// arithmetic on the shape fields of p only (csk_tcn_step_f32_tile)
int csk_tcn_step16_tile(const StepParams &p, int n_emit);
// fused stack of 64-channel blocks (csk_co_block_step_f32 / csk_co_stack_step_f32); -2: shape not supported
int csk_launch_co_stack16(int n_blocks, const csk_co_block_args *blocks, int n_skel, int V, int64_t P, void *stream);
