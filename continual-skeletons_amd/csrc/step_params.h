// step_params.h -- the host path shared by the continual-step entries (step.hip: csk_tcn_step_f32 and the 32x32x2 tiles; step16.hip:
// the slot-balanced 16x16x4 tiles; step_split.hip: csk_tcn_step_bf16x3): the call record, its check, the launch parameters
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

// The arguments of csk_tcn_step_f32 in their order (include/cskel.h), its split last (1 / null: unsplit).  Every entry fills one; nothing
// below the entries takes the positional list.  w / w_res are untyped: csk_tcn_step_bf16x3 fills the same record with its images.
struct StepCall {
    const float *ring; int slots, head, head_step, n_emit; const void *w; const float *x_res; int x_res_slots, x_res_slot0, x_res_step; const void *w_res;
    const float *bias; float *out; int out_slots, out_slot0, c, c_out; int64_t P; int k, res_mode, c_res, relu, ksplit; float *partial;
};

// The fields both launchers (step.hip, step16.hip) derive from a call; the launcher adds the grid.  A call without x_res still forms slot offsets
// from the residual ring: the post-GCN ring stands in as a ring of ONE slot (the one copy of that rule: the split entry reads it from here).
inline StepParams step_params(const StepCall &c) {
    StepParams p = {};
    p.ring = c.ring; p.w = (const float *)c.w; p.xres = c.x_res ? c.x_res : c.ring; p.wres = (const float *)c.w_res; p.bias = c.bias; p.out = c.out;
    p.C = c.c; p.Cpad = round_up(c.c, CSK_CPAD); p.Cout = c.c_out; p.Mpad = round_up(c.c_out, CSK_MT);
    p.K = c.k; p.slots = c.slots; p.head = c.head; p.head_step = c.head_step; p.res_mode = c.res_mode;
    p.Cres = c.c_res > 0 ? c.c_res : 1; p.CresPad = round_up(p.Cres, CSK_CPAD); p.relu = c.relu; p.P = c.P;
    p.fast_epi = c.P < (1ll << 27);         // 32-bit lane byte offsets: 4 * (4 * row_stride + position) must stay below 2^32
    p.xres_slots = c.x_res ? c.x_res_slots : 1; p.xres_slot0 = c.x_res ? c.x_res_slot0 : 0; p.xres_step = c.x_res_step; p.out_slots = c.out_slots; p.out_slot0 = c.out_slot0;
    p.ksplit = split_ranges(p.Cpad, c.c, c.ksplit, KC, &p.cper); p.part = c.partial;
    return p;
}

// What csk_tcn_step_f32 and csk_tcn_step_bf16x3 require of a call, reported as "<w>: ..." in the ONE order of the lines below (slots_head: how
// the entry words that line; the exact entry, whose k varies, names k there).  operands = false is the SHAPE level of the query: what reads a
// pointer or a slot index is left out.  What only ONE entry requires is in its limits (0, or -1 with the message set):
//   csk_tcn_step_f32     k in 1..9; head_step >= 0; ksplit in 1..32 and its buffer (aligned: checked once the ranges are known); the P bound
//   csk_tcn_step_bf16x3  k == 9; head_step in 1..2; a valid res_mode; out and the images aligned; no ring of 4 GB; c_res > 0 (after the shared lines)
// A call that breaks one requirement is refused with the text it always had.  Which of SEVERAL broken requirements is named follows this
// order in both entries; each used to have an order of its own.
template <class Limits>
inline int step_check(const char *w, const char *slots_head, const StepCall &c, bool operands, Limits limits) {
    if (operands && (!c.ring || !c.w || !c.bias || !c.out)) CSK_FAIL("%s: null pointer", w);
    if (c.c <= 0 || c.c_out <= 0 || c.P < 4 || (c.P & 3)) CSK_FAIL("%s: bad dims (P must be a positive multiple of 4)", w);
    if (const int rc = limits()) return rc;
    if (c.slots < c.k || (operands && (c.head < 0 || c.head >= c.slots))) CSK_FAIL("%s: bad %s", w, slots_head);
    if (c.n_emit < 1 || c.n_emit > 64 || c.out_slots < c.n_emit || (operands && (c.out_slot0 < 0 || c.out_slot0 >= c.out_slots))) CSK_FAIL("%s: bad emission geometry", w);
    if (c.slots < c.k - 1 + (c.n_emit - 1) * c.head_step + 1) CSK_FAIL("%s: ring too shallow for %d emissions", w, c.n_emit);
    if (c.res_mode != CSK_RES_NONE) {
        if (operands && !c.x_res) CSK_FAIL("%s: residual requested without x_res", w);
        if (c.x_res_slots < 1 || (operands && (c.x_res_slot0 < 0 || c.x_res_slot0 >= c.x_res_slots || c.x_res_step < 0))) CSK_FAIL("%s: bad residual ring geometry", w);
        if (c.res_mode == CSK_RES_IDENTITY && c.c_res != c.c_out) CSK_FAIL("%s: identity residual needs c_res == c_out", w);
        if (operands && c.res_mode == CSK_RES_CONV && !c.w_res) CSK_FAIL("%s: conv residual without w_res", w);
    }
    if (operands && (((uintptr_t)c.ring | (uintptr_t)c.x_res) & 15)) CSK_FAIL("%s: state pointers must be 16-byte aligned", w);
    return 0;
}

// step16.hip: the slot-balanced tile family (64 channels x 16*NB columns, v_mfma_f32_16x16x4_f32).  The instantiation a launch runs, NB * 1000
// + E * 100 + HS * 10 + TAIL of tcn_step16_kernel; 0: not a launch of this family, which has its own fp32 summation order and so takes a launch
// by (k, ksplit, ring size) only, never by its size.  Host arithmetic on the shape fields of p, asked once per launch (step_route, step.hip)
int csk_tcn_step16_tile(const StepParams &p, int n_emit);
// launches the instantiation `tile` names: the non-zero value csk_tcn_step16_tile gave for this p and n_emit
int csk_launch_tcn_step16(StepParams p, int n_emit, int tile, void *stream);
// fused stack of 64-channel blocks (csk_co_block_step_f32 / csk_co_stack_step_f32); -2: shape not supported
int csk_launch_co_stack16(int n_blocks, const csk_co_block_args *blocks, int n_skel, int V, int64_t P, void *stream);
