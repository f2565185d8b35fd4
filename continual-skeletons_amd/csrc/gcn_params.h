// gcn_params.h -- launch parameters shared by the GCN-stage kernels (gcn.hip, gcn_dense.hip)
#pragma once
#include <stdint.h>

#include "mfma_core.h"

struct GcnParams {
    const float *x, *w, *bias;
    float *y;
    const int32_t *ell_src;
    const float *ell_val;
    int ell_cnt[3];
    int ell_w;
    int64_t adj_seg_stride, x_seg_stride, x_chan_stride, y_seg_stride, y_chan_stride;
    int Cin, CinPad, Cout, Mpad, frames, V, R, res_mode, ldb;
    unsigned vmagic, mtiles, qtiles;
    int dense;   // src[e] == e for all subsets and columns (checked on the host side of the ABI by construction)
    int adj_per_frame;   // the (dense) adjacency varies per FRAME of a segment: index = seg * frames + frame
    int lds_frames;      // frames of adjacency staged per workgroup in that mode
    int fast_epi;        // channel strides fit the 32-bit lane offsets of the scalar-base epilogue addressing
    // split-K (latency mode, csk_gcn_stage_splitk_f32): split ks of a tile covers channels [ks * cper, + cper) and writes raw
    // partial sums to part[(seg * ksplit + ks)][Cout][y_chan_stride]; gcn_reduce_kernel adds them up in split order
    int ksplit, cper;
    float *part;
    // step16.hip: segment s of the launch is slot (ring_slot0 + s) % ring_slots of x / y (plain calls: no wrap, 1 << 30 slots)
    int x_ring_slots, x_ring_slot0, y_ring_slots, y_ring_slot0;
};

// The arguments of csk_gcn_stage_f32 in their order (include/cskel.h), then the split of csk_gcn_stage_splitk_f32 (1 / null: unsplit).
// Every entry point fills one; nothing below the entries takes the positional list.
struct GcnCall {
    const float *x;
    float *y;
    const float *w, *bias;
    const int32_t *ell_src;
    const float *ell_val;
    const int32_t *ell_cnt;
    int ell_w;
    int64_t adj_seg_stride;
    int adj_per_frame, n_seg, c_in, c_out, frames, V;
    int64_t x_seg_stride, x_chan_stride, y_seg_stride, y_chan_stride;
    int res_mode, ksplit;
    float *partial;
};

// The fields every launcher (gcn.hip, step16.hip) derives from the operands: a plain, unsplit call.  The launcher adds its own:
// tile geometry, dense / adj_per_frame / lds_frames, ring slots, a split.
inline GcnParams gcn_params(const GcnCall &c) {
    GcnParams p = {};
    p.x = c.x; p.w = c.w; p.bias = c.bias; p.y = c.y; p.ell_src = c.ell_src; p.ell_val = c.ell_val;
    for (int i = 0; i < 3; ++i) p.ell_cnt[i] = c.ell_cnt[i];
    p.ell_w = c.ell_w; p.adj_seg_stride = c.adj_seg_stride;
    p.x_seg_stride = c.x_seg_stride; p.x_chan_stride = c.x_chan_stride; p.y_seg_stride = c.y_seg_stride; p.y_chan_stride = c.y_chan_stride;
    p.Cin = c.c_in; p.CinPad = round_up(c.c_in, CSK_CPAD); p.Cout = c.c_out; p.Mpad = round_up(c.c_out, CSK_MT);
    p.frames = c.frames; p.V = c.V; p.R = c.res_mode == CSK_RES_CONV ? 4 : 3; p.res_mode = c.res_mode;
    p.vmagic = vmagic_of(c.V);
    // 32-bit lane byte offsets: 4 * (4 * row_stride + position) must stay below 2^32
    p.fast_epi = c.x_chan_stride < (1ll << 27) && c.y_chan_stride < (1ll << 27);
    p.x_ring_slots = p.y_ring_slots = 1 << 30; p.x_ring_slot0 = p.y_ring_slot0 = 0;
    p.ksplit = 1; p.cper = p.CinPad; p.part = c.partial;
    return p;
}

// gcn_dense.hip: dense (per-segment or per-frame) adjacency at the joint counts V = 18 and V = 25.  The instantiation a launch
// runs, MT * 1000 + V * 10 + CONVRES of gcn_stage_dense2_kernel; 0 where the shape is not one the file is built for (the caller
// then uses the kernels of gcn.hip).  Host arithmetic: of p.x / p.ell_val only the alignment is read (csk_gcn_stage_f32_route)
int csk_gcn_dense2_route(const GcnParams &p, int n_seg);
// launches the instantiation `route` names: the non-zero value csk_gcn_dense2_route gave for this p and n_seg
int csk_launch_gcn_dense2(GcnParams p, int n_seg, int route, void *stream);

// step16.hip: the slot-balanced 16x16x4 tiles for skeleton-sparse adjacencies on 16-byte-aligned layouts.  The instantiation a
// launch runs, NB * 1000 + F * 100 + CONVRES * 10 of gcn16_kernel; 0 where the shape is not supported or the 32x32x2 kernels pack
// the chip as well (bitwise the same results either way).  Host arithmetic: of p.x / p.y only the alignment is read
// (csk_gcn_stage_f32_tile)
int csk_gcn16_tile(const GcnParams &p, int n_seg);
// launches the instantiation `tile` names: the non-zero value csk_gcn16_tile gave for this p and n_seg
int csk_launch_gcn16(GcnParams p, int n_seg, int tile, void *stream);
