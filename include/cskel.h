/*
 * cskel.h -- C ABI of the MI355X-native ST-GCN / CoST-GCN forward path (libcskel_hip.so).
 *
 * The reference (LukasHedegaard/continual-skeletons) has no native code and no FFI: its hot path is
 * the Python nn.Module surface of models/base.py issuing stock ATen ops.  Each entry point below
 * replaces the ATen op sequence of one reference method (cited per function); the Python host layer
 * in continual-skeletons_amd/ mirrors the reference's module interface and binds these with ctypes.
 *
 * Conventions
 *  - all tensors fp32, device (HBM) pointers, laid out exactly as the reference's contiguous tensors:
 *    clip activations (NM, C, T, V) with V innermost; "segment" = one of the NM skeleton sequences.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); launches are asynchronous.  The stage / step /
 *    head entry points (csk_gcn_stage_f32 ... csk_fuse_rank_f32) neither allocate nor synchronise and are
 *    graph-capture safe (the first launch of a kernel instantiation raises its LDS cap with hipFuncSetAttribute).
 *    Exceptions: csk_stream_overlap_probe synchronises both streams it is given; csk_co_plan_create / _destroy
 *    allocate host memory.
 *  - packed weights are produced once on the host by continual-skeletons_amd/fold.py
 *    (BatchNorm(eval) + bias folding, zero padding of channel counts to CSK_CPAD / CSK_MT multiples).
 *  - return value: 0 = ok; <0 = argument error (see csk_last_error()); >0 = hipError_t of the launch.
 */
#ifndef CSKEL_H
#define CSKEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Stays 16 while entries are only added: csk_derive_modality_f32 / _frames_f32, csk_prenorm_f32 / _frames_f32,
 * csk_tcn_stage_wino_valid_f32, csk_tcn_stage_wino_valid_res_f32, csk_co_plan_set_delays, csk_gcn_stage_f32_route, csk_gcn_stage_splitk_f32_route, csk_co_prime_pack_f32, csk_co_head_clip_f32, csk_str_unit_f32_route,
 * csk_co_stack_step_f32_route, csk_tcn_step_f32_route and
 * csk_select_people_f32 / _frames_f32 and csk_ntu_intake_f32 are additive (no existing entry, struct
 * or constant changed). */
#define CSK_ABI_VERSION 16
#define CSK_KC 8    /* channel-chunk of the K loop of the TCN kernels                                */
#define CSK_CPAD 16 /* packed weights zero-pad C_in to a multiple of this                             */
#define CSK_MT 64  /* packed weights pad C_out to a multiple of this                               */

/* residual forms of SpatioTemporalBlock (models/base.py:367-374) and GraphConvolution (:246-254) */
#define CSK_RES_NONE 0
#define CSK_RES_IDENTITY 1
#define CSK_RES_CONV 2

int csk_abi_version(void);
/* thread-local text of the last argument error */
const char *csk_last_error(void);

/*
 * Do two HIP streams execute concurrently on this device?  HIP multiplexes its streams onto a few hardware queues
 * (4 by default); two streams that land on the same queue run strictly one after the other, which silently turns the
 * stream shards of the continual path (parallel.py:StreamShards; the reference has no counterpart, it steps one
 * Python module at a time) into a serial schedule.  Launches one single-wavefront kernel that spins for spin_us
 * microseconds on each stream behind a common start event and writes
 *   *ratio = (time until both have finished) / (time of one alone):   ~1 = concurrent, ~2 = serialised.
 * Synchronises both streams.  No other work should be in flight on either stream.
 */
int csk_stream_overlap_probe(void *stream_a, void *stream_b, int spin_us, float *ratio);

/*
 * GraphConvolution.forward, models/base.py:260-270 (and its per-frame use by CoGraphConvolution,
 * base.py:273-276):   y = ReLU( BN( sum_i W_i * (x .A_eff[i]) + b_i ) + gcn_residual(x) )
 *
 *  x        (n_seg, c_in, frames, V) with strides x_seg_stride / x_chan_stride (elements); frames
 *           contiguous (V floats each).
 *  y        (n_seg, c_out, frames, V), same convention.
 *  w        packed [R][c_in_pad][c_out_pad]; R = 3 subsets (+1 = conv gcn_residual when
 *           res_mode == CSK_RES_CONV); BN scale folded in.
 *  bias     [c_out_pad] folded (conv biases, BN shift, and gcn_residual's BN shift).
 *  ell_src  [3][V][ell_w] int32 : row indices v of the non-zeros of column w of A_eff[i] (padded with 0)
 *  ell_val  [3][V][ell_w] fp32  : their values (padded with 0.0)
 *  ell_cnt  [3] : number of meaningful entries per subset (<= ell_w) -- lets sparse subsets skip padding
 *  adj_seg_stride: 0 for a graph shared by all segments (ST-GCN); 3*V*ell_w for per-segment VALUES
 *           (A-GCN's per-sample attention, models/a_gcn/a_gcn.py:62-65; ell_src stays shared).  A per-segment
 *           adjacency with ell_w == V and ell_cnt == {V,V,V} MUST list every source joint in order
 *           (ell_src[i][w][e] == e): the kernel then takes its dense fast path and does not read ell_src.
 *  adj_per_frame: 0, or 1 = the dense adjacency varies per FRAME: matrix index = seg*frames + frame, consecutive
 *           matrices adj_seg_stride apart (continual A-GCN: every frame of the channel-major layout is another
 *           skeleton with its own attention, models/coa_gcn/coa_gcn.py:11-14).
 *  res_mode CSK_RES_IDENTITY (c_in == c_out) or CSK_RES_CONV.
 */
int csk_gcn_stage_f32(const float *x, float *y, const float *w, const float *bias,
                      const int32_t *ell_src, const float *ell_val, const int32_t *ell_cnt,
                      int ell_w, int64_t adj_seg_stride, int adj_per_frame,
                      int n_seg, int c_in, int c_out, int frames, int V,
                      int64_t x_seg_stride, int64_t x_chan_stride,
                      int64_t y_seg_stride, int64_t y_chan_stride,
                      int res_mode, void *stream);

/*
 * The tile family csk_gcn_stage_f32 picks for a launch: 0 = the 32x32x2 kernels (csrc/gcn.hip), else the instantiation of the
 * slot-balanced 16x16x4 graph conv (csrc/step16.hip) as NB * 1000 + F * 100 + CONVRES * 10 -- NB column blocks of 16 positions
 * per tile (25 or 18), F segments per tile (4, 2 or 1), CONVRES 1 for the conv gcn_residual.  Arguments as the stage's own; of
 * x and y only the alignment is read, they are never dereferenced.  Host arithmetic only (no GPU); -1 on bad dims.  For tests
 * and tools: results do not depend on the family (bitwise the same sums).
 */
int csk_gcn_stage_f32_tile(const float *x, const float *y, const int32_t *ell_cnt, int ell_w, int64_t adj_seg_stride,
                           int adj_per_frame, int n_seg, int c_in, int c_out, int frames, int V,
                           int64_t x_seg_stride, int64_t x_chan_stride, int64_t y_seg_stride, int64_t y_chan_stride,
                           int res_mode);

/*
 * The kernel csk_gcn_stage_f32 launches for a call, as family * 1000000 + the template arguments of the instantiation:
 *   1000000 + MT * 10 + CONVRES            gcn_stage_sparse2_kernel<MT, CONVRES, 8>    (csrc/gcn.hip; skeleton-sparse shared adjacency)
 *   2000000 + csk_gcn_stage_f32_tile's     gcn16_kernel<NB, F, CONVRES, 8>             (csrc/step16.hip; the value above, never 0 here)
 *   3000000 + MT * 1000 + V * 10 + CONVRES gcn_stage_dense2_kernel<MT, CONVRES, V, 8>  (csrc/gcn_dense.hip; dense per-segment / per-frame
 *                                                                                       adjacency at V = 18 / 25)
 *   4000000 + CONVRES                      gcn_stage_dense_kernel<128, CONVRES, 8, 3>  (csrc/gcn.hip; dense per-segment adjacency,
 *                                                                                       C_out_pad a multiple of 128, 4 <= V <= 32)
 *   5000000 + MT * 10 + NJ                 gcn_stage_kernel<MT, NJ>                    (csrc/gcn.hip; everything else)
 * MT = rows of a workgroup tile (128 when C_out_pad is a multiple of 128, else 64), CONVRES 1 for the conv gcn_residual, NJ the
 * 64-lane sweeps that stage one activation row (3 / 4 at MT = 128, 5 / 6 at MT = 64).  Arguments as the stage's own without w,
 * bias, ell_src and stream (csk_gcn_stage_f32_tile's plus ell_val): of x, y and ell_val only the alignment is read -- the V = 18
 * form of gcn_dense.hip wants x and ell_val 8-byte aligned and even strides -- they are never dereferenced.  Host arithmetic only
 * (no GPU); -1 (csk_last_error set) where csk_gcn_stage_f32 fails on the dimensions.  The launcher switches on the function this
 * entry reports.  For tests and tools: families 1 and 2 give bitwise the same sums, the others differ in summation order.
 */
int csk_gcn_stage_f32_route(const float *x, const float *y, const float *ell_val, const int32_t *ell_cnt, int ell_w,
                            int64_t adj_seg_stride, int adj_per_frame, int n_seg, int c_in, int c_out, int frames, int V,
                            int64_t x_seg_stride, int64_t x_chan_stride, int64_t y_seg_stride, int64_t y_chan_stride,
                            int res_mode);

/*
 * The same stage with its K loop split over workgroups (latency mode: a handful of streams, where one workgroup per tile
 * would walk all 3 * c_in / 8 K-chunks alone -- 41 us at c_in = 256): the channel axis is cut into up to ksplit ranges
 * computed by separate workgroups into `partial` ([n_seg * ksplit][c_out][y_chan_stride] floats) and summed in split
 * order by a second kernel that also applies bias / identity gcn_residual / ReLU.  Graphs shared by all segments with
 * <= 1 / 1 / 4 non-zeros per column only (skeleton graphs).  Results differ from csk_gcn_stage_f32 by fp32 summation
 * order only; for a given ksplit they do not depend on n_seg or frames.  ksplit = 1 is csk_gcn_stage_f32.
 */
int csk_gcn_stage_splitk_f32(const float *x, float *y, const float *w, const float *bias, const int32_t *ell_src,
                             const float *ell_val, const int32_t *ell_cnt, int ell_w, int n_seg, int c_in, int c_out,
                             int frames, int V, int64_t x_seg_stride, int64_t x_chan_stride, int64_t y_seg_stride,
                             int64_t y_chan_stride, int res_mode, int ksplit, float *partial, void *stream);

/*
 * The launch csk_gcn_stage_splitk_f32 makes for a call.  A request that collapses to ONE channel range (ksplit == 1, or c_in no larger
 * than one range) runs the unsplit stage and no reduction: the value is csk_gcn_stage_f32_route's.  Otherwise
 *   (1 << 30) | (MT == 128) << 29 | CONVRES << 28 | (ranges - 1) << 23 | cper / 8
 * gcn_stage_sparse2_kernel<MT, CONVRES, 8, false, true> over `ranges` channel ranges of cper channels each (the last one what is left
 * of c_in_pad) followed by gcn_reduce_kernel; cper = ceil(c_in_pad / ksplit) rounded up to a multiple of 8, ranges = ceil(c_in / cper)
 * <= ksplit <= 32.  Arguments as the split entry's without w, bias, ell_src and stream; x, y, ell_val and partial are never
 * dereferenced.  Host arithmetic only (no GPU); -1 (csk_last_error set) where csk_gcn_stage_splitk_f32 refuses the call.  The launcher
 * switches on the function this entry reports.
 */
int csk_gcn_stage_splitk_f32_route(const float *x, const float *y, const float *ell_val, const int32_t *ell_cnt, int ell_w, int n_seg,
                                   int c_in, int c_out, int frames, int V, int64_t x_seg_stride, int64_t x_chan_stride,
                                   int64_t y_seg_stride, int64_t y_chan_stride, int res_mode, int ksplit, const float *partial);

/*
 * TemporalConvolution.forward (models/base.py:302-304) fused with the tail of
 * SpatioTemporalBlock.forward (base.py:376-387):
 *     out = ReLU( BN(conv_{k x 1, stride s, pad p}(y)) + residual(x[:, :, shrink:T-shrink]) )
 * or, with relu == 0 and res_mode == NONE, a bare TemporalConvolution.
 *
 *  y        (n_seg, c, t_in, V) contiguous           -- output of the GCN stage
 *  w        packed [k][c_pad][c_out_pad], BN scale folded
 *  x_res    (n_seg, c_res, t_res, V) contiguous or NULL -- block input for the residual
 *  w_res    packed [1][c_res_pad][c_out_pad] (CSK_RES_CONV) or NULL
 *  bias     [c_out_pad] folded (t_conv bias, BN shift, residual conv bias + BN shift)
 *  out      (n_seg, c_out, t_out, V), t_out = (t_in + 2p - k)/s + 1
 *  res_off  frame offset of the residual: out[t'] pairs with x_res[t'*s + res_off]
 *           (= residual_shrink, base.py:379-383; 0 when padded)
 */
int csk_tcn_stage_f32(const float *y, const float *w, const float *x_res, const float *w_res,
                      const float *bias, float *out,
                      int n_seg, int c, int c_out, int t_in, int V, int k, int stride, int pad,
                      int res_mode, int c_res, int t_res, int res_off, int relu, void *stream);

/*
 * csk_tcn_stage_f32 with the 9 x 1 conv evaluated by Winograd minimal filtering where the shape allows (csrc/tcn_wino.hip):
 * the taps as three 3-tap groups, each an F(2, 3) (two output frames from four input frames, points 0, 1, -1, inf), the groups
 * summed in the transformed domain -- 12 instead of 18 fp32 MFMA K-blocks per output frame pair.  Exact fp32 arithmetic; the
 * result differs from csk_tcn_stage_f32 by the rounding of the transformed weights and operands (about 1e-6 relative).
 * Arguments of csk_tcn_stage_f32 plus
 *  w_wino   packed [12][c_pad][c_out_pad]: element [4 g + i][c][co] = sum_r G[i][r] * W'[co][c][3 g + r] (g = 0..2, i = 0..3),
 *           G = {{1, 0, 0}, {1/2, 1/2, 1/2}, {1/2, -1/2, 1/2}, {0, 0, 1}}, formed in fp64 from the BN-folded weight and
 *           rounded to fp32 once (fold.pack_conv_weight_wino); may be NULL
 * Taken for k = 9, stride 1, pad 4, an identity residual without shrink (res_off 0, t_res == t_in), V in {25, 18},
 * c_out % 64 == 0 and w_wino != NULL -- a function of the layer, never of n_seg.  Any other call runs csk_tcn_stage_f32.
 */
int csk_tcn_stage_wino_f32(const float *y, const float *w, const float *x_res, const float *w_res,
                           const float *bias, float *out,
                           int n_seg, int c, int c_out, int t_in, int V, int k, int stride, int pad,
                           int res_mode, int c_res, int t_res, int res_off, int relu, const float *w_wino, void *stream);

/*
 * csk_tcn_stage_f32 with the Winograd forms for the blocks csk_tcn_stage_wino_f32 leaves to the direct kernels (k = 9, pad 4,
 * res_off 0, V in {25, 18}, c_out % 64 == 0, w_wino_ext != NULL; a function of the layer, never of n_seg or t_in):
 *  stride 1, res_mode NONE: the F(2, 3) kernel of csk_tcn_stage_wino_f32 without the residual load;
 *           w_wino_ext = the [12][c_pad][c_out_pad] image of fold.pack_conv_weight_wino.
 *  stride 2, res_mode NONE or CONV (t_res == t_in): with e[n] = y[2 n], o[n] = y[2 n + 1] the conv is a 5-tap conv on e (taps
 *           0, 2, 4, 6, 8) plus a 4-tap conv on o (taps 1, 3, 5, 7), cut into the groups E0 = (w0, w2, w4), E1 = (w6, w8, 0),
 *           O0 = (w1, w3, 0), O1 = (w5, w7, 0), each an F(2, 3); the point-inf product of a 2-tap group is zero and skipped:
 *           13 instead of 18 fp32 MFMA K-blocks per output frame pair and channel.  The 1 x 1 stride-2 residual conv adds 2 per
 *           residual channel, as in the direct form, and streams the direct w_res image.
 *           w_wino_ext = packed [13][c_pad][c_out_pad] (fold.pack_conv_weight_wino_s2): rows 0-3 G.E0, rows 4-6 / 7-9 / 10-12 the
 *           first three rows of G.E1 / G.O0 / G.O1; fp64, rounded to fp32 once.  The caller passes the image that belongs to
 *           `stride`: the entry is not told its size.
 * Exact fp32 arithmetic; differs from csk_tcn_stage_f32 by the rounding of the transformed weights and operands (about 1e-6
 * relative).  Any other call runs csk_tcn_stage_f32.  The Python host layer's SpatioTemporalBlock calls this entry for its
 * stride-2 blocks only; the stride-1 form is for callers that do not need csk_tcn_stage_f32's bits (csk_block_few_channels_f32
 * is bit for bit the direct two-launch block).
 */
int csk_tcn_stage_wino_ext_f32(const float *y, const float *w, const float *x_res, const float *w_res,
                               const float *bias, float *out,
                               int n_seg, int c, int c_out, int t_in, int V, int k, int stride, int pad,
                               int res_mode, int c_res, int t_res, int res_off, int relu, const float *w_wino_ext, void *stream);

/*
 * The VALID (pad 0) form of the stride-1 Winograd kernel: the temporal conv of the unpadded "*" blocks (SpatioTemporalBlock with
 * temporal_padding = 0; StGcnMod layers 2-4, 6-7, 9-10).  Arguments as csk_tcn_stage_f32 plus w_wino, the [12][c_pad][c_out_pad]
 * image of fold.pack_conv_weight_wino -- the SAME image as the padded form's.  For a 9-tap stride-1 conv the unpadded output
 * frame u is the padded output frame u + 4, and the centred identity residual x[u + 4] has that frame's index: the valid form is
 * the kernel of csk_tcn_stage_wino_f32 restricted to the output frames [4, t_in - 4) and stored at t - 4 -- pair columns start
 * at the padded form's pair 2, no column is spent on a halo frame; out is (n_seg, c_out, t_in - 8, V).  Per element the same
 * products in the same order: bit for bit the padded form's frames [4, t_in - 4) (tests/test_gpu_winograd_valid.py).
 * Taken when k == 9, stride == 1, pad == 0, t_in >= 9, V in {25, 18}, c_out % 64 == 0, w_wino != NULL and res_mode is NONE, or
 * IDENTITY with res_off == 4, c_res == c_out, t_res == t_in (a function of the layer, never of n_seg or t_in; the workgroup
 * shape follows the valid form's own column count).  Any other call runs csk_tcn_stage_f32.
 */
int csk_tcn_stage_wino_valid_f32(const float *y, const float *w, const float *x_res, const float *w_res,
                                 const float *bias, float *out,
                                 int n_seg, int c, int c_out, int t_in, int V, int k, int stride, int pad,
                                 int res_mode, int c_res, int t_res, int res_off, int relu, const float *w_wino, void *stream);

/*
 * The valid form with the CONV residual on the centred shrink -- the unpadded "*" blocks that change the channel count (layers 5
 * and 8 of the "*" tables at stride 1; SpatioTemporalBlock with temporal_padding = 0 and in_channels != out_channels):
 *     out[u] = ReLU( BN(conv_{9 x 1, pad 0}(y))[u] + BN(conv_{1 x 1}(x_res))[u + 4] ),   u = 0 .. t_in - 9
 * The kernel of csk_tcn_stage_wino_valid_f32 with a second K phase over the c_res channels of x_res: per output frame pair j the
 * phase adds w_res . x_res[2 j + 4] to the accumulator set M0 and w_res . (-x_res[2 j + 5]) to M3, which the output transform
 * out(2 j) = M0 + M1 + M2, out(2 j + 1) = M1 - M2 - M3 turns into the residual of both frames -- no accumulator set of its own,
 * and the sign is applied to the staged activation, so w_res is the direct [1][c_res_pad][c_out_pad] image of csk_tcn_stage_f32
 * and bias its folded bias (both BN shifts).  Exact fp32 arithmetic; differs from csk_tcn_stage_f32 by the rounding of the
 * transformed weights and operands (about 1e-6 relative).
 * Taken when k == 9, stride == 1, pad == 0, t_in >= 9, V in {25, 18}, c_out % 64 == 0, res_mode == CSK_RES_CONV, res_off == 4,
 * t_res == t_in, c_res a multiple of 16 and x_res, w_res, w_wino != NULL (a function of the layer, never of n_seg or t_in).
 * UNLIKE the entries above this one does not fall back: for any other call it returns -2, launches nothing and leaves
 * csk_last_error() alone; the caller runs csk_tcn_stage_f32.  Arguments as csk_tcn_stage_wino_valid_f32 without the direct conv
 * weight w, which this entry never reads.
 */
int csk_tcn_stage_wino_valid_res_f32(const float *y, const float *x_res, const float *w_res, const float *bias, float *out,
                                     int n_seg, int c, int c_out, int t_in, int V, int k, int stride, int pad,
                                     int res_mode, int c_res, int t_res, int res_off, int relu, const float *w_wino, void *stream);

/*
 * A whole SpatioTemporalBlock with a FEW input channels and no block residual -- layer 1 of the reference's stacks
 * (models/st_gcn/st_gcn.py:30: StGcnBlock(3, 64, A, residual=False); block body models/base.py:376-387) -- in ONE launch:
 *   out = ReLU( tcn( gcn(x) ) ),  gcn(x) = ReLU( sum_k W'_k . (x . A_k) + b' + conv1x1+BN(x) )   (models/base.py:230-270)
 * csk_gcn_stage_f32 (conv gcn_residual) followed by csk_tcn_stage_f32 (k = 9, stride 1, pad 4, no residual), with the graph
 * conv formed on the fly inside the temporal conv's tile: y never travels through memory (2 GB per batch-256 forward).  The
 * results are BIT FOR BIT those of the two calls (the same fmaf chain in the graph conv's K order; zero in the frames of the
 * temporal padding).
 *  x        (n_seg, c_in, t_in, V) contiguous, 1 <= c_in <= 4;  out (n_seg, c_out, t_in, V)
 *  gcn_w / gcn_bias / ell_*  the packed operands of csk_gcn_stage_f32 with the conv gcn_residual as 4th subset, c_mid outputs
 *  tcn_w / tcn_bias          the packed operands of csk_tcn_stage_f32 (c_mid -> c_out, 9 taps)
 *  V in {25, 18}; c_mid a multiple of 8; a skeleton-sparse adjacency (ell_cnt <= 1 / 1 / 4).  Other shapes: the two calls.
 */
int csk_block_few_channels_f32(const float *x, const float *gcn_w, const float *gcn_bias, const int32_t *ell_src,
                               const float *ell_val, const int32_t *ell_cnt, int ell_w, const float *tcn_w,
                               const float *tcn_bias, float *out, int n_seg, int c_in, int c_mid, int c_out, int t_in,
                               int V, int pad, void *stream);

/*
 * csk_tcn_stage_f32 for launches of a FEW tiles (small-batch clip inference; the reference's own CPU protocol is batch 1,
 * scripts/benchmark_all_ntu60.py:17): the K loop of every output tile is cut into `ksplit` channel ranges walked by
 * separate workgroups; raw partial sums go to `partial` ([n_seg * ksplit][c_out][t_out * V] floats, 16-byte aligned) and a
 * second launch adds them IN SPLIT ORDER, then bias, identity residual and ReLU (the conv residual rides in split 0).
 * Same method and arguments as csk_tcn_stage_f32 (models/base.py:302-304 + 376-387); k must be 9.  For a given ksplit the
 * result of a clip does not depend on n_seg; against ksplit = 1 it differs by the summation order only.
 */
int csk_tcn_stage_splitk_f32(const float *y, const float *w, const float *x_res, const float *w_res,
                             const float *bias, float *out,
                             int n_seg, int c, int c_out, int t_in, int V, int k, int stride, int pad,
                             int res_mode, int c_res, int t_res, int res_off, int relu, int ksplit, float *partial,
                             void *stream);

/*
 * Bare 1 x 1 conv + bias on the layouts of csk_gcn_stage_f32 (no adjacency, no residual, no ReLU): the six a_i / b_i
 * embedding convs of AdaptiveGraphConvolution fused into one GEMM, models/a_gcn/a_gcn.py:27-28, 53-59.
 *  x (n_seg, c_in, frames, V), y (n_seg, c_out, frames, V) with explicit segment / channel strides (elements);
 *  w packed [1][c_in_pad][c_out_pad], bias [c_out_pad].
 */
int csk_conv1x1_f32(const float *x, float *y, const float *w, const float *bias, int n_seg, int c_in, int c_out,
                    int frames, int V, int64_t x_seg_stride, int64_t x_chan_stride, int64_t y_seg_stride,
                    int64_t y_chan_stride, void *stream);

/*
 * OPT-IN precision mode "bf16x3" of csk_tcn_stage_f32 (same reference method, models/base.py:302-304 + 376-387; same
 * arguments and layouts except the weights): the 9 x 1 temporal conv and the 1 x 1 residual conv run on the bf16 matrix
 * pipe with every fp32 operand split into three bf16 pieces (h + m + l, 24 significand bits) and the six piece products
 * of order <= 2 accumulated in fp32 -- fp32-GRADE results (measured max error vs the oracle: profiles/r03_parity_report.json),
 * not the exact fp32 arithmetic of csk_tcn_stage_f32.  Never selected implicitly: blocks.set_precision(module, "bf16x3").
 *  w_split      packed split weights of the (k = 9) conv, BN scale folded: 16-byte vectors of 8 bf16 (8 consecutive
 *               input channels) indexed [c_pad / 16][9 tap slots][3 pieces][2 channel halves][c_out_pad], the taps in
 *               CLASS-MAJOR order (0, s, 2s, ..., 1, 1 + s, ... for stride s: the taps of a residue class read one
 *               de-interleaved set of source frames); fold.pack_conv_weight_split
 *  w_res_split  the same for the 1 x 1 residual conv: [c_res_pad / 16][3 slots: tap 0, zero, zero][3][2][c_out_pad], or NULL
 *  k            must be 9; stride <= 4
 */
int csk_tcn_stage_bf16x3(const float *y, const void *w_split, const float *x_res, const void *w_res_split,
                         const float *bias, float *out,
                         int n_seg, int c, int c_out, int t_in, int V, int k, int stride, int pad,
                         int res_mode, int c_res, int t_res, int res_off, int relu, void *stream);

/*
 * OPT-IN precision mode "bf16x3" of csk_gcn_stage_f32 (same reference method, models/base.py:260-270) for skeleton-sparse
 * graphs (<= 1/1/4 non-zeros per adjacency column), C_out a multiple of 128 and contiguous (n_seg, C, frames, V) tensors:
 * the adjacency aggregation stays exact fp32, the channel-mixing GEMM runs on the bf16 matrix pipe with its operands split
 * into three bf16 pieces (fp32-grade, see csk_tcn_stage_bf16x3).
 *  w_split      split image of the three 1 x 1 convs (BN scale folded): [c_in_pad / 16][3 subsets][3 pieces][2 halves][c_out_pad]
 *  w_res_split  split image of the conv gcn_residual, [c_in_pad / 16][3 slots: the conv, zero, zero][3][2][c_out_pad], or NULL
 *  bias, ell_*  as csk_gcn_stage_f32 (shared adjacency: adj_seg_stride = 0)
 */
int csk_gcn_stage_bf16x3(const float *x, float *y, const void *w_split, const void *w_res_split, const float *bias,
                         const int32_t *ell_src, const float *ell_val, const int32_t *ell_cnt, int ell_w,
                         int n_seg, int c_in, int c_out, int frames, int V, int res_mode, void *stream);

/*
 * Input permute + data_bn + reshape, models/st_gcn/st_gcn.py:49-57 (clip) and
 * models/base.py:73-82 (per frame, t = 1):
 *     h[n*M+m, c, t, v] = x[n, c, t, v, m] * scale[(m*V+v)*C+c] + shift[(m*V+v)*C+c]
 *  x (N, C, T, V, M) contiguous;  h (N*M, C, T, V) with strides h_seg_stride/h_chan_stride.
 */
int csk_input_norm_f32(const float *x, const float *scale, const float *shift, float *h,
                       int N, int C, int T, int V, int M,
                       int64_t h_seg_stride, int64_t h_chan_stride, void *stream);

/*
 * Head, models/st_gcn/st_gcn.py:60-64: feat[n, c] = mean_m mean_{t,v} h[n*M+m, c, t, v];
 * logits = feat @ fc_w^T + fc_b.   h (N*M, C, TV) contiguous; feat (N, C) is also returned
 * (it is the per-step feature of CoModelBase.spatial_pool, models/base.py:84).
 *  fc_w (classes, C) row-major as in nn.Linear; logits (N, classes).  Pass logits == NULL to only pool.
 */
int csk_pool_fc_f32(const float *h, const float *fc_w, const float *fc_b, float *feat, float *logits,
                    int N, int M, int C, int TV, int classes, void *stream);

/* feat[n, c] = scale * mean_m mean_{tv} h[n*M+m, c, tv]: the clip-mode evaluation of CoModelBase's head
 * (spatial_pool + zero-padded co.AvgPool1d window, models/base.py:84-97,166-181) uses scale = frames/pool_size */
int csk_pool_scaled_f32(const float *h, float *feat, int N, int M, int C, int TV, float scale, void *stream);

/* plain FC on pooled features: logits[n] = feat[n] @ fc_w^T + fc_b  (co.Linear, models/base.py:99).  When C is a
 * multiple of 4 the rows are read 16 bytes at a time: feat and fc_w must then be 16-byte aligned (an error otherwise). */
int csk_fc_f32(const float *feat, const float *fc_w, const float *fc_b, float *logits,
               int N, int C, int classes, void *stream);

/*
 * A-GCN adaptive adjacency, models/a_gcn/a_gcn.py:53-63.  E holds the a_conv / b_conv embeddings of the three
 * subsets (channels [i*inter+k] = a_conv_i, [(3+i)*inter+k] = b_conv_i, biases included; produced by
 * csk_conv1x1_f32); element (n, ch, t, v) at
 * (n / seg_per_group)*e_group_stride + (n % seg_per_group)*e_seg_stride + ch*e_chan_stride + t*V + v
 * (clip: seg_per_group = n_seg, e_group_stride = 0; continual: a group = one channel-major frame (6*inter, P) of
 * the frames of a launch cycle, a segment = one skeleton of it, e_seg_stride = V, T = 1 -- per-frame attention,
 * models/coa_gcn/coa_gcn.py:11-14).  For every sample and subset:
 *     adj[i][v, w] = softmax_v( sum_{k,t} Ea[k,t,v] * Eb[k,t,w] / (inter*T) ) + a_sum[i][v, w],   a_sum = A + graph_attn
 * written as the dense column-wise ELL values ell_val[n][i][w][v] that csk_gcn_stage_f32 consumes with
 * ell_w = V, ell_cnt = {V,V,V}, adj_seg_stride = 3*V*V.
 * scratch: n_seg * 3 * 4 * V * V floats of partial logits (clip form, T > 1: the K = inter*T contraction is cut into 4
 * channel ranges per sample, summed in a fixed order); may be NULL for T == 1.  In the clip form E must be readable
 * 12 bytes past its last element (16-byte loads of the last partial row vector) and 4-byte aligned rows suffice.
 */
int csk_agcn_attention_f32(const float *E, const float *a_sum, float *ell_val, float *scratch, int n_seg, int inter, int T,
                           int V, int64_t e_seg_stride, int64_t e_chan_stride, int seg_per_group, int64_t e_group_stride,
                           void *stream);

/* The two entries above fused (no E tensor in memory): the six embedding 1x1 convs and the attention.
 * x: n_seg segments of `frames` frames (element (seg, c, frame, v) at seg*x_seg_stride + c*x_chan_stride + frame*V + v); w_pairs / b_pairs: the embedding weights packed as for csk_conv1x1_f32 ([C_in_pad][C_out_pad], C_out =
 * 6*inter) but in PAIR-MAJOR row order: rows i*2*inter + k = a_conv_i[k], i*2*inter + inter + k = b_conv_i[k].
 * per_frame = 1 (CoAGCN step form, models/coa_gcn/coa_gcn.py:11-14: the module applied per frame, T = 1; a segment is a
 *   channel-major slot, its "frames" are skeletons): one attention per (segment, frame), ell_val[(seg*frames + frame)][i][w][v].
 * per_frame = 0 (A-GCN clip form, models/a_gcn/a_gcn.py:53-63): one attention per segment over all frames, ell_val[seg][i][w][v];
 *   scratch: n_seg * 3 * ceil(frames / (128 / V)) * V * V floats (partial logits per tile of 128 / V frames, summed in tile order).
 * Built for V in {18, 25} and inter in {16, 32, 64}; fails otherwise (callers then use the two entries above).  Even V: rows
 * 8-byte aligned. */
int csk_agcn_embed_attention_f32(const float *x, const float *w_pairs, const float *b_pairs, const float *a_sum, float *ell_val,
                                 float *scratch, int n_seg, int c_in, int inter, int frames, int V, int per_frame,
                                 int64_t x_seg_stride, int64_t x_chan_stride, void *stream);

/*
 * The adaptive graph-conv stage applied PER FRAME to a clip tensor in one launch (csrc/agcn_framewise.hip): for every (segment,
 * frame) what csk_agcn_embed_attention_f32 (per_frame = 1) followed by csk_gcn_stage_f32 (adj_per_frame = 1) compute -- the step
 * form of the module, models/coa_gcn/coa_gcn.py:11-14 -- with the per-frame adjacencies kept in LDS / registers: the entry takes
 * no adjacency buffer.  With x_f = x[seg, :, f, :]:
 *     E_f = W_e x_f + b_e;   L_i[v, w] = sum_k Ea_i[k, v] Eb_i[k, w] / inter;   adj_i = softmax over v of L_i + a_sum_i
 *     y_f = ReLU( sum_i W'_i (x_f adj_i) + b' + gcn_residual(x_f) )
 * x, y, w, bias, strides, res_mode as csk_gcn_stage_f32; w_pairs, b_pairs, a_sum as csk_agcn_embed_attention_f32.  The softmax
 * arithmetic is that entry's; the aggregation sums even and odd joints in separate chains (csrc/gcn_dense.hip); the channel mix is
 * exact-fp32 MFMA.  A frame's result does not depend on `frames`, on its position or on the other frames (bitwise).  Results
 * differ from the two composed entries by fp32 summation order only.
 * Built for V in {18, 25}, inter in {16, 32, 64} with c_out == 4 * inter, any c_in (even V: rows 8-byte aligned); fails with a
 * message otherwise (callers then compose the two entries).
 */
int csk_agcn_stage_framewise_f32(const float *x, float *y, const float *w, const float *bias, const float *w_pairs,
                                 const float *b_pairs, const float *a_sum, int n_seg, int c_in, int c_out, int inter, int frames,
                                 int V, int64_t x_seg_stride, int64_t x_chan_stride, int64_t y_seg_stride, int64_t y_chan_stride,
                                 int res_mode, void *stream);
/* The instantiation agcn_stage_framewise_kernel<INTER, V, CONVRES> that call launches, as INTER * 1000 + V * 10 + CONVRES; 0 where
 * the shape is not built (the call fails); -1 (csk_last_error set) on bad dims.  Host arithmetic only (no GPU): of x only the
 * alignment is read.  The launcher switches on the function this entry reports. */
int csk_agcn_stage_framewise_f32_route(const float *x, int n_seg, int c_in, int c_out, int inter, int frames, int V,
                                       int64_t x_seg_stride, int64_t x_chan_stride, int res_mode);

/* ------------------------------------------------------------------------------------------------
 * Continual (frame-by-frame) path.  The arithmetic the reference delegates to the third-party package
 * continual-inference (co.Conv2d / co.Delay / co.Residual / co.AvgPool1d, call sites models/base.py:73-101,
 * 273-276, 307-334, 390-446) on per-module Python-side buffers runs here on a persistent HBM state slab in
 * CHANNEL-MAJOR layout: a frame of activations for all streams is a (C, P) matrix, P = streams*M*V positions
 * rounded up to a multiple of 4, joint innermost.  csk_gcn_stage_f32 handles the per-frame graph conv on that
 * layout (n_seg = 1, frames = streams*M, x_chan_stride = P).
 * ------------------------------------------------------------------------------------------------ */

/*
 * Emitting step(s) of CoTemporalConvolution (+ residual + ReLU of CoSpatioTemporalBlock, base.py:412-446).
 * For emission j = 0 .. n_emit-1 (n_emit > 1 batches the frames of a stride cycle; the kernel folds 2 or 4 emissions
 * into one workgroup tile when their count allows, so that one staged ring window serves all their taps):
 *     h_j   = (head + j*head_step) mod slots                       slot of the newest post-GCN frame
 *     out_j[co, p] = ReLU( sum_r sum_c W[r][c][co] * ring[(h_j-(k-1)+r) mod slots][c][p] + bias[co] + res_j[co, p] )
 *  ring   [slots][c][P] post-GCN frames; zero-initialised slots act as the clip conv's zero padding;
 *         slots >= k + (n_emit-1)*head_step.
 *  x_res  ring [x_res_slots][c_res][P] of block inputs or NULL; emission j pairs with slot
 *         (x_res_slot0 + j*x_res_step) mod x_res_slots = the input delayed by (k-1)/2 frames (co.Delay).
 *  out    ring [out_slots][c_out][P]; emission j is written to slot (out_slot0 + j) mod out_slots.
 *  All ring bases 16-byte aligned, P % 4 == 0.
 *  ksplit > 1: the channel axis is cut into up to ksplit ranges computed by separate workgroups into `partial`
 *  ([n_emit * ksplit][c_out][P] floats, 16-byte aligned) and summed in a fixed order by a second kernel that also
 *  applies bias / identity residual / ReLU.  Used in latency mode for few streams, where one workgroup per tile would walk
 *  the whole K loop alone (rounds 2-5 also split the 256-channel blocks in 3 in the default mode; the slot-balanced tiles of
 *  csrc/step16.hip made that unnecessary).  Results differ from ksplit = 1 by fp32
 *  summation order only; for a given ksplit they do not depend on n_emit or P.
 */
int csk_tcn_step_f32(const float *ring, int slots, int head, int head_step, int n_emit, const float *w,
                     const float *x_res, int x_res_slots, int x_res_slot0, int x_res_step,
                     const float *w_res, const float *bias, float *out, int out_slots, int out_slot0,
                     int c, int c_out, int64_t P, int k, int res_mode, int c_res, int relu, int ksplit, float *partial,
                     void *stream);

/*
 * The kernel csk_tcn_step_f32 picks for a launch shape: 0 = the 32x32x2 kernels of csrc/step.hip (split-K, k != 9, P < 8, a ring
 * of 4 GB or more), else the instantiation of the slot-balanced 16x16x4 step (csrc/step16.hip) as
 * NB * 1000 + E * 100 + HS * 10 + TAIL -- NB column blocks of 16 positions per tile (25 or 18), E emissions folded into a tile
 * (4, 2 or 1), HS the head_step the tile is built for, TAIL 1 when a channel count is not whole CSK_CPAD blocks.  Arguments as
 * the step's own; x_res_slots <= 0 stands for x_res == NULL.  Host arithmetic only (no GPU); -1 on bad dims.  For tests and
 * tools: only NB follows the launch size, and an output's summation order does not depend on it.
 */
int csk_tcn_step_f32_tile(int slots, int head_step, int n_emit, int x_res_slots, int out_slots, int c, int c_out, int64_t P,
                          int k, int res_mode, int c_res, int ksplit);

/*
 * The kernel csk_tcn_step_f32 launches for a launch shape -- the function the launcher switches on.  Arguments and argument checks
 * as csk_tcn_step_f32_tile's (-1 with the same message).
 *  route[0]  the family: 1 = the slot-balanced 16x16x4 step (csrc/step16.hip), 2 = the 32x32x2 step (csrc/step.hip)
 *  route[1]  the instantiation: family 1, csk_tcn_step_f32_tile's value (never 0 here); family 2,
 *            MT * 100000 + E * 10000 + HS * 1000 + SPLIT * 100 + K9 * 10 + OCC of tcn_step_kernel<MT, E, HS, SPLIT, K9, OCC> -- MT rows
 *            of a workgroup tile (128 when c_out_pad is a multiple of 128, else 64), E emissions folded into a tile (4, 2 or 1), HS
 *            the head_step the tile is built for, SPLIT 1 when the request leaves more than one channel range (followed by
 *            step_reduce_kernel), K9 1 for k == 9, OCC workgroups per CU (2; 3 = the 168-register twin of <64, 4, 1>)
 *  route[2]  family 2: the workgroups of that launch (-1: 2^31 or more, the entry refuses it as "grid too large"); family 1: 0
 * Host arithmetic only (no GPU).  For tests and tools: within family 2, E, HS and OCC follow the launch size and do not change an
 * output's summation order.
 */
#define CSK_STEP_ROUTE_WORDS 3
int csk_tcn_step_f32_route(int slots, int head_step, int n_emit, int x_res_slots, int out_slots, int c, int c_out, int64_t P,
                           int k, int res_mode, int c_res, int ksplit, int32_t *route);

/*
 * OPT-IN step precision "bf16x3" of csk_tcn_step_f32 (same reference method, models/base.py:307-334, 390-446; same rings,
 * slot arithmetic and arguments except the weights and the split-K pair, which this entry does not take): the 9 x 1 temporal
 * conv and the 1 x 1 conv residual of the emitting step(s) run on the bf16 matrix pipe with every fp32 operand split into
 * three bf16 pieces and the six piece products of order <= 2 accumulated in fp32 (v_mfma_f32_16x16x32_bf16; see
 * csk_tcn_stage_bf16x3) -- fp32-GRADE results, not the arithmetic of csk_tcn_step_f32.  The identity residual is added in
 * exact fp32 from the x_res ring; the output ring is fp32.  The ring is split when a slot is staged (no shadow state).  Never
 * selected implicitly: continual.set_step_precision(module, "bf16x3").  An output's summation order does not depend on
 * n_emit, P or the tile the launch picks.
 *  w_split      the image of csk_tcn_stage_bf16x3 packed for stride = head_step (fold.pack_conv_weight_split):
 *               [c_pad / 16][9 tap slots, class-major][3 pieces][2 channel halves][c_out_pad] vectors of 8 bf16
 *  w_res_split  [c_res_pad / 16][3 slots: tap 0, zero, zero][3][2][c_out_pad] (CSK_RES_CONV) or NULL
 *  k            must be 9; head_step 1 or 2; every ring below 4 GB; images 16-byte aligned
 */
int csk_tcn_step_bf16x3(const float *ring, int slots, int head, int head_step, int n_emit, const void *w_split,
                        const float *x_res, int x_res_slots, int x_res_slot0, int x_res_step,
                        const void *w_res_split, const float *bias, float *out, int out_slots, int out_slot0,
                        int c, int c_out, int64_t P, int k, int res_mode, int c_res, int relu, void *stream);

/*
 * The tile csk_tcn_step_bf16x3 picks for a launch shape: 16-position column blocks per workgroup (25 or 18 for an odd
 * n_emit, one emission per tile; 13 or 9 for an even one, two emissions per tile).  Host arithmetic only (no GPU); -1 on bad
 * dims.  For tests and tools: results do not depend on the tile.
 */
int csk_tcn_step_bf16x3_tile(int n_emit, int c_out, int64_t P);

/*
 * One CoSpatioTemporalBlock.forward_step cycle in one call (models/base.py:412-446): graph conv of the 4 new frames of
 * a stride cycle + the 4 emitting steps of the temporal conv + residual + ReLU -- csk_gcn_stage_f32 followed by
 * csk_tcn_step_f32 with n_emit = 4.  ONE launch where the slot-balanced tile family covers the shape (csrc/step16.hip:
 * identity gcn_residual, V dividing a tile of 100 or 72 positions (25, 18), c_out a multiple of 16, rings below 4 GB),
 * else that family's two launches: the same arithmetic in the same summation order, bit-identical results either way.
 * For blocks with c_out <= 64, temporal stride 1, k = 9, a skeleton-sparse adjacency (ell_cnt <= 1/1/4) and a block
 * residual that is absent (CSK_RES_NONE) or the identity; all 4 frames must emit (the block has seen >= 4 frames
 * before).  Arguments are checked before anything is launched (-1 and csk_last_error()).
 *  xin     block input ring [xin_slots][c_in][P]; new frame f = 0..3 in slot (xin_slot0 + f) mod xin_slots; the residual
 *          frame of emission j in slot (x_res_slot0 + j) mod xin_slots (the input delayed by 4 frames)
 *  y_ring  [y_slots][c_out][P] post-GCN frames, y_slots >= 12; new frame f is WRITTEN to slot (y_slot0 + f) mod y_slots,
 *          the temporal window of emission j is slots y_slot0 + j - 8 .. y_slot0 + j
 *  out     [out_slots][c_out][P]; emission j goes to slot (out_slot0 + j) mod out_slots
 *  n_skel  skeletons per frame (streams * M); P >= n_skel * V, a multiple of 4
 *  gcn_* / ell_* / tcn_*: the packed operands of csk_gcn_stage_f32 / csk_tcn_step_f32.
 */
int csk_co_block_step_f32(const float *xin, int xin_slots, int xin_slot0, int c_in, const float *gcn_w,
                          const float *gcn_bias, const int32_t *ell_src, const float *ell_val, const int32_t *ell_cnt,
                          int ell_w, int gcn_res_mode, float *y_ring, int y_slots, int y_slot0, const float *tcn_w,
                          const float *tcn_bias, int res_mode, int x_res_slot0, float *out, int out_slots, int out_slot0,
                          int c_out, int n_skel, int V, int64_t P, void *stream);

/*
 * A STACK of consecutive blocks of that kind in one launch (round 6): csk_co_block_step_f32 for block 0, then for block 1 on
 * block 0's output ring, ... -- n_blocks <= CSK_CO_STACK_MAX.  Block i + 1's `xin` must be block i's `out` (same slot counts),
 * its new frames the slots block i emits into.  A workgroup owns the same positions (whole skeletons) of the four frames
 * through every block: no workgroup depends on another (step mode has no temporal halo), stage outputs travel through the
 * state rings and L2.  Bitwise the results of the per-block calls.  Needs the slot-balanced tile family (csrc/step16.hip:
 * the shapes named at csk_co_block_step_f32); otherwise (or with one block) it issues the launches of the per-block calls.
 * Every block is checked as csk_co_block_step_f32 checks its arguments BEFORE anything is launched: an invalid block i
 * fails the call without the blocks in front of it having been launched.
 */
#define CSK_CO_STACK_MAX 4
typedef struct csk_co_block_args {          /* the arguments of csk_co_block_step_f32 that differ per block */
    const float *xin;
    int32_t xin_slots, xin_slot0, c_in;
    const float *gcn_w, *gcn_bias;
    const int32_t *ell_src;
    const float *ell_val;
    int32_t ell_cnt[3], ell_w, gcn_res_mode;
    float *y_ring;
    int32_t y_slots, y_slot0;
    const float *tcn_w, *tcn_bias;
    int32_t res_mode, x_res_slot0;
    float *out;
    int32_t out_slots, out_slot0, c_out;
} csk_co_block_args;
int csk_co_stack_step_f32(int n_blocks, const csk_co_block_args *blocks, int n_skel, int V, int64_t P, void *stream);

/*
 * What a csk_co_stack_step_f32 call (a csk_co_block_step_f32 call: n_blocks = 1) with these arguments launches -- the function the
 * launcher switches on.  Host arithmetic only: no GPU call, and of the blocks only their scalar fields are read (the ring and
 * operand pointers are checked as the entry checks them -- non-null, alignment, the chain -- and never dereferenced).  The same
 * argument checks as the entry: -1 with the same message.
 *  route[0]      1: the whole call is ONE launch of the fused stack kernel (csrc/step16.hip: co_stack16_kernel<NB>); 0: per block
 *  route[1]      NB of the call's fused launches, 25 or 18: tiles of 4 NB positions x the four new frames (0: it has none)
 *  route[2]      their grid, ceil(P / (4 NB)) workgroups (0: none)
 *  route[3 + i]  block i: 1 = carried by a fused launch (the one launch if route[0], else a launch of its own), 0 = the tile
 *                family's two stages (graph-conv launches per slot run, then the four emitting steps); -1 for i >= n_blocks
 */
#define CSK_CO_ROUTE_WORDS (3 + CSK_CO_STACK_MAX)
int csk_co_stack_step_f32_route(int n_blocks, const csk_co_block_args *blocks, int n_skel, int V, int64_t P, int32_t *route);

/* spatial_pool of CoModelBase (models/base.py:84) on a channel-major frame: feat[n, c] = mean of the MV = M*V
 * positions of stream n.  h (C, P); feat (N, C). */
int csk_co_spatial_pool_f32(const float *h, float *feat, int N, int C, int MV, int64_t P, void *stream);

/* co.AvgPool1d(window, stride 1) step (models/base.py:97): pooled = (1/window) * sum of the `count` newest
 * entries of ring [window][n_elem] (newest at slot `head`); missing entries count as zeros. */
int csk_co_window_mean_f32(const float *ring, float *pooled, int64_t n_elem, int window, int head, int count,
                           void *stream);

/* The three steps above and csk_fc_f32 in ONE launch (one workgroup per stream), bit-identical to issuing them one by one:
 * spatial_pool of frame h (NULL: a zero feature, the window's end padding) into pool_ring[head], then -- when `emit` --
 * pooled = window mean of the `count` newest entries and logits = pooled @ fc_w^T + fc_b.  pool_ring [window][N][C],
 * pooled [N][C], logits [N][classes]. */
int csk_co_head_step_f32(const float *h, float *pool_ring, float *pooled, const float *fc_w, const float *fc_b, float *logits,
                         int N, int C, int MV, int64_t P, int window, int head, int count, int emit, int classes, void *stream);

/* The continual head over a whole CLIP in one call: every prediction a fresh model stepped through the clip releases, from the
 * clip tensor of the last block.  h (N*M, C, t_src, V) contiguous; its frames 0 .. frames-1 are real, the
 * frames behind them are never read.  Entry j < frames of the pooling window is the spatial mean of frame j over the stream's
 * M*V positions, in the arithmetic and summation order of csk_co_head_step_f32's pool (the CSK_PRIME_POOL job of
 * csk_co_prime_pack_f32); entries >= frames are +0.0 (the window's end padding), entries < 0 do not exist.  Prediction
 * k = 0 .. n_pred-1 closes on entry e = first_entry + k: pooled[k] = (sum of entries max(0, e + 1 - window) .. e, oldest first)
 * / window -- csk_co_window_mean_f32's order, re-summed per prediction -- and logits[k] = pooled[k] @ fc_w^T + fc_b with
 * csk_fc_f32's four interleaved chains: bit for bit the composition pool job -> csk_co_window_mean_f32 per prediction ->
 * csk_fc_f32.  entries: caller-owned scratch [frames][N][C] (may be NULL when frames == 0), written by a pool kernel and read
 * by a window + FC kernel (one workgroup per stream and group of 16 predictions), both issued by this call; pooled
 * [n_pred][N][C], logits [n_pred][N][classes].  Checked on the host before anything is launched (-1, csk_last_error): null
 * or misaligned pointers (4 bytes; pooled and fc_w 16 bytes when C % 4 == 0, csk_fc_f32's rule), a dim < 1, frames outside
 * 0..t_src, window < 1, first_entry < 0, n_pred < 0; limits of this form: C <= 8192, window <= 8192 - 15, N <= 65535.
 * n_pred == 0 launches nothing. */
int csk_co_head_clip_f32(const float *h, int t_src, int frames, float *entries, int window, int first_entry, int n_pred,
                         const float *fc_w, const float *fc_b, float *pooled, float *logits, int N, int M, int C, int V,
                         int classes, void *stream);

/* csk_input_norm_f32 for the r = 1..8 frames of a launch cycle in one launch (continual form, T = 1): frames[f] (N, C, V, M)
 * -> dst[f] channel-major (C, P) (models/base.py:73-82).  frames / dst are HOST arrays of device pointers. */
int csk_input_norm_frames_f32(const float *const *frames, float *const *dst, int r, const float *scale, const float *shift,
                              int N, int C, int V, int M, int64_t P, void *stream);

/*
 * Bone / motion input modalities derived from the joint tensor (the reference derives them offline over whole datasets:
 * datasets/data_preparation/bone_data_prep.py:158-163, motion_data_prep.py:28-30).  x (N, C, T, V, M) as the models take
 * it; p(v) = parents[v], the 0-based parent joint, p(root) = root.  All C channels alike.  Every subtraction below is one
 * fp32 rounding, in the order written, so the result equals the reference's numpy arithmetic bit for bit:
 *   CSK_MODALITY_BONE          b[t, v] = x[t, v] - x[t, p(v)]                      (both read from the original x)
 *   CSK_MODALITY_JOINT_MOTION  m[t] = x[t+1] - x[t] for t < T-1,  m[T-1] = 0
 *   CSK_MODALITY_BONE_MOTION   (x[t+1, v] - x[t+1, p(v)]) - (x[t, v] - x[t, p(v)]) for t < T-1,  0 at T-1
 * (CSK_MODALITY_JOINT names the input itself: nothing to derive, the entries refuse it.)
 * parents is a HOST array of V ints (may be NULL for CSK_MODALITY_JOINT_MOTION): the entry refuses an index outside
 * [0, V) before it launches anything -- which it could not do without a synchronisation if the table lived on the
 * device -- and hands the table to the kernel by value.  out: same shape as x, another buffer.  One pass, 16-byte
 * accesses when x and out are 16-byte aligned.  V <= 64, V * M <= 512.
 * Returns -2 (csk_last_error set, nothing launched) for an unknown mode or a parent index outside [0, V).
 */
#define CSK_MODALITY_JOINT 0
#define CSK_MODALITY_BONE 1
#define CSK_MODALITY_JOINT_MOTION 2
#define CSK_MODALITY_BONE_MOTION 3
int csk_derive_modality_f32(const float *x, float *out, int mode, const int32_t *parents, int N, int C, int T, int V, int M,
                            void *stream);

/*
 * The same for the r = 1..8 frames of a launch cycle of the continual path in one launch, in the causal (backward) form
 *   m'[s] = x[s] - x[s-1],  0 on a stream's first frame        (m'[s] = m[s-1] of the clip form)
 * frames[i] (N, C, V, M) -> dst[i], same shape; frames / dst are HOST arrays of device pointers, as for
 * csk_input_norm_frames_f32; every dst[i] is a buffer of its own.  Frame i >= 1 is differenced against frame i-1 of the
 * cycle, frame 0 against prev (N, C, V, M), the raw (joint) frame the last updating call ended with; a stream n whose
 * has_prev[n] is 0 gets 0 for frame 0 (int32 per stream, on the device).  update != 0: the launch then stores frames[r-1]
 * into prev and sets has_prev[n] = 1 for all n -- after every read of them, by the workgroup that read them; update == 0
 * leaves both bitwise untouched (forward_step(update_state=False)).  CSK_MODALITY_BONE has no state: prev / has_prev are
 * not used (may be NULL).  parents, modes and limits as above.  No allocation, no synchronisation, graph-capture safe.
 * Returns -2 (csk_last_error set, nothing launched) for an unknown mode, a parent index outside [0, V), or r outside 1..8.
 */
int csk_derive_modality_frames_f32(const float *const *frames, float *const *dst, int r, int mode, const int32_t *parents,
                                   float *prev, int32_t *has_prev, int update, int N, int C, int V, int M, void *stream);

/*
 * Pre-normalisation of raw joint frames (the reference runs it offline over whole datasets:
 * datasets/data_preparation/preprocess.py:14-93 from ntu60_prep.py:179 / ntu120_prep.py:219; rotation.py:10-50).
 * x (N, 3, T, V, M): C = 3 coordinate channels, persons m, joints v; the main body is m = 0, the centre joint is joint 1.
 * Per sample, every frame t:
 *   1. null mask   joint (t, v, m) is null iff (x0 + x1) + x2 == 0 in fp32; a null joint comes out as +0 in all channels
 *   2. centre      c[t] = x[t, joint 1, person 0];  s1 = x - c[t]            (one fp32 rounding per channel, every person)
 *   3. z-rotation  d = s1[0, zaxis1, 0] - s1[0, zaxis0, 0]                   (fp32, frame 0, person 0; s1 of a null joint is 0)
 *                  axis = d x (0,0,1), angle = acos(clip(d/|d| . (0,0,1))), Rz = the quaternion form of rotation.py:10-29 with
 *                  its identity shortcuts (sum|axis| < 1e-6, |angle| < 1e-6; angle = 0 for sum|d| < 1e-6) -- all in fp64
 *                  s2 = fp32(Rz . fp64(s1))                                  (three-term fp64 dot, one rounding to fp32)
 *   4. x-rotation  the same from d' = s2[0, xaxis0, 0] - s2[0, xaxis1, 0] against (1,0,0):  out = fp32(Rx . fp64(s2))
 * The rounding to fp32 between the two rotations is part of the definition (the reference stores each stage into its fp32
 * array).  The reference takes the unit vector d/|d| in fp32, so it is matched to ~1 fp32 ulp, not bit for bit.
 * Deliberately NOT reproduced:
 *   - the reference's first step (preprocess.py:18-39) pads null frames by compacting and repeating earlier frames; it looks
 *     ahead, which a causal stream cannot do, and the clip form leaves it out too so that clip and step form agree;
 *   - the reference's `== 0` tests on whole-person / whole-frame sums also fire when non-zero coordinates cancel exactly;
 *     here only all-zero data is skipped, where the result is the same up to the sign of zero;
 *   - a sample / stream whose first frame has an empty main body latches the identity (reset the stream when a body appears).
 * The reference's defaults are zaxis = (0, 1), xaxis = (8, 4).  out: same shape as x, another buffer.  One launch, no
 * allocation, no synchronisation, no scratch, graph-capture safe.
 * Returns -1 for a null pointer, out == x or a dim < 1; -2 for V < 2 or a joint index outside [0, V) (csk_last_error set,
 * nothing launched).
 */
int csk_prenorm_f32(const float *x, float *out, int N, int T, int V, int M, int zaxis0, int zaxis1, int xaxis0, int xaxis1,
                    void *stream);

/*
 * The same for the r = 1..8 frames of a launch cycle of the continual path in one launch.  The centring is per frame and so
 * causal; the two matrices are latched from a stream's FIRST frame: rot (N, 18) fp64 holds a stream's Rz then Rx (row-major),
 * has_rot (N,) int32 says whether it does (both on the device).  frames[i] (N, 3, V, M) -> dst[i], same shape; frames / dst
 * are HOST arrays of device pointers, as for csk_derive_modality_frames_f32; every dst[i] is a buffer of its own.  A stream
 * with has_rot == 0 computes both matrices from frames[0] -- exactly as csk_prenorm_f32 does from frame 0 of a clip, so the
 * two forms agree bit for bit -- and uses them for all r frames.  update != 0: the launch then stores them into rot and sets
 * has_rot -- behind a workgroup barrier, by the workgroup that read them (a workgroup owns whole streams); update == 0
 * leaves both bitwise untouched (forward_step(update_state=False)).
 * Returns -1 for a null pointer (frames, dst, a frame, rot, has_rot), a dim < 1 or a dst that is a source frame; -2 for r
 * outside 1..8, V < 2 or a joint index outside [0, V) (csk_last_error set, nothing launched).
 */
int csk_prenorm_frames_f32(const float *const *frames, float *const *dst, int r, double *rot, int32_t *has_rot, int update, int N,
                           int V, int M, int zaxis0, int zaxis1, int xaxis0, int xaxis1, void *stream);

/*
 * Kinetics keypoint intake (csrc/keypoints.hip): the arithmetic of the reference's offline Feeder_kinetics.__getitem__
 * (datasets/data_preparation/kinetics400_prep.py:100-138) on the device.  k (N, T, P, V, 3) -> out (N, 3, T, V, M):
 * k[n, t, p, v, :] = (x, y, s), the P people a pose estimator found in a frame, their V joints and per joint the two image
 * coordinates in [0, 1] and the confidence score -- the reference's pose[0::2], pose[1::2] and score, person-major.
 * Per (sample, frame), on its own (so the operation is causal and has no state):
 *   1. S[p] = sum over v of s[p, v], accumulated in fp64 with v ascending (the reference sums in fp64; for fp32 scores the sum
 *      is exact over any realistic range, so the order does not hang on rounding)
 *   2. person p is placed before person q iff S[p] > S[q], or the two compare equal and p < q; a NaN sum goes behind every
 *      number, NaN sums among themselves by index.  (numpy.argsort of -S, the reference's, agrees wherever the sums of the
 *      people present are distinct; its order of ties is platform dependent, this one is fixed.)
 *   3. for m < M, with p = order[m], per joint v:
 *        out[0] = (s == 0) ? +0.0f : x - 0.5f
 *        out[1] = (s == 0) ? +0.0f : -(y - 0.5f)       subtracted, then negated: y == 0.5 with a score gives -0.0, as the
 *        out[2] = s                                     reference's; 0.5f - y would give +0.0
 *      The zeroing is per joint (a score of -0.0 counts as 0) and does not enter S.
 * Limits: 1 <= M <= P <= 8, 1 <= V <= 64.  out is another buffer than k.  One launch, no allocation, no synchronisation, no
 * scratch, graph-capture safe.  Not reproduced: reading the estimator's JSON, and datasets/tools.py:openpose_match (tracking
 * people across frames), which the reference's pipeline does not call.
 * Returns -1 for a null pointer, out == k or a dim < 1; -2 for a violated limit (csk_last_error set, nothing launched).
 */
int csk_select_people_f32(const float *k, float *out, int N, int T, int P, int V, int M, void *stream);

/*
 * The same for the r = 1..8 frames of a launch cycle of the continual path in one launch: frames[i] (N, P, V, 3) -> dst[i]
 * (N, 3, V, M); frames / dst are HOST arrays of device pointers, as for csk_prenorm_frames_f32; every dst[i] is a buffer of
 * its own.  The arithmetic per (stream, frame) is csk_select_people_f32's, bit for bit.
 * Returns -1 for a null pointer (frames, dst, a frame), a dim < 1 or a dst that is a source frame or another dst; -2 for r
 * outside 1..8 or a violated limit (csk_last_error set, nothing launched).
 */
int csk_select_people_frames_f32(const float *const *frames, float *const *dst, int r, int N, int P, int V, int M, void *stream);

/*
 * NTU RGB+D body intake for WHOLE CLIPS (csrc/ntu_intake.hip): what the reference's offline pipeline does to a
 * recorded Kinect clip before it centres and rotates it -- read_xyz's choice of the max_body_true bodies with the largest motion
 * energy (datasets/data_preparation/ntu60_prep.py:101-128), gendata's placement into max_frame frames (:169-177) and the
 * null-frame padding that opens pre_normalization (preprocess.py:18-39).  csk_prenorm_f32 on the result is the rest of that
 * function.  bodies (N, T, P, V, 3) -> out (N, 3, T_out, V, M): bodies[n, t, p, v, :] = (x, y, z) of joint v of the sensor's body
 * slot p; a frame in which a body is not tracked is all zero (as read_xyz leaves it).  Per clip, on its own:
 *   a. a frame of a body is NULL iff all its V * 3 values are +-0.  (The reference tests `sum == 0`, which also fires when
 *      non-zero values cancel exactly; only all-zero data is acted on here, as in csk_prenorm_f32.)
 *   b. E[p] = sum over the 3 coordinates of the population standard deviation (ddof 0) of that coordinate over (the body's
 *      non-null frames x V); 0 for a body without a non-null frame.  fp64 from the fp32 values, two passes (the mean, then the
 *      squared deviations), in a summation order that is a function of (T, V) only: bodies with the same data get the same
 *      bits whatever their slot, and a clip's result does not depend on N or on its place in the batch.
 *   c. output person m is the body of rank m by descending E; equal energies: the HIGHER slot first (numpy's
 *      energy.argsort()[::-1], the reference's).  A NaN energy goes behind every number.
 *   d. with b = the body of person m: an empty body gives +0 everywhere.  Frame 0 non-null: L = index of the last non-null
 *      frame + 1, src(t) = t mod L (null frames inside stay null).  Frame 0 null: idx[0..L-1] = the non-null frames in order,
 *      src(t) = idx[t mod L].  out[n, c, t, v, m] = bodies[n, src(t), b, v, c] for t in [0, T_out): a late body is moved to
 *      the front, a short clip is filled by repeating itself.  Frames >= T of the input count as null.
 *   e. NaN coordinates are outside the contract (the reference's own result then hangs on `person *= 0` leaving NaN behind);
 *      the kernel takes every index from the null flags, so it stays inside its operands and the other clips keep their bits.
 * The padding looks ahead: there is no frames form, the continual path cannot run it (prepare a history for priming with it).
 * Limits: 1 <= M <= P <= 8, 1 <= V <= 64, T <= T_out <= CSK_NTU_MAX_FRAMES (the reference's max_frame is 300).  out is another
 * buffer than bodies.  One launch (one workgroup per clip), no allocation, no synchronisation, no scratch, graph-capture safe.
 * Returns -1 for a null pointer, out == bodies or a dim < 1; -2 for a violated limit (csk_last_error set, nothing launched).
 */
#define CSK_NTU_MAX_FRAMES 1024
int csk_ntu_intake_f32(const float *bodies, float *out, int N, int T, int P, int V, int M, int T_out, void *stream);

/*
 * Multi-stream logit fusion + top-k support, scripts/multi_stream_eval.py:33-60: fused = left fold of add
 * (use_max = 0) or maximum (1) over n_streams <= 4 prediction arrays (host array of device pointers); element
 * (n, c) of every array at n*sample_stride + c*class_stride (a (N, classes, steps) array with the reference's
 * `preds[:, :, 0]` selection has sample_stride = classes*steps, class_stride = steps).  Outputs (either may be
 * NULL): fused (N, classes) contiguous; rank[n] = number of classes scoring strictly higher than targets[n]
 * (top-k hit <=> rank < k; out-of-range targets give rank = classes).
 */
int csk_fuse_rank_f32(const float *const *preds, int n_streams, int use_max, int N, int classes,
                      int64_t sample_stride, int64_t class_stride, const int64_t *targets, float *fused, int *rank,
                      void *stream);

/* ------------------------------------------------------------------------------------------------
 * Native step executor ("plan"): the counterpart of co.Sequential.forward_step driving the ten continual
 * blocks and the head (models/base.py:108-122,183-190) -- one C call issues every launch of a cycle of 1..8
 * frames (input norm, per block one GCN-stage + one multi-emission TCN-step launch, spatial pool, temporal
 * window mean, FC).  The plan holds operands and geometry only: the stepping position (the counters every ring slot and
 * stride phase follows from) belongs to the caller and is handed to each csk_co_plan_cycle call.  No device allocation, no sync.
 * ------------------------------------------------------------------------------------------------ */
#define CSK_CO_MAX_CYCLE 8
/* Ring depths are per layer (csk_co_layer.y_slots / .out_slots, csk_co_plan_create xin0_slots), derived from the frames ONE
 * launch of the layer can receive (max_in = CSK_CO_MAX_CYCLE / cumulative stride of the layers in front of it):
 *   post-GCN ring   : the (k-1) = 8 window frames of co.Conv2d + the new frames      -> CSK_CO_Y_SLOTS(max_in)
 *   input history   : residual lag (k-1)/2 = 4 (co.Delay / residual_shrink) + the new frames -> CSK_CO_IN_SLOTS(max_in);
 *                     a layer's output ring IS the next layer's input history, so out_slots(l) = CSK_CO_IN_SLOTS(max_in(l+1))
 *                     (last layer: at least its own emissions per launch; csk_co_block_step_f32 wants >= 4).
 * A frame s lives in slot s % depth of its ring.  Deeper rings are accepted. */
#define CSK_CO_Y_SLOTS(max_in) (8 + (max_in))
#define CSK_CO_IN_SLOTS(max_in) (4 + (max_in))

typedef struct csk_co_layer {
    int32_t c_in, c_out, stride, res_kind;   /* res_kind: CSK_RES_NONE / IDENTITY / CONV (block residual) */
    int32_t gcn_res_mode, ell_w, ell_cnt[3];
    int32_t tcn_ksplit;                      /* split-K of the TCN step (csk_tcn_step_f32); 1 = off               */
    int32_t y_slots, out_slots;              /* depths of y_ring / out_ring (see CSK_CO_Y_SLOTS / CSK_CO_IN_SLOTS)  */
    int32_t partial_emits;                   /* emissions the split-K scratch holds (0 when tcn_ksplit == 1)       */
    int32_t agcn_adj_frames;                 /* frames of per-skeleton adjacencies agcn_adj holds (0: no adaptive graph conv) */
    int32_t gcn_ksplit, gcn_partial_frames;  /* split-K of the graph conv (csk_gcn_stage_splitk_f32, latency mode); <= 1 = off.  Its
                                              * partial sums go to tcn_partial as well (launches are stream-ordered), which then
                                              * holds gcn_partial_frames * gcn_ksplit * c_out * P floats: the frames ONE graph-conv
                                              * launch may cover (more frames in a cycle fail with an error) */
    const float *gcn_w, *gcn_bias;           /* packed operands of csk_gcn_stage_f32                       */
    const int32_t *ell_src;
    const float *ell_val;
    const float *tcn_w, *tcn_w_res, *tcn_bias; /* packed operands of csk_tcn_step_f32                      */
    float *y_ring;                           /* [y_slots][c_out][P]                                        */
    float *out_ring;                         /* [out_slots][c_out][P]; input history of the next layer     */
    float *tcn_partial;                      /* [partial_emits * tcn_ksplit][c_out][P] or NULL (tcn_ksplit == 1): raw partial sums
                                              * of the emissions ONE launch of this layer produces (may be shared by all
                                              * layers: launches are stream-ordered); a cycle whose launch would emit more
                                              * fails with an error instead of overrunning it */
    /* adaptive graph conv (CoAGCN, models/coa_gcn/coa_gcn.py:11-14); agcn_inter == 0: plain GraphConvolution.  Otherwise the
     * layer's adjacency is computed per skeleton frame by csk_agcn_embed_attention_f32 (per-frame form) into agcn_adj
     * ([agcn_adj_frames * skeletons][3][V][V] floats, may be shared by all layers: launches are stream-ordered) and ell_src /
     * ell_w / ell_cnt describe the dense pattern (ell_w = V, ell_cnt = {V, V, V}); ell_val is not used. */
    int32_t agcn_inter, agcn_pad_;
    const float *agcn_w_pairs, *agcn_b_pairs, *agcn_a_sum;
    float *agcn_adj;
} csk_co_layer;

typedef struct csk_co_plan csk_co_plan;

/* xin0: [xin0_slots][C][P] input ring of layer 0.  xin0_slots = CSK_CO_IN_SLOTS(max_cycle) fixes the largest cycle the plan
 * accepts (max_cycle = xin0_slots - 4, at most CSK_CO_MAX_CYCLE); every layer's rings are checked against it (max_in above
 * with max_cycle in the place of CSK_CO_MAX_CYCLE): a slab for 4-frame cycles is 19 % smaller than one for 8-frame cycles.
 * pool_ring: [pool_size][N][feat_c]; pooled: [N][feat_c]. */
csk_co_plan *csk_co_plan_create(int n_layers, const csk_co_layer *layers, float *xin0, int xin0_slots, int N, int C, int V, int M,
                                int64_t P, const float *bn_scale, const float *bn_shift, int classes,
                                const float *fc_w, const float *fc_b, int pool_size, int pool_padding,
                                float *pool_ring, float *pooled);
void csk_co_plan_destroy(csk_co_plan *plan);
/* swap in refolded weights (same geometry and state rings); the plan holds no stepping state, so none is touched */
int csk_co_plan_update_weights(csk_co_plan *plan, int n_layers, const csk_co_layer *layers, const float *bn_scale,
                               const float *bn_shift, const float *fc_w, const float *fc_b);
/* 1 (default): blocks that qualify advance a 4-frame cycle with one csk_co_block_step_f32 launch instead of a
 * csk_gcn_stage_f32 + csk_tcn_step_f32 pair (bit-identical results); 0: always the two-launch form. */
int csk_co_plan_set_fusion(csk_co_plan *plan, int enable);
/* Per-layer emission delay k - 1 - padding of the blocks' temporal convs: layer i emits nothing during its first delays[i]
 * steps.  A new plan has 4 in every layer (padding "equal", CoST-GCN); the unpadded "*" stacks (CoST-GCN*, padding 0) set 8.
 * The residual lag stays (k - 1) / 2 = 4 in both families (co.Delay / the centred residual shrink), and so do the ring depths:
 * an emission reads the k - 1 post-GCN frames behind it and the input frame 4 behind it whatever the delay.  delays is a HOST
 * array of n_layers values in [4, 8]; it lives in the plan's own layer description (csk_co_layer is unchanged). */
int csk_co_plan_set_delays(csk_co_plan *plan, int n_layers, const int32_t *delays);
/* Advance by r = 1..CSK_CO_MAX_CYCLE frames, frames[i] = (N, C, V, M) device pointers.  On return
 * *last_slot / *n_feat describe the last layer's emissions of this cycle (slot of the first, count) and
 * *n_logits how many predictions were written to `logits` ([CSK_CO_MAX_CYCLE][N][classes], slice j = prediction j).
 * counters = the caller's stepping position, {frames, features, then (received, emitted) per layer}, n_counters =
 * 2 + 2*n_layers values >= 0 (all zero = clean state, models/base.py:161-164).  Read on entry and advanced when the call
 * returns 0; on any other return, after any number of launches, it is exactly what was passed in.  A step only overwrites
 * ring slots whose content is older than any window, so the counters are the whole state of a single step:
 * forward_step(x, update_state=False) (models/base.py:183-185) = run the cycle on a copy. */
int csk_co_plan_cycle(csk_co_plan *plan, int64_t *counters, int n_counters, const float *const *frames, int r, float *logits,
                      int *last_slot, int *n_feat, int *n_logits, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Per-stream reset of the continual slab: zero the state of SOME of the N streams that share the rings, leaving every
 * other stream -- and the P-padding behind the last one -- untouched.  A job names a ring and a run of n_slots slots
 * starting at slot0, taken modulo the ring depth:
 *   CSK_SCRUB_BLOCK_RING  ring [depth][rows][row_floats] (xin0, a layer's y_ring / out_ring: rows = channels, row_floats = P);
 *                         stream n owns floats [n * seg, (n + 1) * seg) of every row (seg = M * V)
 *   CSK_SCRUB_POOL_RING   ring [depth][rows][row_floats] with rows = N and seg = row_floats = feat_c (pool_ring): stream n
 *                         owns row n
 * One launch covers up to CSK_CO_SCRUB_MAX_JOBS jobs (a whole model is 21 block rings and the pooling ring) for the
 * n_streams indices of the DEVICE array `streams` (values in [0, n_total), n_total = N; an index outside writes nothing).
 * jobs is a HOST array.  The same entry serves the full reset (every slot of every ring) and the per-cycle scrub of a
 * warming stream (the slots one cycle wrote; co_reset.py).  Segments need 4-byte alignment only; the store width follows
 * the address.  n_streams == 0 and empty runs (n_slots == 0) are accepted and launch nothing.
 * ------------------------------------------------------------------------------------------------ */
#define CSK_CO_SCRUB_MAX_JOBS 24
#define CSK_SCRUB_BLOCK_RING 0
#define CSK_SCRUB_POOL_RING 1
typedef struct csk_scrub_job {
    float *ring;
    int64_t row_floats;
    int32_t depth, rows, slot0, n_slots, seg, kind;
} csk_scrub_job;
int csk_co_scrub_streams_f32(const csk_scrub_job *jobs, int n_jobs, const int32_t *streams, int n_streams, int n_total,
                             void *stream);

/* ------------------------------------------------------------------------------------------------
 * Moving live streams between slabs: the copying counterpart of csk_co_scrub_streams_f32.  One launch gathers (to_ring = 0,
 * export) the state of SOME streams of a slab into a packed, position-independent buffer, or scatters it back (to_ring = 1,
 * import) into the same or another slab.  A job names a ring as a scrub job does (kind, depth, rows, row_floats, seg), and
 *   newest   the slot of the ring's newest live frame / emission: its frame number modulo the depth
 *   window   how many newest slots move (0 <= window <= depth; 0 moves nothing)
 *   offset   where the job's floats start inside one stream's record
 * packed is a DEVICE buffer of n_streams records of record_floats floats each; record j pairs with stream streams[j] (a
 * DEVICE array; an index outside [0, n_total) moves nothing and leaves record j alone).  Inside a record a job's floats are
 * [window slot, OLDEST first][row][seg]: neither the ring depth nor the slot position, N or the P padding of a slab appears in
 * it, so a record exported from one slab imports into a slab with other depths, positions and stream counts.  An import writes
 * the named streams' segments in the window's slots and nothing else.  Words are moved as 32-bit patterns: per-stream int32
 * flags (seg = 1) and fp64 values (seg = 2 per value) travel as block rings of one slot and one row.  jobs is a HOST array;
 * every job's [offset, offset + window * rows * seg) must lie inside the record and the caller keeps them disjoint.  One launch
 * covers up to CSK_CO_MOVE_MAX_JOBS jobs: a whole model is 21 rings plus up to four small per-stream states, more than
 * CSK_CO_SCRUB_MAX_JOBS, so this entry has a limit of its own.  Buffers need 4-byte alignment only; the access width follows
 * the addresses.  n_streams == 0 launches nothing.
 * ------------------------------------------------------------------------------------------------ */
#define CSK_CO_MOVE_MAX_JOBS 32
typedef struct csk_move_job {
    void *ring;
    int64_t row_floats;
    int64_t offset;
    int32_t depth, rows, newest, window, seg, kind;   /* kind: CSK_SCRUB_BLOCK_RING / CSK_SCRUB_POOL_RING */
} csk_move_job;
int csk_co_move_streams_f32(const csk_move_job *jobs, int n_jobs, void *packed, int64_t record_floats, const int32_t *streams,
                            int n_streams, int n_total, int to_ring, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Priming streams from buffered history: write the packed records csk_co_move_streams_f32 imports -- the same layout, job by
 * job -- from the tensors of a CLIP pass over the streams' history instead of from a slab (co_prime.py).  One
 * launch; record k of packed ([n_streams][record_floats], device) belongs to stream k of every source.  A job names
 *   kind     CSK_PRIME_RING   src = clip tensor (n_streams * M, rows, t_src, V) contiguous: the job's floats are
 *                             [frame first + i, i = 0 .. window - 1][row][m * V + v], window * rows * M * V per stream -- what
 *                             a ring job of csk_co_move_streams_f32 holds for a ring whose frame j is clip frame j.  A frame
 *                             index < 0 (first may be negative) is written as +0.0, the zero state of a fresh model's ring.
 *                             Words travel as 32-bit patterns.
 *            CSK_PRIME_POOL   src as above (the last layer's output): entry i is the spatial mean of frame first + i over the
 *                             stream's M * V positions, rows floats per entry, window * rows per stream, in the arithmetic
 *                             and summation order of csk_co_head_step_f32's pool (bit for bit its ring entry for the same
 *                             feature frame); a frame index < 0 gives +0.0.
 *            CSK_PRIME_WORDS  src = [n_streams][rows] 32-bit words (flags, fp64 halves, a raw frame): copied as they are;
 *                             first = 0, t_src = 1, window = 1 (0: nothing)
 *   offset   where the job's floats start inside one stream's record
 * jobs is a HOST array of 1..CSK_CO_MOVE_MAX_JOBS jobs.  Checked on the host before anything is launched (csk_last_error
 * set, -1): the job count, null and misaligned (4-byte) pointers, dims < 1, window < 0, first + window > t_src (no frame
 * behind the source is ever read), offset < 0 or offset + size > record_floats.  The caller keeps the jobs disjoint.  Buffers
 * need 4-byte alignment only; the stores are 16 bytes wide behind the leading unaligned words of a job's run.  n_streams == 0
 * and empty windows launch nothing.
 * ------------------------------------------------------------------------------------------------ */
#define CSK_PRIME_RING 0
#define CSK_PRIME_POOL 1
#define CSK_PRIME_WORDS 2
typedef struct csk_prime_job {
    const void *src;
    int64_t offset;
    int32_t kind, rows, t_src, first, window, pad_;
} csk_prime_job;
int csk_co_prime_pack_f32(const csk_prime_job *jobs, int n_jobs, void *packed, int64_t record_floats, int n_streams, int M, int V,
                          void *stream);

/*
 * S-TR spatial-attention graph unit (GcnUnitAttention, models/s_tr/s_tr.py:303-477, in the configuration STr / CoSTr build:
 * only_attention, no relative / adjacency / more_channels, data_bn, skip, BN; Nh = 8, dk = C_out / 4, dv = C_out).  Per
 * frame (seg, f) of x:
 *     x^ = s_in[c, v] x + t_in[c, v]                      (data_bn, BatchNorm1d over c*V + v)
 *     [q; k; v] = w_qkv^T x^ + b_qkv                      (qkv_conv; q rows pre-scaled by dkh^-0.5)
 *     o[h dvh + d, i] = sum_j softmax_j(sum_e q[h dkh + e, i] k[h dkh + e, j]) v[h dvh + d, j]     (8 heads)
 *     y = ReLU(w_out^T o + b_out (+ res_scale[c] x[c]))   (attn_out with BN folded in; the skip when C_in == C_out)
 * Element (seg, c, f, v) of x / y at seg * seg_stride + c * chan_stride + f * V + v: the clip layout (seg = sample, chan
 * stride = T V, frames = T) and the continual channel-major ring slots (seg = slot, chan stride = P, frames = skeletons).
 *  w_qkv    packed [c_in][Mq], Mq = 2 dk + dv rounded up to 64, zero columns beyond 2 dk + dv; b_qkv [Mq]   (16-B aligned)
 *  s_in / t_in  [c_in][V]
 *  w_out    packed [c_out][Mo], Mo = c_out rounded up to 64; b_out [Mo]; res_scale [c_out] or NULL (no skip)
 *  scratch  >= n_seg * (2 dk + 2 dv) * frames * V floats (scratch_floats): the qkv and attention-output images.  Their layout is
 *           part of the contract (the stage-wise tests read both): both dense, rows of frames * V columns,
 *             qkv [n_seg][2 dk + dv][frames V] at offset 0 (rows: dk of q, dk of k, dv of v; head h owns q / k rows
 *                                                           h dkh .. and v rows h dvh .., dkh = dk / 8, dvh = dv / 8)
 *             o   [n_seg][dv][frames V]        at offset n_seg (2 dk + dv) frames V
 *           every element of both images is written by every call; nothing beyond n_seg (2 dk + 2 dv) frames V floats is touched.
 * Three launches (data_bn + QKV GEMM, attention, output GEMM + epilogue); fp32 MFMA for both GEMMs, exact fp32 throughout.
 * Returns -2 for shapes not built: V not in {18, 25}, C_out not in {32, 64, 128, 256}, C_in not a multiple of 16.
 */
int csk_str_unit_f32(const float *x, float *y, float *scratch, int64_t scratch_floats, const float *w_qkv,
                     const float *b_qkv, const float *s_in, const float *t_in, const float *w_out, const float *b_out,
                     const float *res_scale, int n_seg, int c_in, int c_out, int frames, int V, int64_t x_seg_stride,
                     int64_t x_chan_stride, int64_t y_seg_stride, int64_t y_chan_stride, void *stream);

/*
 * What the three launches of csk_str_unit_f32 run for a shape (has_res: res_scale != NULL).  Host arithmetic only, no GPU call:
 * the function the launchers switch on.  route[CSK_STR_ROUTE_WORDS]:
 *   [0..3]   QKV GEMM (data_bn at staging, M = 2 dk + dv rows): MI (tile rows = 32 MI), row tiles, column tiles (256 columns), grid
 *   [4..6]   attention: V, DKH, grid (= n_seg * frames, one frame per workgroup)
 *   [7..11]  output projection (M = c_out rows): RES (the skip is fused), MI, row tiles, column tiles, grid
 * grid = row tiles * column tiles * n_seg; workgroup id -> (row tile fastest, column tile, segment) after the XCD remap.
 * Returns 0, or the value csk_str_unit_f32 returns for the same (n_seg, c_in, c_out, frames, V, has_res): -1 / -2.
 */
#define CSK_STR_ROUTE_WORDS 12
int csk_str_unit_f32_route(int n_seg, int c_in, int c_out, int frames, int V, int has_res, int32_t *route);

#ifdef __cplusplus
}
#endif
#endif /* CSKEL_H */
