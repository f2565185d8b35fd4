// executor.hip -- native step executor for the continual stack (host code only; launches go through the C ABI
// entry points of gcn.hip / step.hip / head.hip).  Mirrors continual.py:CoSpatioTemporalBlock.engine_advance and
// CoStGcn._python_cycle / _head_step one to one; the Python versions remain the reference for the protocol.  The stepping
// position (frames, features, per-layer received / emitted) belongs to the caller: a cycle works on a copy of the caller's
// counters and stores it back when every launch of the cycle was issued, so either driver can run any cycle.
#include <vector>

#include "mfma_core.h"

struct BlockCounters {
    int64_t s;   // frames received
    int64_t e;   // frames emitted
};

// one cycle's working copy of the caller's counters (include/cskel.h: csk_co_plan_cycle)
struct Counters {
    int64_t frames, feats;
    std::vector<BlockCounters> layer;
};

struct csk_co_plan {
    std::vector<csk_co_layer> layers;
    float *xin0;
    int xin0_slots;
    int N, C, V, M, classes, pool_size, pool_padding;
    int64_t P;
    const float *bn_scale, *bn_shift, *fc_w, *fc_b;
    float *pool_ring, *pooled;
    bool fuse = true;          // csk_co_block_step_f32 for the blocks that qualify
    int max_cycle = CSK_CO_MAX_CYCLE;   // frames one cycle may carry = what the rings were sized for (xin0_slots - 4, at most 8)
};

extern "C" csk_co_plan *csk_co_plan_create(int n_layers, const csk_co_layer *layers, float *xin0, int xin0_slots, int N, int C,
                                           int V, int M, int64_t P, const float *bn_scale, const float *bn_shift, int classes,
                                           const float *fc_w, const float *fc_b, int pool_size, int pool_padding,
                                           float *pool_ring, float *pooled) {
    if (n_layers <= 0 || !layers || !xin0 || N <= 0 || C <= 0 || V < 2 || M <= 0 || P < (int64_t)N * M * V || (P & 3) ||
        !bn_scale || !bn_shift || classes <= 0 || !fc_w || !fc_b || pool_size <= 0 || pool_padding < 0 ||
        pool_padding >= pool_size || !pool_ring || !pooled) {
        snprintf(csk_err_buf(), 256, "co_plan_create: bad argument");
        return nullptr;
    }
    if (xin0_slots < CSK_CO_IN_SLOTS(1)) {
        snprintf(csk_err_buf(), 256, "co_plan_create: the input ring needs >= %d slots, got %d", CSK_CO_IN_SLOTS(1), xin0_slots);
        return nullptr;
    }
    // the largest cycle the plan accepts is what the input ring was sized for: xin0_slots = CSK_CO_IN_SLOTS(max_cycle)
    const int max_cycle = xin0_slots - CSK_CO_IN_SLOTS(0) < CSK_CO_MAX_CYCLE ? xin0_slots - CSK_CO_IN_SLOTS(0) : CSK_CO_MAX_CYCLE;
    // ring depths against the frames one launch of each layer can receive / emit (include/cskel.h: CSK_CO_Y_SLOTS, CSK_CO_IN_SLOTS)
    for (int i = 0, max_in = max_cycle; i < n_layers; ++i) {
        const csk_co_layer &l = layers[i];
        if (l.stride < 1 || l.stride > 2) break;                              // reported by the per-layer checks below
        const int max_emit = max_in / l.stride > 0 ? max_in / l.stride : 1;
        const int want_out = i + 1 < n_layers ? CSK_CO_IN_SLOTS(max_emit) : max_emit;
        if (l.y_slots < CSK_CO_Y_SLOTS(max_in) || l.out_slots < want_out) {
            snprintf(csk_err_buf(), 256, "co_plan_create: layer %d rings too shallow: y_slots %d (need >= %d), out_slots %d (need >= %d)", i,
                     l.y_slots, CSK_CO_Y_SLOTS(max_in), l.out_slots, want_out);
            return nullptr;
        }
        if (l.gcn_ksplit > 1 && (l.gcn_partial_frames < 1 || !l.tcn_partial || l.agcn_inter > 0)) {
            snprintf(csk_err_buf(), 256, "co_plan_create: layer %d splits its graph conv but has no partial-sum buffer (or an adaptive graph conv)", i);
            return nullptr;
        }
        if (l.tcn_ksplit > 1 && l.partial_emits < 1) {
            snprintf(csk_err_buf(), 256, "co_plan_create: layer %d splits its K loop but partial_emits is %d", i, l.partial_emits);
            return nullptr;
        }
        if (l.agcn_inter > 0 && l.agcn_adj_frames < 1) {
            snprintf(csk_err_buf(), 256, "co_plan_create: layer %d has an adaptive graph conv but agcn_adj_frames is %d", i, l.agcn_adj_frames);
            return nullptr;
        }
        max_in = max_emit;
    }
    for (int i = 0; i < n_layers; ++i) {
        const csk_co_layer &l = layers[i];
        if (l.agcn_inter < 0 || (l.agcn_inter > 0 && (!l.agcn_w_pairs || !l.agcn_b_pairs || !l.agcn_a_sum || !l.agcn_adj ||
                                                      l.ell_w != V || l.ell_cnt[0] != V || l.ell_cnt[1] != V || l.ell_cnt[2] != V))) {
            snprintf(csk_err_buf(), 256, "co_plan_create: bad adaptive graph conv operands in layer %d", i);
            return nullptr;
        }
        if (l.c_in <= 0 || l.c_out <= 0 || l.stride < 1 || l.stride > 2 || !l.gcn_w || !l.gcn_bias || !l.ell_src ||
            (!l.ell_val && l.agcn_inter == 0) || !l.tcn_w || !l.tcn_bias || !l.y_ring || !l.out_ring ||
            (l.res_kind == CSK_RES_CONV && !l.tcn_w_res) || (i > 0 && l.c_in != layers[i - 1].c_out) ||
            (l.tcn_ksplit > 1 && !l.tcn_partial)) {
            snprintf(csk_err_buf(), 256, "co_plan_create: bad layer %d", i);
            return nullptr;
        }
    }
    csk_co_plan *p = new csk_co_plan();
    p->max_cycle = max_cycle;
    p->layers.assign(layers, layers + n_layers);
    p->xin0 = xin0; p->xin0_slots = xin0_slots; p->N = N; p->C = C; p->V = V; p->M = M; p->P = P;
    p->bn_scale = bn_scale; p->bn_shift = bn_shift; p->classes = classes; p->fc_w = fc_w; p->fc_b = fc_b;
    p->pool_size = pool_size; p->pool_padding = pool_padding;
    p->pool_ring = pool_ring; p->pooled = pooled;
    return p;
}

extern "C" void csk_co_plan_destroy(csk_co_plan *plan) { delete plan; }

extern "C" int csk_co_plan_update_weights(csk_co_plan *plan, int n_layers, const csk_co_layer *layers,
                                          const float *bn_scale, const float *bn_shift, const float *fc_w,
                                          const float *fc_b) {
    if (!plan || !layers || !bn_scale || !bn_shift || !fc_w || !fc_b) CSK_FAIL("co_plan_update_weights: null pointer");
    if (n_layers != (int)plan->layers.size()) CSK_FAIL("co_plan_update_weights: layer count mismatch");
    for (int i = 0; i < n_layers; ++i) {
        const csk_co_layer &o = plan->layers[i], &n = layers[i];
        if (o.c_in != n.c_in || o.c_out != n.c_out || o.stride != n.stride || o.res_kind != n.res_kind ||
            o.y_ring != n.y_ring || o.out_ring != n.out_ring || o.agcn_inter != n.agcn_inter || o.agcn_adj != n.agcn_adj ||
            o.y_slots != n.y_slots || o.out_slots != n.out_slots || o.partial_emits != n.partial_emits ||
            o.tcn_partial != n.tcn_partial || o.agcn_adj_frames != n.agcn_adj_frames || o.gcn_ksplit != n.gcn_ksplit ||
            o.gcn_partial_frames != n.gcn_partial_frames)
            CSK_FAIL("co_plan_update_weights: layer %d geometry/state differs", i);
    }
    plan->layers.assign(layers, layers + n_layers);
    plan->bn_scale = bn_scale; plan->bn_shift = bn_shift; plan->fc_w = fc_w; plan->fc_b = fc_b;
    return 0;
}

extern "C" int csk_co_plan_set_fusion(csk_co_plan *plan, int enable) {
    if (!plan) CSK_FAIL("co_plan_set_fusion: null pointer");
    plan->fuse = enable != 0;
    return 0;
}

// a whole emitting 4-frame cycle of a 64-row block that csk_co_block_step_f32 / csk_co_stack_step_f32 take (continual.py:_fusable)
static bool fusable_cycle(const csk_co_layer &l, const BlockCounters &c, int r, int V) {
    return l.agcn_inter == 0 && r == 4 && l.stride == 1 && l.c_out <= 64 && c.s >= 4 && l.res_kind != CSK_RES_CONV && l.tcn_ksplit <= 1 &&
           l.gcn_ksplit <= 1 && l.ell_cnt[0] <= 1 && l.ell_cnt[1] <= 1 && l.ell_cnt[2] <= 4 && ((64 + V - 2) / V + 1) * V <= 128;
}

// one block: r frames are already in xin[(s .. s+r-1) % HIST] (HIST = depth of the input ring = the upstream layer's
// out_slots); returns emissions via *slot0 / *n_emit
static int advance_block(const csk_co_layer &l, BlockCounters &c, const float *xin, int HIST, int r, int n_frames, int V,
                         int64_t P, int *slot0, int *n_emit, bool fuse, void *stream) {
    constexpr int K = 9, DELAY = 4, LAG = 4;      // padding="equal": delay = k-1-p = 4; residual lag (k-1)/2
    const int YRING = l.y_slots, OUT = l.out_slots;
    const long s0 = c.s;
    if (r + K - 1 > YRING || r + LAG > HIST)
        CSK_FAIL("co_plan_cycle: %d frames do not fit the rings of a layer (y ring %d slots, input ring %d)", r, YRING, HIST);
    // one fused launch for a whole emitting 4-frame cycle of a 64-row block (continual.py:_fusable)
    if (fuse && fusable_cycle(l, c, r, V)) {
        *slot0 = (int)(c.e % OUT);
        const int rc = csk_co_block_step_f32(xin, HIST, (int)(s0 % HIST), l.c_in, l.gcn_w, l.gcn_bias,
                                         l.ell_src, l.ell_val, l.ell_cnt, l.ell_w, l.gcn_res_mode, l.y_ring, YRING,
                                         (int)(s0 % YRING), l.tcn_w, l.tcn_bias, l.res_kind,
                                         (int)((s0 - LAG) % HIST), l.out_ring, OUT, *slot0, l.c_out, n_frames, V, P,
                                         stream);
        if (rc) return rc;
        c.s += 4; c.e += 4;
        *n_emit = 4;
        return 0;
    }
    for (int f = 0; f < r;) {                      // per-frame graph conv, one launch per non-wrapping slot run
        const long s = s0 + f;
        int run = r - f;
        if (run > HIST - (int)(s % HIST)) run = HIST - (int)(s % HIST);
        if (run > YRING - (int)(s % YRING)) run = YRING - (int)(s % YRING);
        const float *xs = xin + (s % HIST) * (int64_t)l.c_in * P;
        float *ys = l.y_ring + (s % YRING) * (int64_t)l.c_out * P;
        int rc;
        if (l.agcn_inter > 0) {
            if (run > l.agcn_adj_frames) CSK_FAIL("co_plan_cycle: %d frames of adjacencies do not fit agcn_adj (%d frames)", run, l.agcn_adj_frames);
            // adaptive graph conv (continual-skeletons_amd/agcn.py:AdaptiveGraphConvolution.stage): the adjacency of every
            // skeleton frame of the run, then the graph conv with it
            rc = csk_agcn_embed_attention_f32(xs, l.agcn_w_pairs, l.agcn_b_pairs, l.agcn_a_sum, l.agcn_adj, nullptr, run, l.c_in,
                                              l.agcn_inter, n_frames, V, 1, (int64_t)l.c_in * P, P, stream);
            if (rc) return rc;
            rc = csk_gcn_stage_f32(xs, ys, l.gcn_w, l.gcn_bias, l.ell_src, l.agcn_adj, l.ell_cnt, l.ell_w, (int64_t)3 * V * V, 1,
                                   run, l.c_in, l.c_out, n_frames, V, (int64_t)l.c_in * P, P, (int64_t)l.c_out * P, P,
                                   l.gcn_res_mode, stream);
        } else if (l.gcn_ksplit > 1) {
            if (run > l.gcn_partial_frames)
                CSK_FAIL("co_plan_cycle: %d frames exceed the split-K scratch of the layer's graph conv (%d frames)", run, l.gcn_partial_frames);
            rc = csk_gcn_stage_splitk_f32(xs, ys, l.gcn_w, l.gcn_bias, l.ell_src, l.ell_val, l.ell_cnt, l.ell_w, run, l.c_in, l.c_out,
                                          n_frames, V, (int64_t)l.c_in * P, P, (int64_t)l.c_out * P, P, l.gcn_res_mode, l.gcn_ksplit,
                                          l.tcn_partial, stream);
        } else {
            rc = csk_gcn_stage_f32(xs, ys, l.gcn_w, l.gcn_bias, l.ell_src, l.ell_val, l.ell_cnt, l.ell_w, 0, 0, run, l.c_in,
                                   l.c_out, n_frames, V, (int64_t)l.c_in * P, P, (int64_t)l.c_out * P, P, l.gcn_res_mode, stream);
        }
        if (rc) return rc;
        f += run;
    }
    long first = -1;
    for (long s = s0; s < s0 + r; ++s)
        if (s >= DELAY && (s - DELAY) % l.stride == 0) { first = s; break; }
    c.s += r;
    *n_emit = 0;
    if (first < 0) return 0;
    const int ne = (int)((s0 + r - 1 - first) / l.stride) + 1;
    if (ne > OUT) CSK_FAIL("co_plan_cycle: %d emissions do not fit an output ring of %d slots", ne, OUT);
    if (l.tcn_ksplit > 1 && ne > l.partial_emits)
        CSK_FAIL("co_plan_cycle: %d emissions exceed the split-K scratch of the layer (%d emissions)", ne, l.partial_emits);
    *slot0 = (int)(c.e % OUT);
    const int rc = csk_tcn_step_f32(l.y_ring, YRING, (int)(first % YRING), l.stride, ne, l.tcn_w,
                                    l.res_kind ? xin : nullptr, HIST, (int)((first - LAG) % HIST), l.stride,
                                    l.tcn_w_res, l.tcn_bias, l.out_ring, OUT, *slot0, l.c_out, l.c_out, P, K,
                                    l.res_kind, l.res_kind ? l.c_in : 0, 1, l.tcn_ksplit > 1 ? l.tcn_ksplit : 1, l.tcn_partial,
                                    stream);
    if (rc) return rc;
    c.e += ne;
    *n_emit = ne;
    return 0;
}

// the ten blocks for r new frames: *n_last emissions of the last block starting at output-ring slot *slot0
static int run_blocks(const csk_co_plan *p, std::vector<BlockCounters> &cnt, int r, int *slot0, int *n_last, void *stream) {
    const float *xin = p->xin0;
    int rr = r, in_slots = p->xin0_slots;
    *n_last = 0;
    for (size_t i = 0; i < p->layers.size(); ++i) {
        // consecutive blocks that each advance a whole emitting cycle: ONE launch for the run (csk_co_stack_step_f32)
        auto stackable = [&](size_t k, int r) {             // identity gcn_residual: what the fused stack kernel covers
            return fusable_cycle(p->layers[k], cnt[k], r, p->V) && p->layers[k].gcn_res_mode == CSK_RES_IDENTITY;
        };
        if (p->fuse && i + 1 < p->layers.size() && stackable(i, rr) && stackable(i + 1, 4)) {
            csk_co_block_args args[CSK_CO_STACK_MAX];
            int n = 0;
            size_t j = i;
            for (; j < p->layers.size() && n < CSK_CO_STACK_MAX && stackable(j, 4); ++j, ++n) {
                const csk_co_layer &l = p->layers[j];
                const long s0 = cnt[j].s;
                if (4 + 8 > l.y_slots || 4 + 4 > in_slots) CSK_FAIL("co_plan_cycle: 4 frames do not fit the rings of layer %d", (int)j);
                csk_co_block_args &a = args[n];
                a.xin = xin; a.xin_slots = in_slots; a.xin_slot0 = (int)(s0 % in_slots); a.c_in = l.c_in; a.gcn_w = l.gcn_w;
                a.gcn_bias = l.gcn_bias; a.ell_src = l.ell_src; a.ell_val = l.ell_val;
                a.ell_cnt[0] = l.ell_cnt[0]; a.ell_cnt[1] = l.ell_cnt[1]; a.ell_cnt[2] = l.ell_cnt[2];
                a.ell_w = l.ell_w; a.gcn_res_mode = l.gcn_res_mode; a.y_ring = l.y_ring; a.y_slots = l.y_slots; a.y_slot0 = (int)(s0 % l.y_slots);
                a.tcn_w = l.tcn_w; a.tcn_bias = l.tcn_bias; a.res_mode = l.res_kind; a.x_res_slot0 = (int)((s0 - 4) % in_slots);
                a.out = l.out_ring; a.out_slots = l.out_slots; a.out_slot0 = (int)(cnt[j].e % l.out_slots); a.c_out = l.c_out;
                xin = l.out_ring;
                in_slots = l.out_slots;
            }
            if (const int rc = csk_co_stack_step_f32(n, args, p->N * p->M, p->V, p->P, stream)) return rc;
            for (size_t k = i; k < j; ++k) { cnt[k].s += 4; cnt[k].e += 4; }
            *slot0 = args[n - 1].out_slot0;
            rr = 4;
            i = j - 1;
            continue;
        }
        int ne = 0;
        const int rc = advance_block(p->layers[i], cnt[i], xin, in_slots, rr, p->N * p->M, p->V, p->P, slot0, &ne, p->fuse, stream);
        if (rc) return rc;
        if (ne == 0) return 0;
        rr = ne;
        xin = p->layers[i].out_ring;
        in_slots = p->layers[i].out_slots;
    }
    *n_last = rr;
    return 0;
}

// the launches of one cycle on the working copy w.  A launch can fail half way through (bad pointer, launch error): w is
// then dropped.  (Ring slots already overwritten belong to frames older than every window or to the cycle that failed;
// re-running the cycle rewrites them.)
static int run_cycle(const csk_co_plan *p, Counters &w, const float *const *frames, int r, float *logits, int *last_slot,
                     int *n_feat, int *n_logits, void *stream) {
    {   // reshape1 + data_bn + reshape2 of the cycle's frames into the channel-major ring: one launch
        float *dst[CSK_CO_MAX_CYCLE];
        for (int f = 0; f < r; ++f) {
            if (!frames[f]) CSK_FAIL("co_plan_cycle: null frame");
            dst[f] = p->xin0 + ((w.frames + f) % p->xin0_slots) * (int64_t)p->C * p->P;
        }
        if (const int rc = csk_input_norm_frames_f32(frames, dst, r, p->bn_scale, p->bn_shift, p->N, p->C, p->V, p->M, p->P, stream)) return rc;
        w.frames += r;
    }
    int rr = 0, slot0 = 0;
    if (const int rc = run_blocks(p, w.layer, r, &slot0, &rr, stream)) return rc;
    if (rr == 0) return 0;
    *last_slot = slot0;
    *n_feat = rr;
    const csk_co_layer &last = p->layers.back();
    for (int j = 0; j < rr; ++j) {                 // spatial_pool -> co.AvgPool1d window -> co.Linear: one launch per emission
        const int slot = (slot0 + j) % last.out_slots;
        const int head = (int)(w.feats % p->pool_size);
        w.feats++;
        const int emit = w.feats >= p->pool_size - p->pool_padding;
        const int count = (int)(w.feats < p->pool_size ? w.feats : p->pool_size);
        const int rc = csk_co_head_step_f32(last.out_ring + slot * (int64_t)last.c_out * p->P, p->pool_ring, p->pooled, p->fc_w, p->fc_b,
                                            logits + (int64_t)(*n_logits) * p->N * p->classes, p->N, last.c_out, p->M * p->V, p->P,
                                            p->pool_size, head, count, emit, p->classes, stream);
        if (rc) return rc;
        if (emit) (*n_logits)++;
    }
    return 0;
}

extern "C" int csk_co_plan_cycle(csk_co_plan *p, int64_t *counters, int n_counters, const float *const *frames, int r,
                                 float *logits, int *last_slot, int *n_feat, int *n_logits, void *stream) {
    if (!p || !counters || !frames || !logits || !last_slot || !n_feat || !n_logits) CSK_FAIL("co_plan_cycle: null pointer");
    const int n_layers = (int)p->layers.size();
    if (n_counters != 2 + 2 * n_layers) CSK_FAIL("co_plan_cycle: expected %d counters, got %d", 2 + 2 * n_layers, n_counters);
    for (int i = 0; i < n_counters; ++i)
        if (counters[i] < 0) CSK_FAIL("co_plan_cycle: negative counter");
    if (r < 1 || r > p->max_cycle) CSK_FAIL("co_plan_cycle: r must be in [1, %d] (the rings of this plan were sized for cycles of %d frames)", p->max_cycle, p->max_cycle);
    *n_feat = *n_logits = 0;
    *last_slot = 0;
    Counters w{counters[0], counters[1], std::vector<BlockCounters>(n_layers)};
    for (int i = 0; i < n_layers; ++i) w.layer[i] = {counters[2 + 2 * i], counters[3 + 2 * i]};
    const int rc = run_cycle(p, w, frames, r, logits, last_slot, n_feat, n_logits, stream);
    if (rc) return rc;                             // the caller's counters are as they were passed in
    counters[0] = w.frames; counters[1] = w.feats;
    for (int i = 0; i < n_layers; ++i) { counters[2 + 2 * i] = w.layer[i].s; counters[3 + 2 * i] = w.layer[i].e; }
    return 0;
}
