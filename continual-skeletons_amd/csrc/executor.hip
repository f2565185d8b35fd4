// executor.hip -- native step executor for the continual stack (host code only; launches go through the C ABI
// entry points of gcn.hip / step.hip / step16.hip / head.hip).  Mirrors continual.py:CoSpatioTemporalBlock.engine_advance
// (advance_block: the two stages; run_blocks: the fused cycles, one csk_co_stack_step_f32 call per run of blocks) and
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
    std::vector<int> delay;    // per layer: steps before the first emission, k - 1 - padding (4: padding "equal"; 8: padding 0)
    float *xin0;
    int xin0_slots;
    int N, C, V, M, classes, pool_size, pool_padding;
    int64_t P;
    const float *bn_scale, *bn_shift, *fc_w, *fc_b;
    float *pool_ring, *pooled;
    bool fuse = true;          // one fused call for the blocks that qualify (run_blocks)
    int max_cycle = CSK_CO_MAX_CYCLE;   // frames one cycle may carry = what the rings were sized for (xin0_slots - 4, at most 8)
};

// csk_co_plan_create returns a pointer: a refusal leaves its message and no plan

#define CREATE_FAIL(...) do { snprintf(csk_err_buf(), 256, __VA_ARGS__); return nullptr; } while (0)
extern "C" csk_co_plan *csk_co_plan_create(int n_layers, const csk_co_layer *layers, float *xin0, int xin0_slots, int N, int C,
                                           int V, int M, int64_t P, const float *bn_scale, const float *bn_shift, int classes,
                                           const float *fc_w, const float *fc_b, int pool_size, int pool_padding,
                                           float *pool_ring, float *pooled) {
    if (n_layers <= 0 || !layers || !xin0 || N <= 0 || C <= 0 || V < 2 || M <= 0 || P < (int64_t)N * M * V || (P & 3) ||
        !bn_scale || !bn_shift || classes <= 0 || !fc_w || !fc_b || pool_size <= 0 || pool_padding < 0 ||
        pool_padding >= pool_size || !pool_ring || !pooled)
        CREATE_FAIL("co_plan_create: bad argument");
    if (xin0_slots < CSK_CO_IN_SLOTS(1))
        CREATE_FAIL("co_plan_create: the input ring needs >= %d slots, got %d", CSK_CO_IN_SLOTS(1), xin0_slots);
    // the largest cycle the plan accepts is what the input ring was sized for: xin0_slots = CSK_CO_IN_SLOTS(max_cycle)
    const int max_cycle = xin0_slots - CSK_CO_IN_SLOTS(0) < CSK_CO_MAX_CYCLE ? xin0_slots - CSK_CO_IN_SLOTS(0) : CSK_CO_MAX_CYCLE;
    // ring depths against the frames one launch of each layer can receive / emit (include/cskel.h: CSK_CO_Y_SLOTS, CSK_CO_IN_SLOTS)
    for (int i = 0, max_in = max_cycle; i < n_layers; ++i) {
        const csk_co_layer &l = layers[i];
        if (l.stride < 1 || l.stride > 2) break;                              // reported by the per-layer checks below
        const int max_emit = max_in / l.stride > 0 ? max_in / l.stride : 1;
        const int want_out = i + 1 < n_layers ? CSK_CO_IN_SLOTS(max_emit) : max_emit;
        if (l.y_slots < CSK_CO_Y_SLOTS(max_in) || l.out_slots < want_out)
            CREATE_FAIL("co_plan_create: layer %d rings too shallow: y_slots %d (need >= %d), out_slots %d (need >= %d)", i,
                        l.y_slots, CSK_CO_Y_SLOTS(max_in), l.out_slots, want_out);
        if (l.gcn_ksplit > 1 && (l.gcn_partial_frames < 1 || !l.tcn_partial || l.agcn_inter > 0))
            CREATE_FAIL("co_plan_create: layer %d splits its graph conv but has no partial-sum buffer (or an adaptive graph conv)", i);
        if (l.tcn_ksplit > 1 && l.partial_emits < 1)
            CREATE_FAIL("co_plan_create: layer %d splits its K loop but partial_emits is %d", i, l.partial_emits);
        if (l.agcn_inter > 0 && l.agcn_adj_frames < 1)
            CREATE_FAIL("co_plan_create: layer %d has an adaptive graph conv but agcn_adj_frames is %d", i, l.agcn_adj_frames);
        max_in = max_emit;
    }
    for (int i = 0; i < n_layers; ++i) {
        const csk_co_layer &l = layers[i];
        if (l.agcn_inter < 0 || (l.agcn_inter > 0 && (!l.agcn_w_pairs || !l.agcn_b_pairs || !l.agcn_a_sum || !l.agcn_adj ||
                                                      l.ell_w != V || l.ell_cnt[0] != V || l.ell_cnt[1] != V || l.ell_cnt[2] != V)))
            CREATE_FAIL("co_plan_create: bad adaptive graph conv operands in layer %d", i);
        if (l.c_in <= 0 || l.c_out <= 0 || l.stride < 1 || l.stride > 2 || !l.gcn_w || !l.gcn_bias || !l.ell_src ||
            (!l.ell_val && l.agcn_inter == 0) || !l.tcn_w || !l.tcn_bias || !l.y_ring || !l.out_ring ||
            (l.res_kind == CSK_RES_CONV && !l.tcn_w_res) || (i > 0 && l.c_in != layers[i - 1].c_out) ||
            (l.tcn_ksplit > 1 && !l.tcn_partial))
            CREATE_FAIL("co_plan_create: bad layer %d", i);
    }
    csk_co_plan *p = new csk_co_plan();
    p->max_cycle = max_cycle;
    p->layers.assign(layers, layers + n_layers);
    p->delay.assign(n_layers, 4);
    p->xin0 = xin0; p->xin0_slots = xin0_slots; p->N = N; p->C = C; p->V = V; p->M = M; p->P = P;
    p->bn_scale = bn_scale; p->bn_shift = bn_shift; p->classes = classes; p->fc_w = fc_w; p->fc_b = fc_b;
    p->pool_size = pool_size; p->pool_padding = pool_padding;
    p->pool_ring = pool_ring; p->pooled = pooled;
    return p;
}

#undef CREATE_FAIL

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

extern "C" int csk_co_plan_set_delays(csk_co_plan *plan, int n_layers, const int32_t *delays) {
    if (!plan || !delays) CSK_FAIL("co_plan_set_delays: null pointer");
    if (n_layers != (int)plan->layers.size()) CSK_FAIL("co_plan_set_delays: layer count mismatch");
    for (int i = 0; i < n_layers; ++i)
        if (delays[i] < 4 || delays[i] > 8) CSK_FAIL("co_plan_set_delays: layer %d delay %d outside [4, 8] (k - 1 - padding, k = 9)", i, delays[i]);
    plan->delay.assign(delays, delays + n_layers);
    return 0;
}

// a whole emitting 4-frame cycle of a 64-row block that csk_co_block_step_f32 / csk_co_stack_step_f32 take (continual.py:_fusable);
// the fused kernels emit for all four frames and read y[s - 8 .. s], x[s - 4]: right for any delay once s >= delay
static bool fusable_cycle(const csk_co_layer &l, const BlockCounters &c, int delay, int r, int V) {
    return l.agcn_inter == 0 && r == 4 && l.stride == 1 && l.c_out <= 64 && c.s >= delay && l.res_kind != CSK_RES_CONV && l.tcn_ksplit <= 1 &&
           l.gcn_ksplit <= 1 && l.ell_cnt[0] <= 1 && l.ell_cnt[1] <= 1 && l.ell_cnt[2] <= 4 && ((64 + V - 2) / V + 1) * V <= 128;
}

// the arguments of a fused 4-frame cycle of layer l at position c, its new frames in xin[(c.s .. c.s + 3) % in_slots]
static csk_co_block_args co_block_args(const csk_co_layer &l, const BlockCounters &c, const float *xin, int in_slots) {
    return {xin, in_slots, (int)(c.s % in_slots), l.c_in, l.gcn_w, l.gcn_bias, l.ell_src, l.ell_val,
            {l.ell_cnt[0], l.ell_cnt[1], l.ell_cnt[2]}, l.ell_w, l.gcn_res_mode, l.y_ring, l.y_slots, (int)(c.s % l.y_slots),
            l.tcn_w, l.tcn_bias, l.res_kind, (int)((c.s - 4) % in_slots), l.out_ring, l.out_slots, (int)(c.e % l.out_slots), l.c_out};
}

// Of the steps s0 .. s0 + r - 1, those that emit are the s >= delay with (s - delay) % stride == 0: the first of them and how
// many (*n = 0: none).  continual.py:emissions
static int64_t emissions(int64_t s0, int r, int delay, int stride, int *n) {
    int64_t first = s0 > delay ? s0 : delay;
    first += (stride - (first - delay) % stride) % stride;
    *n = first < s0 + r ? (int)((s0 + r - 1 - first) / stride) + 1 : 0;
    return first;
}

// one block in two stages: r frames are already in xin[(s .. s+r-1) % HIST] (HIST = depth of the input ring = the upstream
// layer's out_slots); returns emissions via *slot0 / *n_emit
static int advance_block(const csk_co_layer &l, BlockCounters &c, int delay, const float *xin, int HIST, int r, int n_frames, int V,
                         int64_t P, int *slot0, int *n_emit, void *stream) {
    constexpr int K = 9, LAG = 4;                 // delay = k-1-p (4: padding="equal", 8: padding 0); residual lag (k-1)/2 in both
    const int YRING = l.y_slots, OUT = l.out_slots;      // (run_blocks has checked that r frames fit YRING and HIST)
    const int64_t s0 = c.s;
    for (int f = 0; f < r;) {                      // per-frame graph conv, one launch per non-wrapping slot run
        const int64_t s = s0 + f;
        const int run = ring_run(r - f, (int)(s % HIST), HIST, (int)(s % YRING), YRING);
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
    int ne;
    const int64_t first = emissions(s0, r, delay, l.stride, &ne);
    c.s += r;
    *n_emit = 0;
    if (ne == 0) return 0;
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
    auto fusable = [&](size_t k, int r) { return p->fuse && k < p->layers.size() && fusable_cycle(p->layers[k], cnt[k], p->delay[k], r, p->V); };
    // identity gcn_residual: what the fused stack kernel covers
    auto stackable = [&](size_t k, int r) { return fusable(k, r) && p->layers[k].gcn_res_mode == CSK_RES_IDENTITY; };
    for (size_t i = 0; i < p->layers.size(); ++i) {
        const csk_co_layer &l = p->layers[i];
        // n consecutive blocks from i on that each advance a whole emitting 4-frame cycle go in ONE call.  A run grows past its
        // first block only over stackable blocks: layer 1 (conv gcn_residual) and a block without such a neighbour are runs of one.
        size_t n = fusable(i, rr) ? 1 : 0;
        if (n && stackable(i, rr))
            while (n < CSK_CO_STACK_MAX && stackable(i + n, 4)) ++n;
        // (two refusal texts for rings that are too shallow: a run of several blocks names the layer, below)
        if (n < 2 && (rr + 8 > l.y_slots || rr + 4 > in_slots))
            CSK_FAIL("co_plan_cycle: %d frames do not fit the rings of a layer (y ring %d slots, input ring %d)", rr, l.y_slots, in_slots);
        if (n) {
            csk_co_block_args args[CSK_CO_STACK_MAX];
            for (size_t k = 0; k < n; ++k) {
                const csk_co_layer &b = p->layers[i + k];
                if (4 + 8 > b.y_slots || 4 + 4 > in_slots) CSK_FAIL("co_plan_cycle: 4 frames do not fit the rings of layer %d", (int)(i + k));
                args[k] = co_block_args(b, cnt[i + k], xin, in_slots);
                xin = b.out_ring;
                in_slots = b.out_slots;
            }
            if (const int rc = csk_co_stack_step_f32((int)n, args, p->N * p->M, p->V, p->P, stream)) return rc;
            for (size_t k = 0; k < n; ++k) { cnt[i + k].s += 4; cnt[i + k].e += 4; }
            *slot0 = args[n - 1].out_slot0;
            rr = 4;
            i += n - 1;
            continue;
        }
        int ne = 0;
        const int rc = advance_block(l, cnt[i], p->delay[i], xin, in_slots, rr, p->N * p->M, p->V, p->P, slot0, &ne, stream);
        if (rc) return rc;
        if (ne == 0) return 0;
        rr = ne;
        xin = l.out_ring;
        in_slots = l.out_slots;
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
