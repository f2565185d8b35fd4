// executor_trace_main.cpp -- launch trace of the native step executor (csrc/executor.hip) without a GPU: the executor's object
// linked against recording stubs of every entry it calls.  Prints one JSON object {scenario: [call, ...]} that
// tests/test_executor_trace_cpu.py compares with tests/golden/executor_trace.json.  No HIP call is made; device buffers are
// fake address ranges with distinct bases, and every pointer is written as "name+byte offset" ("null" for a null pointer).  A
// pointer that lies in no buffer ends the program with an error.
//
// Record forms (a JSON list each, name first):
//   the stage / step / head entries: their arguments in the order of include/cskel.h (ell_cnt as its three values);
//   "fused": n_blocks, n_skel, V, P, then every block's csk_co_block_args -- the form of csk_co_stack_step_f32 AND of
//            csk_co_block_step_f32 (one block): which of the two entries issued a one-block call is not part of the trace;
//   "cycle": r, return code, *last_slot, *n_feat, *n_logits, the counters after the call (one per csk_co_plan_cycle);
//   "error": the message of a refused call;
//   "fail":  k, return code, counters unchanged (1/0), launches before k equal the unfailing run's (1/0), their count.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "cskel.h"

namespace {

struct Buf {
    std::string name;
    uintptr_t base;
    uint64_t bytes;
};
std::vector<Buf> bufs;
std::vector<std::string> calls;      // the records of the running scenario
long fail_at = -1;                   // the stub of launch number fail_at (of the cycle) returns FAIL_RC instead of recording
long n_launch = 0;
constexpr int FAIL_RC = 700;
char err_text[256];

template <class T = float>
T *fake(const std::string &name, uint64_t bytes) {
    bufs.push_back({name, (uintptr_t)(bufs.size() + 1) << 36, bytes});
    return (T *)bufs.back().base;
}

std::string P_(const void *p) {
    if (!p) return "\"null\"";
    const uintptr_t a = (uintptr_t)p;
    for (const Buf &b : bufs)
        if (a >= b.base && a < b.base + b.bytes) return "\"" + b.name + "+" + std::to_string(a - b.base) + "\"";
    fprintf(stderr, "executor_trace: pointer %p lies in no buffer (call %zu)\n", p, calls.size());
    exit(2);
}
std::string I_(long long v) { return std::to_string(v); }

struct Rec {
    std::string s;
    explicit Rec(const char *name) : s(std::string("[\"") + name + "\"") {}
    Rec &p(const void *ptr) { s += "," + P_(ptr); return *this; }
    Rec &i(long long v) { s += "," + I_(v); return *this; }
    Rec &cnt(const int32_t *c) { return i(c[0]).i(c[1]).i(c[2]); }
    int done() {
        if (n_launch++ == fail_at) return FAIL_RC;
        calls.push_back(s + "]");
        return 0;
    }
};

int fused(int n, const csk_co_block_args *b, int n_skel, int V, int64_t P) {
    Rec r("fused");
    r.i(n).i(n_skel).i(V).i(P);
    for (int k = 0; k < n; ++k) {
        const csk_co_block_args &a = b[k];
        r.p(a.xin).i(a.xin_slots).i(a.xin_slot0).i(a.c_in).p(a.gcn_w).p(a.gcn_bias).p(a.ell_src).p(a.ell_val).cnt(a.ell_cnt)
            .i(a.ell_w).i(a.gcn_res_mode).p(a.y_ring).i(a.y_slots).i(a.y_slot0).p(a.tcn_w).p(a.tcn_bias).i(a.res_mode)
            .i(a.x_res_slot0).p(a.out).i(a.out_slots).i(a.out_slot0).i(a.c_out);
    }
    return r.done();
}

}  // namespace

// ---- recording stubs of what executor.hip calls --------------------------------------------------------------------------
char *csk_err_buf() { return err_text; }

extern "C" int csk_input_norm_frames_f32(const float *const *frames, float *const *dst, int r, const float *scale,
                                         const float *shift, int N, int C, int V, int M, int64_t P, void *stream) {
    Rec rec("csk_input_norm_frames_f32");
    for (int f = 0; f < r; ++f) rec.p(frames[f]);
    for (int f = 0; f < r; ++f) rec.p(dst[f]);
    return rec.i(r).p(scale).p(shift).i(N).i(C).i(V).i(M).i(P).p(stream).done();
}

extern "C" int csk_gcn_stage_f32(const float *x, float *y, const float *w, const float *bias, const int32_t *ell_src,
                                 const float *ell_val, const int32_t *ell_cnt, int ell_w, int64_t adj_seg_stride,
                                 int adj_per_frame, int n_seg, int c_in, int c_out, int frames, int V, int64_t x_seg_stride,
                                 int64_t x_chan_stride, int64_t y_seg_stride, int64_t y_chan_stride, int res_mode, void *stream) {
    return Rec("csk_gcn_stage_f32").p(x).p(y).p(w).p(bias).p(ell_src).p(ell_val).cnt(ell_cnt).i(ell_w).i(adj_seg_stride)
        .i(adj_per_frame).i(n_seg).i(c_in).i(c_out).i(frames).i(V).i(x_seg_stride).i(x_chan_stride).i(y_seg_stride)
        .i(y_chan_stride).i(res_mode).p(stream).done();
}

extern "C" int csk_gcn_stage_splitk_f32(const float *x, float *y, const float *w, const float *bias, const int32_t *ell_src,
                                        const float *ell_val, const int32_t *ell_cnt, int ell_w, int n_seg, int c_in, int c_out,
                                        int frames, int V, int64_t x_seg_stride, int64_t x_chan_stride, int64_t y_seg_stride,
                                        int64_t y_chan_stride, int res_mode, int ksplit, float *partial, void *stream) {
    return Rec("csk_gcn_stage_splitk_f32").p(x).p(y).p(w).p(bias).p(ell_src).p(ell_val).cnt(ell_cnt).i(ell_w).i(n_seg).i(c_in)
        .i(c_out).i(frames).i(V).i(x_seg_stride).i(x_chan_stride).i(y_seg_stride).i(y_chan_stride).i(res_mode).i(ksplit)
        .p(partial).p(stream).done();
}

extern "C" int csk_agcn_embed_attention_f32(const float *x, const float *w_pairs, const float *b_pairs, const float *a_sum,
                                            float *ell_val, float *scratch, int n_seg, int c_in, int inter, int frames, int V,
                                            int per_frame, int64_t x_seg_stride, int64_t x_chan_stride, void *stream) {
    return Rec("csk_agcn_embed_attention_f32").p(x).p(w_pairs).p(b_pairs).p(a_sum).p(ell_val).p(scratch).i(n_seg).i(c_in)
        .i(inter).i(frames).i(V).i(per_frame).i(x_seg_stride).i(x_chan_stride).p(stream).done();
}

extern "C" int csk_tcn_step_f32(const float *ring, int slots, int head, int head_step, int n_emit, const float *w,
                                const float *x_res, int x_res_slots, int x_res_slot0, int x_res_step, const float *w_res,
                                const float *bias, float *out, int out_slots, int out_slot0, int c, int c_out, int64_t P, int k,
                                int res_mode, int c_res, int relu, int ksplit, float *partial, void *stream) {
    return Rec("csk_tcn_step_f32").p(ring).i(slots).i(head).i(head_step).i(n_emit).p(w).p(x_res).i(x_res_slots).i(x_res_slot0)
        .i(x_res_step).p(w_res).p(bias).p(out).i(out_slots).i(out_slot0).i(c).i(c_out).i(P).i(k).i(res_mode).i(c_res).i(relu)
        .i(ksplit).p(partial).p(stream).done();
}

extern "C" int csk_co_block_step_f32(const float *xin, int xin_slots, int xin_slot0, int c_in, const float *gcn_w,
                                     const float *gcn_bias, const int32_t *ell_src, const float *ell_val, const int32_t *ell_cnt,
                                     int ell_w, int gcn_res_mode, float *y_ring, int y_slots, int y_slot0, const float *tcn_w,
                                     const float *tcn_bias, int res_mode, int x_res_slot0, float *out, int out_slots,
                                     int out_slot0, int c_out, int n_skel, int V, int64_t P, void *stream) {
    const csk_co_block_args a = {xin, xin_slots, xin_slot0, c_in, gcn_w, gcn_bias, ell_src, ell_val,
                                 {ell_cnt[0], ell_cnt[1], ell_cnt[2]}, ell_w, gcn_res_mode, y_ring, y_slots, y_slot0,
                                 tcn_w, tcn_bias, res_mode, x_res_slot0, out, out_slots, out_slot0, c_out};
    (void)stream;
    return fused(1, &a, n_skel, V, P);
}

extern "C" int csk_co_stack_step_f32(int n_blocks, const csk_co_block_args *blocks, int n_skel, int V, int64_t P, void *stream) {
    (void)stream;
    return fused(n_blocks, blocks, n_skel, V, P);
}

extern "C" int csk_co_head_step_f32(const float *h, float *pool_ring, float *pooled, const float *fc_w, const float *fc_b,
                                    float *logits, int N, int C, int MV, int64_t P, int window, int head, int count, int emit,
                                    int classes, void *stream) {
    return Rec("csk_co_head_step_f32").p(h).p(pool_ring).p(pooled).p(fc_w).p(fc_b).p(logits).i(N).i(C).i(MV).i(P).i(window)
        .i(head).i(count).i(emit).i(classes).p(stream).done();
}

// ---- scenarios -----------------------------------------------------------------------------------------------------------
namespace {

constexpr int N = 1, M = 2, V = 25, C = 3, CLASSES = 60, POOL = 6, POOL_PAD = 2;
constexpr int64_t P = 52;            // N * M * V = 50 positions rounded up to a multiple of 4

struct Shape { int c_in, c_out, stride, res_kind; };
constexpr int NONE = CSK_RES_NONE, IDENT = CSK_RES_IDENTITY, CONV = CSK_RES_CONV;
const std::vector<Shape> TEN = {{3, 64, 1, NONE}, {64, 64, 1, IDENT}, {64, 64, 1, IDENT}, {64, 64, 1, IDENT}, {64, 128, 2, CONV},
                                {128, 128, 1, IDENT}, {128, 128, 1, IDENT}, {128, 256, 2, CONV}, {256, 256, 1, IDENT}, {256, 256, 1, IDENT}};
const std::vector<Shape> LONE = {{64, 64, 1, IDENT}, {64, 128, 2, CONV}, {128, 128, 1, IDENT}};      // a lone fusable block in front of a strided one

struct Options {
    int max_cycle = 8;
    int split_k = 0;         // latency mode: the factors continual.py:_pick_ksplit / _pick_gcn_ksplit give for this split_k
    bool agcn = false;       // adaptive graph convs in every layer (inter = c_out / 4)
    bool fuse = true;
};

struct Model {
    std::vector<csk_co_layer> layers;
    csk_co_plan *plan = nullptr;
    std::vector<int64_t> counters;
    std::vector<const float *> frames;
    float *logits = nullptr;
    int c_first;
};

Model make(const std::vector<Shape> &table, const Options &o) {
    bufs.clear();
    Model m;
    const int n = (int)table.size();
    m.c_first = table[0].c_in;
    float *xin0 = fake("xin0", (uint64_t)CSK_CO_IN_SLOTS(o.max_cycle) * m.c_first * P * 4);
    float *partial = nullptr, *adj = nullptr;
    if (o.split_k > 1) partial = fake("partial", (uint64_t)o.max_cycle * 32 * 256 * P * 4);
    if (o.agcn) adj = fake("agcn_adj", (uint64_t)o.max_cycle * N * M * 3 * V * V * 4);
    int max_in = o.max_cycle;
    for (int i = 0; i < n; ++i) {
        const Shape &s = table[i];
        const std::string L = "L" + std::to_string(i) + ".";
        const int max_emit = max_in / s.stride > 0 ? max_in / s.stride : 1;
        csk_co_layer l = {};
        l.c_in = s.c_in; l.c_out = s.c_out; l.stride = s.stride;
        l.res_kind = s.res_kind;
        l.gcn_res_mode = s.c_in == s.c_out ? CSK_RES_IDENTITY : CSK_RES_CONV;
        l.ell_w = o.agcn ? V : 4;
        for (int k = 0; k < 3; ++k) l.ell_cnt[k] = o.agcn ? V : (k < 2 ? 1 : 4);
        l.y_slots = CSK_CO_Y_SLOTS(max_in);
        l.out_slots = i + 1 < n ? CSK_CO_IN_SLOTS(max_emit) : (max_emit > 4 ? max_emit : 4);
        l.gcn_w = fake(L + "gcn_w", 4096); l.gcn_bias = fake(L + "gcn_bias", 4096);
        l.ell_src = fake<int32_t>(L + "ell_src", 4096);
        l.ell_val = o.agcn ? nullptr : fake(L + "ell_val", 4096);
        l.tcn_w = fake(L + "tcn_w", 4096); l.tcn_bias = fake(L + "tcn_bias", 4096);
        l.tcn_w_res = l.res_kind == CSK_RES_CONV ? fake(L + "tcn_w_res", 4096) : nullptr;
        l.y_ring = fake(L + "y", (uint64_t)l.y_slots * s.c_out * P * 4);
        l.out_ring = fake(L + "out", (uint64_t)l.out_slots * s.c_out * P * 4);
        l.tcn_ksplit = l.gcn_ksplit = 1;
        if (o.split_k > 1) {
            const auto cap = [&](int c) { const int a = 4 * o.split_k, b = (c + 7) / 8; return a < 32 ? (a < b ? a : b) : (32 < b ? 32 : b); };
            l.tcn_ksplit = cap(s.c_out);
            l.partial_emits = max_emit;
            if (s.c_in >= 16) { l.gcn_ksplit = cap(s.c_in); l.gcn_partial_frames = max_in; }
            l.tcn_partial = partial;
        }
        if (o.agcn) {
            l.agcn_inter = s.c_out / 4; l.agcn_adj_frames = o.max_cycle; l.agcn_adj = adj;
            l.agcn_w_pairs = fake(L + "agcn_w_pairs", 4096); l.agcn_b_pairs = fake(L + "agcn_b_pairs", 4096);
            l.agcn_a_sum = fake(L + "agcn_a_sum", 4096);
        }
        m.layers.push_back(l);
        max_in = max_emit;
    }
    const int feat = table.back().c_out;
    for (int f = 0; f < CSK_CO_MAX_CYCLE; ++f) m.frames.push_back(fake("frame" + std::to_string(f), (uint64_t)N * m.c_first * V * M * 4));
    m.logits = fake("logits", (uint64_t)CSK_CO_MAX_CYCLE * N * CLASSES * 4);
    m.plan = csk_co_plan_create(n, m.layers.data(), xin0, CSK_CO_IN_SLOTS(o.max_cycle), N, m.c_first, V, M, P, fake("bn_scale", 4096),
                                fake("bn_shift", 4096), CLASSES, fake("fc_w", (uint64_t)CLASSES * feat * 4), fake("fc_b", 4096), POOL,
                                POOL_PAD, fake("pool_ring", (uint64_t)POOL * N * feat * 4), fake("pooled", (uint64_t)N * feat * 4));
    if (!m.plan) { fprintf(stderr, "executor_trace: csk_co_plan_create: %s\n", err_text); exit(2); }
    if (!o.fuse && csk_co_plan_set_fusion(m.plan, 0)) exit(2);
    m.counters.assign(2 + 2 * n, 0);
    return m;
}

int cycle(Model &m, int r) {
    int slot = -1, nf = -1, nl = -1;
    n_launch = 0;
    const int rc = csk_co_plan_cycle(m.plan, m.counters.data(), (int)m.counters.size(), m.frames.data(), r, m.logits, &slot, &nf, &nl, nullptr);
    Rec rec("cycle");
    rec.i(r).i(rc).i(slot).i(nf).i(nl);
    for (int64_t c : m.counters) rec.i(c);
    calls.push_back(rec.s + "]");
    if (rc < 0) calls.push_back(std::string("[\"error\",\"") + err_text + "\"]");
    return rc;
}

// the cycle mix: `head` first, then 4-frame cycles, then what is left of `total` frames
void run_mix(Model &m, std::vector<int> head, int total) {
    int done = 0;
    for (int r : head) { cycle(m, r); done += r; }
    while (done < total) { const int r = total - done < 4 ? total - done : 4; cycle(m, r); done += r; }
}

bool first = true;
void emit(const char *name) {
    printf("%s\"%s\":[\n", first ? "" : ",\n", name);
    for (size_t i = 0; i < calls.size(); ++i) printf("%s%s", i ? ",\n" : "", calls[i].c_str());
    printf("]");
    first = false;
    calls.clear();
}

}  // namespace

int main() {
    printf("{");
    Options o;
    {   Model m = make(TEN, o); run_mix(m, {1, 2, 4, 8, 3}, 96); emit("default"); csk_co_plan_destroy(m.plan); }
    {   Options f = o; f.fuse = false; Model m = make(TEN, f); run_mix(m, {1, 2, 4, 8, 3}, 96); emit("fusion_off"); csk_co_plan_destroy(m.plan); }
    {   Options l = o; l.split_k = 2; Model m = make(TEN, l); run_mix(m, {1, 2, 4, 8, 3}, 48); emit("latency"); csk_co_plan_destroy(m.plan); }
    {   Options a = o; a.agcn = true; Model m = make(TEN, a); run_mix(m, {1, 2, 4, 8, 3}, 48); emit("agcn"); csk_co_plan_destroy(m.plan); }
    {   // rings for 4-frame cycles: an 8-frame cycle is refused and leaves no trace
        Options r4 = o; r4.max_cycle = 4; Model m = make(TEN, r4);
        run_mix(m, {1, 2, 4, 3}, 30); cycle(m, 8); run_mix(m, {}, 18);
        emit("ring4"); csk_co_plan_destroy(m.plan);
    }
    {   Model m = make(LONE, o); run_mix(m, {}, 24); emit("lone_block"); csk_co_plan_destroy(m.plan); }
    {   // a stub that fails at launch k of one cycle of the default scenario (the 4-frame cycle after 90 frames: a lone fused
        // block, a fused run, two-stage blocks with wrapped slot runs, a head step), for every k of that cycle
        Model m = make(TEN, o);
        run_mix(m, {1, 2, 4, 8, 3}, 90);
        calls.clear();
        const std::vector<int64_t> before = m.counters;
        cycle(m, 4);
        const std::vector<std::string> whole(calls.begin(), calls.end() - 1);      // without the "cycle" record
        calls.clear();
        std::vector<std::string> out;
        for (long k = 0; k < (long)whole.size(); ++k) {
            m.counters = before;
            fail_at = k;
            const int rc = cycle(m, 4);
            fail_at = -1;
            const std::vector<std::string> got(calls.begin(), calls.end() - 1);
            const bool prefix = got.size() == (size_t)k && std::vector<std::string>(whole.begin(), whole.begin() + k) == got;
            out.push_back("[\"fail\"," + I_(k) + "," + I_(rc) + "," + I_(m.counters == before) + "," + I_(prefix) + "," + I_((long)got.size()) + "]");
            calls.clear();
        }
        calls = out;
        emit("fail_at_k"); csk_co_plan_destroy(m.plan);
    }
    printf("}\n");
    return 0;
}
