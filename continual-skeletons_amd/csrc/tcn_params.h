// tcn_params.h -- launch parameters of the clip temporal-conv stage (tcn.hip: 32x32x2 tiles; tcn16.hip: 16x16x4 tiles;
// tcn_wino.hip: the Winograd forms), and the argument checks its entries share
#pragma once
#include <stdint.h>

#include "mfma_core.h"

struct TcnParams {
    const float *y, *w, *xres, *wres, *bias;
    float *out;
    int C, Cpad, Cout, Mpad, Tin, Tout, V, K, stride, pad;
    int res_mode, Cres, CresPad, Tres, res_off, relu, ldb;
    unsigned vmagic, mtiles, qtiles;
    int nt;                       // positions per tile actually used (<= 16384 / MT)
    int fast_epi;                 // row strides fit the 32-bit lane offsets of the scalar-base epilogue addressing
    int ldb2;                     // conv-residual phase: LDS row stride of its activation tile
    int ksplit, cper;             // split-K form (csk_tcn_stage_splitk_f32): ksplit channel ranges of cper channels per tile,
    float *part;                  // raw partial sums part[(seg * ksplit + ks)][Cout][Tout * V]; ksplit == 1: off
};

// The fields every launcher (tcn.hip, tcn_wino.hip, the few-channel block of tcn16.hip) derives from the operands, in the argument
// order of csk_tcn_stage_f32 with the output frames beside the input frames: a plain, unsplit call.  xres / wres / c_res / t_res /
// res_off are taken as given: a launch without a residual still forms addresses from them, and each launcher keeps the stand-ins
// it has always passed.  The launcher adds its own: tile geometry (mtiles, qtiles, nt, ldb, ldb2), fast_epi, a split.
inline TcnParams tcn_params(const float *y, const float *w, const float *xres, const float *wres, const float *bias, float *out, int c,
                            int c_out, int t_in, int t_out, int V, int k, int stride, int pad, int res_mode, int c_res, int t_res,
                            int res_off, int relu) {
    TcnParams p = {};
    p.y = y; p.w = w; p.xres = xres; p.wres = wres; p.bias = bias; p.out = out;
    p.C = c; p.Cpad = round_up(c, CSK_CPAD); p.Cout = c_out; p.Mpad = round_up(c_out, CSK_MT);
    p.Tin = t_in; p.Tout = t_out; p.V = V; p.K = k; p.stride = stride; p.pad = pad;
    p.res_mode = res_mode; p.Cres = c_res; p.CresPad = round_up(c_res, CSK_CPAD); p.Tres = t_res; p.res_off = res_off; p.relu = relu;
    p.vmagic = vmagic_of(V);
    p.ksplit = 1; p.cper = p.Cpad; p.part = nullptr;
    return p;
}

// The argument checks csk_tcn_stage_f32 / csk_tcn_stage_splitk_f32 (tcn.hip) and csk_tcn_stage_bf16x3 (tcn_split.hip) share,
// reported as "<who>: ..." in the one order all three report them: null pointers, dims, the caller's own limits on k / stride /
// pad (kernel_limits(): 0, or -1 with the message set -- they come before anything divides by the stride), t_in, the residual
// block, the T*V bound.  0 with *t_out set, or -1 with the message set.
template <class KernelLimits>
inline int tcn_stage_check(const char *who, const void *y, const void *w, const void *x_res, const void *w_res, const void *bias,
                           const void *out, int n_seg, int c, int c_out, int t_in, int V, int k, int stride, int pad, int res_mode,
                           int c_res, int t_res, int res_off, KernelLimits kernel_limits, int *t_out) {
    if (!y || !w || !bias || !out) CSK_FAIL("%s: null pointer", who);
    if (n_seg <= 0 || c <= 0 || c_out <= 0 || t_in <= 0 || V < 2 || V > 64) CSK_FAIL("%s: bad dims", who);
    if (const int rc = kernel_limits()) return rc;
    if (t_in + 2 * pad < k) CSK_FAIL("%s: t_in too short for kernel", who);
    *t_out = (t_in + 2 * pad - k) / stride + 1;
    if (res_mode != CSK_RES_NONE) {
        if (!x_res) CSK_FAIL("%s: residual requested without x_res", who);
        if (res_mode == CSK_RES_IDENTITY && c_res != c_out) CSK_FAIL("%s: identity residual needs c_res == c_out", who);
        if (res_mode == CSK_RES_CONV && !w_res) CSK_FAIL("%s: conv residual without w_res", who);
        if ((*t_out - 1) * stride + res_off >= t_res || res_off < 0) CSK_FAIL("%s: residual frames out of range", who);
    }
    if ((int64_t)t_in * V >= (1 << 26)) CSK_FAIL("%s: T*V too large for 32-bit position arithmetic", who);
    return 0;
}

// tcn16.hip: the 16x16x4 tile family for the 9-tap temporal conv at V = 25 / 18 and stride 1 / 2.  csk_tcn_stage16_takes: the
// shape is one it is built for and measures faster on (host arithmetic on the shape fields of p only; tcn_stage_route asks it);
// csk_launch_tcn_stage16 launches such a shape (-2, nothing launched, for any other).  Stride 1: bitwise the sums of tcn_stage_kernel (same (8-channel chunk, tap,
// channel) order).  Stride 2 walks 4-channel chunks: another fp32 summation order, taken by the shape alone.
bool csk_tcn_stage16_takes(const TcnParams &p);
int csk_launch_tcn_stage16(TcnParams p, int n_seg, void *stream);
