#!/usr/bin/env python3
"""Interleaved in-process A/B of the Winograd temporal convs (csk_tcn_stage_wino_f32: identity-residual layers;
csk_tcn_stage_wino_ext_f32: the stride-2 layers and the layer without residual) against the direct kernels (diagnostic
CSK_TCN_WINO=1) on the layers of the clip stacks at batch 256 (512 sequences): both arms call blocks.tcn_stage WITH the Winograd
image, the switch alone decides.  Prints medians, the spread (min - max) of the direct arm's rounds and the largest |difference|
of the two outputs.
AB_TILES=1: the two workgroup shapes of the Winograd kernels against each other instead (CSK_TCN_WINO=2 wide, 64 channels x 128
pair columns; =3 tall, 128 x 64) on the layers with C_out % 128 == 0, and which of the two the host's rule takes.
usage: python tools/ab_wino_probe.py   (AB_NM=<sequences>, AB_ROUNDS=<rounds>, AB_ONLY=ext|identity, AB_TILES=1)"""
import os, sys
os.environ["CSK_DIAG"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, statistics
import _bootstrap
pkg = _bootstrap.load()
dev = "cuda:0"
NM = int(os.environ.get("AB_NM", "512")); ROUNDS = int(os.environ.get("AB_ROUNDS", "12"))
IDENTITY = [(c, c, 1, True, t, v) for v in (25, 18) for (c, t) in ((64, 300), (128, 150), (256, 75))]
EXT = [(ci, co, s, res, t, v) for v in (25, 18) for (ci, co, s, res, t) in ((3, 64, 1, False, 300), (64, 128, 2, True, 300),
                                                                              (128, 256, 2, True, 150))]
only = os.environ.get("AB_ONLY", "")
TILES = os.environ.get("AB_TILES", "") == "1"
ARMS = ("2", "3") if TILES else (None, "1")          # CSK_TCN_WINO of arm 0 / arm 1
if TILES:
    IDENTITY = [(c, c, 1, True, t, v) for v in (25, 18) for (c, t) in ((128, 150), (256, 75), (128, 300), (256, 150))]
    EXT = [(ci, co, s, res, t, v) for v in (25, 18) for (ci, co, s, res, t) in ((64, 128, 2, True, 300), (128, 256, 2, True, 150))]


def issued(t_out, v, co, mw):
    qp, nt, mt = (t_out + 1) // 2 * v, 128 // mw, 64 * mw
    return -(-qp // nt) * nt * -(-co // mt) * mt


for (ci, co, s, has_res, t, v) in (EXT if only == "ext" else IDENTITY if only == "identity" else IDENTITY + EXT):
    A = (pkg.ntu_graph() if v == 25 else pkg.kinetics_graph()).A
    blk = pkg.SpatioTemporalBlock(ci, co, A, stride=s, residual=has_res).eval().to(dev)
    x = torch.rand(NM, ci, t, v, device=dev); y = blk.gcn(x); ops = blk._packed_ops(x.device)
    mode = 0 if not has_res else 1 if (ci == co and s == 1) else 2
    kw = dict(relu=True, res_mode=mode, x_res=x if mode else None, w_res=ops["w_res"], w_wino=ops["w_wino"] if mode == 1 else None,
              w_wino_ext=ops["w_wino_ext"])
    assert (kw["w_wino"] is None) != (kw["w_wino_ext"] is None)
    res, outs = {0: [], 1: []}, {}
    for rnd in range(ROUNDS):
        for flag in (0, 1):
            if ARMS[flag]: os.environ["CSK_TCN_WINO"] = ARMS[flag]
            else: os.environ.pop("CSK_TCN_WINO", None)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = pkg.blocks.tcn_stage(y, ops["w"], ops["bias"], co, 9, s, 4, **kw)
            e1.record(); torch.cuda.synchronize()
            if rnd >= 2: res[flag].append(e0.elapsed_time(e1))
            outs[flag] = out
    os.environ.pop("CSK_TCN_WINO", None)
    diff = float((outs[0] - outs[1]).abs().max())
    m0, m1 = statistics.median(res[0]), statistics.median(res[1])
    if TILES:
        t_out = (t - 1) // s + 1
        rule = "tall" if s == 2 or 16 * issued(t_out, v, co, 2) <= 15 * issued(t_out, v, co, 1) else "wide"     # wino_pick_mw
        print(f"{ci}->{co} s{s} res={mode} T={t} V={v}: wide {m0:.3f} ms ({min(res[0]):.3f} - {max(res[0]):.3f}) | tall {m1:.3f} ms "
              f"({min(res[1]):.3f} - {max(res[1]):.3f}) | wide / tall {m0 / m1:.3f}x | rule takes {rule} | bitwise equal "
              f"{torch.equal(outs[0], outs[1])}", flush=True)
        del x, y, out, outs
        continue
    print(f"{ci}->{co} s{s} res={mode} T={t} V={v}: winograd {m0:.3f} ms (min {min(res[0]):.3f}) | direct {m1:.3f} ms "
          f"({min(res[1]):.3f} - {max(res[1]):.3f}) | speed-up {m1 / m0:.3f}x | max|diff| {diff:.2e} | max|out| {float(outs[1].abs().max()):.2f}",
          flush=True)
    del x, y, out, outs
