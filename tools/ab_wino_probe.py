#!/usr/bin/env python3
"""Interleaved in-process A/B of the Winograd temporal conv (csk_tcn_stage_wino_f32) against the direct kernels (diagnostic
CSK_TCN_WINO=1) on the identity-residual layers of the clip stacks at batch 256 (512 sequences): both arms call
blocks.tcn_stage WITH the Winograd image, the switch alone decides.  Also prints the largest |difference| of the two outputs.
usage: python tools/ab_wino_probe.py   (AB_NM=<sequences>, AB_ROUNDS=<rounds>)"""
import os, sys
os.environ["CSK_DIAG"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, statistics
import _bootstrap
pkg = _bootstrap.load()
dev = "cuda:0"
NM = int(os.environ.get("AB_NM", "512")); ROUNDS = int(os.environ.get("AB_ROUNDS", "12"))
for (c, t, v) in [(64, 300, 25), (128, 150, 25), (256, 75, 25), (64, 300, 18), (128, 150, 18), (256, 75, 18)]:
    A = (pkg.ntu_graph() if v == 25 else pkg.kinetics_graph()).A
    blk = pkg.SpatioTemporalBlock(c, c, A, stride=1).eval().to(dev)
    x = torch.rand(NM, c, t, v, device=dev); y = blk.gcn(x); ops = blk._packed_ops(x.device)
    res, outs = {0: [], 1: []}, {}
    for rnd in range(ROUNDS):
        for flag in (0, 1):
            if flag: os.environ["CSK_TCN_WINO"] = "1"
            else: os.environ.pop("CSK_TCN_WINO", None)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = pkg.blocks.tcn_stage(y, ops["w"], ops["bias"], c, 9, 1, 4, relu=True, res_mode=1, x_res=x, w_wino=ops["w_wino"])
            e1.record(); torch.cuda.synchronize()
            if rnd >= 2: res[flag].append(e0.elapsed_time(e1))
            outs[flag] = out
    os.environ.pop("CSK_TCN_WINO", None)
    diff = float((outs[0] - outs[1]).abs().max())
    m0, m1 = statistics.median(res[0]), statistics.median(res[1])
    print(f"{c}->{c} T={t} V={v}: winograd {m0:.3f} ms (min {min(res[0]):.3f}) | direct {m1:.3f} ms (min {min(res[1]):.3f}) | "
          f"speed-up {m1 / m0:.3f}x | max|diff| {diff:.2e}", flush=True)
    del x, y, out, outs
