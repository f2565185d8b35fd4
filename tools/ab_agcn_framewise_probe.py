#!/usr/bin/env python3
"""What a stored clip costs at the steps' arithmetic on a CoAGcn, three ways, one process, rounds alternating:
  (a) steps:     clean_state(); forward_steps(x)                         -- T cycles of the continual path;
  (b) composed:  forward_clip_as_steps(x) with AdaptiveGraphConvolution.fuse_framewise = False: the per-frame launches
                 (csk_agcn_embed_attention_f32 + csk_gcn_stage_f32, adjacencies through HBM, chunked under framewise_budget_bytes);
  (c) kernel:    forward_clip_as_steps(x) with the frame-wise stage kernel (csk_agcn_stage_framewise_f32) wherever it is built
                 (framewise_everywhere = True);
  (d) shipped:   the default: the kernel where it measured faster, the composed launches elsewhere.
Per forward (HIP events, no sync inside, median of the rounds) and per layer for (b) and (c) (the graph-conv stage of every block on
the block's own input), with the new launch's fraction of the fp32 MFMA peak (157.3 TFLOP/s: 256 CUs x 256 FLOP/clk x 2.4 GHz)
counting the embedding GEMM, the logits and the channel mix.
usage: python tools/ab_agcn_framewise_probe.py [kinetics|ntu] [batch] [T] [rounds]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import _bootstrap  # noqa: E402
import bench  # noqa: E402

pkg = _bootstrap.load()
dev = "cuda:0"
shape = sys.argv[1] if len(sys.argv) > 1 else "kinetics"
batch = int(sys.argv[2]) if len(sys.argv) > 2 else (64 if shape == "kinetics" else 32)
T = int(sys.argv[3]) if len(sys.argv) > 3 else 300
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
PEAK = 157.3e12
A = pkg.kinetics_graph().A if shape == "kinetics" else pkg.ntu_graph().A
V = A.shape[-1]
AGC = pkg.AdaptiveGraphConvolution

net = pkg.CoAGcn(A, input_shape=(3, 300, V, 2), num_classes=400 if V == 18 else 60).eval()
bench.randomise_(net, 0)
net = net.to(dev)
x = torch.rand((batch, 3, T, V, 2), device=dev, generator=torch.Generator(device=dev).manual_seed(1))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def steps():
    net.clean_state()
    return net.forward_steps(x)


def clip(fused, everywhere=True):
    AGC.fuse_framewise, AGC.framewise_everywhere = fused, everywhere
    try:
        return net.forward_clip_as_steps(x)
    finally:
        AGC.fuse_framewise, AGC.framewise_everywhere = True, False


arms = {"a_steps": steps, "b_composed": lambda: clip(False), "c_kernel": lambda: clip(True), "d_shipped": lambda: clip(True, False)}
outs = {k: fn() for k, fn in arms.items()}          # warm-up: code objects, the allocator has seen the sizes
torch.cuda.synchronize()
scale = float(outs["a_steps"].abs().max())
for k in ("b_composed", "c_kernel", "d_shipped"):
    print(f"AGCN_FRAMEWISE_AB {shape} batch {batch} T {T}: {k} against the steps: {tuple(outs[k].shape)}, largest difference "
          f"{float((outs[k] - outs['a_steps']).abs().max()) / scale:.2e} of the largest value", flush=True)
ms = {k: [] for k in arms}
for _ in range(rounds):
    for k, fn in arms.items():                      # alternating: a drift of the clocks hits every arm alike
        ms[k].append(timed(fn)[0])
med = {k: statistics.median(v) for k, v in ms.items()}
for k in arms:
    print(f"AGCN_FRAMEWISE_AB {shape} batch {batch} T {T}: {k} {med[k]:.2f} ms ({min(ms[k]):.2f} - {max(ms[k]):.2f}), "
          f"{batch / med[k]:.2f} k clips/s", flush=True)
print(f"AGCN_FRAMEWISE_AB {shape}: forward (c) against (b) {med['b_composed'] / med['c_kernel']:.3f}x, against (a) "
      f"{med['a_steps'] / med['c_kernel']:.2f}x; (b) against (a) {med['a_steps'] / med['b_composed']:.2f}x; shipped (d) against (b) "
      f"{med['b_composed'] / med['d_shipped']:.3f}x, against (a) {med['a_steps'] / med['d_shipped']:.2f}x", flush=True)

# per layer: the graph-conv stage alone on the layer's own input
h = torch.rand((batch * 2, 3, T, V), device=dev)
for i, blk in enumerate(net._blocks):
    g = blk.gcn
    per = {"b": [], "c": []}
    AGC.framewise_everywhere = True
    for _ in range(rounds + 1):
        for arm, fused in (("b", False), ("c", True)):
            AGC.fuse_framewise = fused
            per[arm].append(timed(lambda: g.forward_framewise(h))[0])
    route = g.framewise_route(h)
    AGC.fuse_framewise, AGC.framewise_everywhere = True, False
    b, c = statistics.median(per["b"][2:]), statistics.median(per["c"][2:])
    n, ci, t, v = h.shape
    co, inter = g.out_channels, g.inter_c
    r = 4 if g._packed_ops(h.device)["res_mode"] == 2 else 3
    flop = 2.0 * n * t * v * (6 * inter * ci + 3 * inter * v + r * co * ci)
    print(f"AGCN_FRAMEWISE_AB {shape} layer {i + 1} ({ci} -> {co}, T {t}, route {route}, shipped: {'kernel' if g.framewise_route(h) else 'composed'}): composed {b:.3f} ms, kernel {c:.3f} ms, "
          f"{b / c:.3f}x; kernel at {flop / (c * 1e-3) / PEAK:.3f} of the fp32 MFMA peak", flush=True)
    h = net._framewise_parts(blk, h)[1]
