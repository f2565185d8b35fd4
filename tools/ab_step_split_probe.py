#!/usr/bin/env python3
"""In-process A/B of the continual temporal step per layer shape (1024 NTU streams, 4 frames per launch): the exact launch
(csk_tcn_step_f32) against the opt-in bf16x3 step (csk_tcn_step_bf16x3, csrc/step_split.hip; it needs no conversion launch:
the ring is split at staging), HIP events, interleaved rounds in three repeats -> median ms per repeat, the spread of the
repeats, max |difference|.  Then the whole cycle: CoStGcn online frames/s on the Python engine, f32 against the mode, with the
native-plan f32 figure alongside, the max |logit difference| and the state-slab bytes.
usage: python tools/ab_step_split_probe.py [streams] [rounds] [cycles]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import _bootstrap  # noqa: E402
import bench  # noqa: E402

pkg = _bootstrap.load()
native = pkg.native
dev = "cuda:0"
streams = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
cycles = int(sys.argv[3]) if len(sys.argv) > 3 else 30
A = pkg.ntu_graph().A
P = (streams * 2 * 25 + 3) // 4 * 4
# layers 5-10 of the ten-block table: (c_in, c_out, stride, frames received per 4-frame cycle)
shapes = [(64, 128, 2, 4), (128, 128, 1, 2), (128, 256, 2, 2), (256, 256, 1, 1)]
for ci, co, s, recv in shapes:
    blk = pkg.CoSpatioTemporalBlock(ci, co, A, stride=s, padding="equal").eval()
    bench.randomise_(blk, 0)
    pkg.set_step_precision(blk, "bf16x3")
    blk = blk.to(dev)
    ops = blk._packed_ops(dev)
    n_emit = recv // s
    mode = 1 if blk.kind == "identity" else 2
    YR, HIST, OUT = 8 + recv, 4 + recv, max(4, n_emit)
    y = torch.rand((YR, co, P), device=dev)
    xin = torch.rand((HIST, ci, P), device=dev)
    out = torch.empty((OUT, co, P), device=dev)
    head = YR - 2                                    # the window of the last emission wraps the ring
    common = (native.ptr(y), YR, head, s, n_emit)
    res = (native.ptr(xin), HIST, 1, s)
    tail = (native.ptr(ops["bias"]), native.ptr(out), OUT, 0, co, co, P, 9, mode, ci, 1)

    def run(split):
        if split:
            pkg.blocks.tcn_step_split_launch(*common, native.ptr(ops["w_split"]), *res, native.ptr(ops["w_res_split"]), *tail,
                                             native.stream_of(y))
        else:
            pkg.blocks.tcn_step_launch(*common, native.ptr(ops["w"]), *res, native.ptr(ops["w_res"]), *tail, 1, None, native.stream_of(y))
    run(False)
    ref = out[:n_emit].clone()
    run(True)
    err = float((ref - out[:n_emit]).abs().max())
    reps = {False: [], True: []}
    for _ in range(3):
        times = {False: [], True: []}
        for _ in range(rounds):
            for split in (False, True):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(3):
                    run(split)
                e1.record()
                torch.cuda.synchronize()
                times[split].append(e0.elapsed_time(e1) / 3)
        for k in times:
            reps[k].append(statistics.median(times[k]))
    m32, m3 = statistics.median(reps[False]), statistics.median(reps[True])
    spread = max(max(r) - min(r) for r in reps.values())
    print(f"STEP_SPLIT_AB {ci}->{co} s{s} emit {n_emit}: f32 {m32:.4f} ms {['%.4f' % r for r in reps[False]]}  bf16x3 {m3:.4f} ms "
          f"{['%.4f' % r for r in reps[True]]}  spread {spread:.4f} ms  speedup {m32 / m3:.3f}x  "
          f"{'WIN' if m32 - m3 > spread else 'no win'}  max|diff| {err:.2e}  |out|max {float(ref.abs().max()):.2f}", flush=True)


def fps(net, x4, n):
    for _ in range(24):                              # past the stack's delay: every layer emits
        net.forward_cycle(x4)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        last = net.forward_cycle(x4)
    e1.record()
    torch.cuda.synchronize()
    return streams * 4 * n / (e0.elapsed_time(e1) / 1e3), last


nets = {}
for name, (plan, prec) in {"plan_f32": (True, "f32"), "python_f32": (False, "f32"), "python_bf16x3": (False, "bf16x3")}.items():
    net = pkg.CoStGcn(A, pool_size=4, pool_padding=1).eval()
    bench.randomise_(net, 0)
    net.use_native_plan = plan
    net.set_max_cycle(4)
    pkg.set_step_precision(net, prec)
    nets[name] = net.to(dev)
g = torch.Generator(device=dev).manual_seed(1)
x4 = [torch.rand((streams, 3, 25, 2), device=dev, generator=g) for _ in range(4)]
rates, logits = {k: [] for k in nets}, {}
for rep in range(3):
    for name, net in nets.items():
        net.clean_state()
        r, last = fps(net, x4, cycles)
        rates[name].append(r)
        logits[name] = last[-1]
for name in nets:
    print(f"STEP_SPLIT_CYCLE {name}: {statistics.median(rates[name]) / 1e3:.1f} k frames/s {['%.1f' % (r / 1e3) for r in rates[name]]}  "
          f"state {nets[name].state_bytes() / 1e9:.3f} GB", flush=True)
print(f"STEP_SPLIT_CYCLE max |logit difference| bf16x3 vs f32 (python engine): "
      f"{float((logits['python_bf16x3'] - logits['python_f32']).abs().max()):.3e}  |logit|max {float(logits['python_f32'].abs().max()):.2f}; "
      f"plan vs python f32 equal: {bool(torch.equal(logits['plan_f32'], logits['python_f32']))}")
