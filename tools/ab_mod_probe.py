#!/usr/bin/env python3
"""In-process timing of the unpadded "*" models.  Clip: StGcnMod at batch 256 (NTU, T = 300) with the valid Winograd route on and
off (SpatioTemporalBlock.wino_valid; the arms alternate round by round), per layer width the valid kernel against the direct
kernel on a layer-sized problem, and StGcn in the same process for orientation.  Online: CoStGcnMod at 1024 streams on the native
plan and on the Python engine, CoStGcn beside it (4-frame cycles from a warm state, per frame-step).  HIP events around every
timed region, warm-up rounds dropped, median and min - max over the rounds printed.
usage: python tools/ab_mod_probe.py   (AB_BATCH=<clips>, AB_STREAMS=<streams>, AB_ROUNDS=<rounds>, AB_ONLY=clip|layers|online)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import statistics, torch
import _bootstrap
import bench
pkg = _bootstrap.load()
dev = "cuda:0"
BATCH = int(os.environ.get("AB_BATCH", "256")); STREAMS = int(os.environ.get("AB_STREAMS", "1024"))
ROUNDS = int(os.environ.get("AB_ROUNDS", "10")); ONLY = os.environ.get("AB_ONLY", "")
A = pkg.ntu_graph().A


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def show(name, ms, unit="ms"):
    print(f"{name}: median {statistics.median(ms):.3f} {unit} (min {min(ms):.3f} - max {max(ms):.3f}, {len(ms)} rounds)", flush=True)
    return statistics.median(ms)


if ONLY in ("", "clip"):
    mod, ref = pkg.StGcnMod(A).eval(), pkg.StGcn(A).eval()
    bench.randomise_(mod, 3); bench.randomise_(ref, 3)
    mod, ref = mod.to(dev), ref.to(dev)
    x = torch.rand(BATCH, 3, 300, 25, 2, device=dev)
    res = {"wino": [], "direct": [], "stgcn": []}
    with torch.no_grad():
        for rnd in range(ROUNDS + 2):
            for arm in ("wino", "direct", "stgcn"):
                for b in mod.layers.values():
                    b.wino_valid = arm == "wino"
                ms = timed(lambda: (ref if arm == "stgcn" else mod)(x))
                if rnd >= 2:
                    res[arm].append(ms)
    w, d = show(f"StGcnMod batch {BATCH} valid Winograd route", res["wino"]), show(f"StGcnMod batch {BATCH} direct kernels", res["direct"])
    show(f"StGcn batch {BATCH}", res["stgcn"])
    print(f"direct / Winograd = {d / w:.3f}x", flush=True)
    del mod, ref, x

if ONLY in ("", "layers"):
    # the identity-residual layers of StGcnMod at their own input lengths (T - 8 (l - 1)): layers 2, 6, 9
    for c, t in ((64, 292), (128, 260), (256, 236)):
        blk = pkg.SpatioTemporalBlock(c, c, A, temporal_padding=0).eval().to(dev)
        xs = torch.rand(2 * BATCH, c, t, 25, device=dev); y = blk.gcn(xs); ops = blk._packed_ops(xs.device)
        kw = dict(relu=True, res_mode=1, x_res=xs, res_off=4)
        res = {0: [], 1: []}
        for rnd in range(ROUNDS + 2):
            for arm in (0, 1):
                ms = timed(lambda: pkg.blocks.tcn_stage(y, ops["w"], ops["bias"], c, 9, 1, 0, w_wino_valid=ops["w_wino"] if arm == 0 else None, **kw))
                if rnd >= 2:
                    res[arm].append(ms)
        w, d = show(f"layer C={c} T={t} valid Winograd", res[0]), show(f"layer C={c} T={t} direct", res[1])
        print(f"C={c}: direct / Winograd = {d / w:.3f}x", flush=True)
        del blk, xs, y

if ONLY in ("", "online"):
    for cls, plan in ((pkg.CoStGcnMod, True), (pkg.CoStGcnMod, False), (pkg.CoStGcn, True), (pkg.CoStGcn, False)):
        net = cls(A, pool_size=4, pool_padding=0).eval()
        bench.randomise_(net, 3)
        net = net.to(dev); net.use_native_plan = plan; net.set_max_cycle(4)
        frames = [torch.rand(STREAMS, 3, 25, 2, device=dev) for _ in range(4)]
        with torch.no_grad():
            for _ in range(160 // 4):               # past every block's delay (80 / 76 frames): every cycle emits
                net.forward_cycle(frames)
            ms = [timed(lambda: [net.forward_cycle(frames) for _ in range(8)]) / 32 for _ in range(ROUNDS + 2)][2:]
        show(f"{cls.__name__} {STREAMS} streams, {'native plan' if plan else 'Python engine'}, per frame-step", ms)
        del net, frames
