#!/usr/bin/env python3
"""In-process A/B of csk_tcn_stage_wino_valid_res_f32 (the valid Winograd temporal conv with the conv residual on the centred shrink)
against the direct kernel csk_tcn_stage_f32 on the two "*" layer shapes it serves, at batch 256 (512 sequences) and their input
lengths in a T = 300 stack: L5 64 -> 128 channels, 268 frames; L8 128 -> 256 channels, 244 frames; V = 25 and V = 18.  Then whole
forwards of AGcnMod and STrMod with the route on and off (SpatioTemporalBlock.wino_valid_res on layers 5 and 8), and StGcnMod in
the same process.  The arms alternate round by round; a timed window is REPS launches (one forward) between two HIP events; the
first two rounds are warm-up and dropped; median and min - max over the rounds are printed, with the largest output difference
between the arms.  A layer "wins" where the medians differ by more than the wider of the two arms' min - max spreads.
usage: python tools/ab_wino_valid_res_probe.py   (AB_BATCH=<clips>, AB_ROUNDS=<rounds>, AB_REPS=<launches per window>, AB_ONLY=layers|models)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import statistics, torch
import _bootstrap
import bench
pkg = _bootstrap.load()
dev = "cuda:0"
BATCH = int(os.environ.get("AB_BATCH", "256")); ROUNDS = int(os.environ.get("AB_ROUNDS", "10")); REPS = int(os.environ.get("AB_REPS", "5"))
ONLY = os.environ.get("AB_ONLY", "")
if not torch.cuda.is_available():
    raise SystemExit("no GPU: nothing is measured without one")


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def show(name, ms):
    print(f"{name}: median {statistics.median(ms):.3f} ms (min {min(ms):.3f} - max {max(ms):.3f}, {len(ms)} rounds)", flush=True)
    return statistics.median(ms), max(ms) - min(ms)


def verdict(name, new, old):
    (mn, sn), (mo, so) = new, old
    wins = mo - mn > max(sn, so)
    print(f"{name}: direct / Winograd = {mo / mn:.3f}x, spread {max(sn, so):.3f} ms -> {'faster than the direct kernel by more than the spread' if wins else 'NOT faster by more than the spread'}", flush=True)


if ONLY in ("", "layers"):
    for v in (25, 18):
        A = (pkg.ntu_graph() if v == 25 else pkg.kinetics_graph()).A
        for name, ci, co, t in (("L5", 64, 128, 268), ("L8", 128, 256, 244)):
            blk = pkg.SpatioTemporalBlock(ci, co, A, temporal_padding=0).eval()
            bench.randomise_(blk, 3)
            blk = blk.to(dev)
            with torch.no_grad():
                xs = torch.rand(2 * BATCH, ci, t, v, device=dev); y = blk.gcn(xs); ops = blk._packed_ops(xs.device)
                out = torch.empty((2 * BATCH, co, t - 8, v), device=dev)
                kw = dict(relu=True, res_mode=2, x_res=xs, w_res=ops["w_res"], res_off=4, out=out)
                run = {0: lambda: pkg.blocks.tcn_stage(y, ops["w"], ops["bias"], co, 9, 1, 0, w_wino_valid_res=ops["w_wino"], **kw),
                       1: lambda: pkg.blocks.tcn_stage(y, ops["w"], ops["bias"], co, 9, 1, 0, **kw)}
                a = run[0]().clone(); d = run[1]()
                diff, ref = float((a - d).abs().max()), float(d.abs().max())
                res = {0: [], 1: []}
                for rnd in range(ROUNDS + 2):
                    for arm in (0, 1):
                        ms = timed(run[arm], REPS)
                        if rnd >= 2:
                            res[arm].append(ms)
            tag = f"{name} {ci}->{co} T={t} V={v} x{2 * BATCH}"
            verdict(tag, show(f"{tag} valid Winograd + conv residual", res[0]), show(f"{tag} direct", res[1]))
            print(f"{tag}: max |Winograd - direct| = {diff:.3e} (max |direct| {ref:.3f})", flush=True)
            del blk, xs, y, out, a, d

if ONLY in ("", "models"):
    A = pkg.ntu_graph().A
    x = torch.rand(BATCH, 3, 300, 25, 2, device=dev)
    for cls in (pkg.agcn.AGcnMod, pkg.str.STrMod):
        net = cls(A).eval()
        bench.randomise_(net, 3)
        net = net.to(dev)
        res = {True: [], False: []}
        with torch.no_grad():
            for rnd in range(ROUNDS + 2):
                for arm in (True, False):
                    for i in (5, 8):
                        net.layers[f"layer{i}"].wino_valid_res = arm
                    ms = timed(lambda: net(x))
                    if rnd >= 2:
                        res[arm].append(ms)
        tag = f"{cls.__name__} batch {BATCH}"
        verdict(tag, show(f"{tag} layers 5, 8 on the valid Winograd form", res[True]), show(f"{tag} layers 5, 8 on the direct kernel", res[False]))
        del net
    ref = pkg.StGcnMod(A).eval()
    bench.randomise_(ref, 3)
    ref = ref.to(dev)
    with torch.no_grad():
        show(f"StGcnMod batch {BATCH} (layers 5, 8 on the direct kernel)", [timed(lambda: ref(x)) for _ in range(ROUNDS + 2)][2:])
