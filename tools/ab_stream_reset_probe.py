#!/usr/bin/env python3
"""Cost of the per-stream reset (CoStGcn.reset_streams) on the online cycle: 1024 NTU streams, 4 frames per cycle, one
process, native plan.  HIP events between consecutive cycles (no sync inside a series) -> ms per cycle, median / max:
  * steady: nobody warms (the cycle that runs without the feature; the only series a build without it can run -- the script
    guards on ``hasattr(net, "reset_streams")``, so the same file gives the parent commit's figure from the parent's tree);
  * one cohort of 1, 16 and 128 streams warming: the 19 cycles after a reset during which the scrub has work (ages 0..72),
    repeated; the reset launch itself is timed apart;
  * 16 cohorts of 8 streams, rolling: every cycle re-resets the oldest cohort, so 16 cohorts are scrubbed in every cycle.
usage: python tools/ab_stream_reset_probe.py [streams] [cycles] [repeats]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import _bootstrap  # noqa: E402
import bench  # noqa: E402

pkg = _bootstrap.load()
dev = "cuda:0"
streams = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 40
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
SCRUB_CYCLES = 19                                    # cycles of 4 frames with age < 76

net = pkg.CoStGcn(pkg.ntu_graph().A, pool_size=4, pool_padding=1).eval()
bench.randomise_(net, 0)
net.set_max_cycle(4)
net = net.to(dev)
has_reset = hasattr(net, "reset_streams")
g = torch.Generator(device=dev).manual_seed(1)
x4 = [torch.rand((streams, 3, 25, 2), device=dev, generator=g) for _ in range(4)]
for _ in range(30):                                  # past the stack's delay: every layer emits, the pooling window is full
    net.forward_cycle(x4)
torch.cuda.synchronize()


def series(n, before_cycle=None):
    """ms of each of ``n`` consecutive cycles (``before_cycle(i)`` runs inside cycle i's interval)."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    for i in range(n):
        ev[i].record()
        if before_cycle:
            before_cycle(i)
        net.forward_cycle(x4)
    ev[n].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]


def report(name, reps, extra=""):
    meds = [statistics.median(r) for r in reps]
    print(f"STREAM_RESET_AB {name}: median {statistics.median(meds):.4f} ms/cycle  per repeat {['%.4f' % m for m in meds]}  "
          f"max cycle {max(max(r) for r in reps):.4f} ms  cycles/repeat {len(reps[0])}  "
          f"{streams * 4 / statistics.median(meds):.0f} k frames/s{extra}", flush=True)
    return statistics.median(meds)


steady = report("steady (no stream warming)" + ("" if has_reset else " [build without reset_streams]"),
                [series(cycles) for _ in range(repeats)])
if has_reset:
    for k in (1, 16, 128):
        idx = list(range(3, 3 + k))
        reps, resets = [], []
        for _ in range(repeats):
            times = []
            for _ in range(-(-cycles // SCRUB_CYCLES)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                net.reset_streams(idx)
                e1.record()
                times += series(SCRUB_CYCLES)
                resets.append(e0.elapsed_time(e1))
            reps.append(times)
            for _ in range(4):                       # let the cohort get ready before the next repeat
                net.forward_cycle(x4)
        m = report(f"one cohort of {k} warming", reps, f"  vs steady {100 * (statistics.median([statistics.median(r) for r in reps]) / steady - 1):+.2f} %  "
                   f"full reset launch {statistics.median(resets):.4f} ms")
    groups = [list(range(8 * j, 8 * j + 8)) for j in range(16)]
    for j in range(16):                              # fill: after 16 cycles every group is a cohort of its own
        net.reset_streams(groups[j])
        net.forward_cycle(x4)
    reps = [series(cycles, lambda i: net.reset_streams(groups[i % 16])) for _ in range(repeats)]
    n_cohorts = len(net._cohorts)
    m = statistics.median([statistics.median(r) for r in reps])
    report(f"16 cohorts of 8 warming, rolling ({n_cohorts} cohorts live, one re-reset per cycle)", reps, f"  vs steady {100 * (m / steady - 1):+.2f} %")
    for _ in range(24):
        net.forward_cycle(x4)
    again = report("steady again (every stream ready)", [series(cycles) for _ in range(repeats)])
    print(f"STREAM_RESET_AB steady again vs steady: {100 * (again / steady - 1):+.2f} %  warming cohorts left: {len(net._cohorts)}", flush=True)
