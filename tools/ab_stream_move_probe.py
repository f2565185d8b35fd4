#!/usr/bin/env python3
"""Cost of moving live streams between slabs (CoStGcn.export_streams / import_streams / resize_streams): 1024 NTU streams, two
ready slabs in one process, native plan, 4 frames per cycle.  HIP events around each call (no sync inside) -> ms, median of the
repeats, with the bytes moved (record_floats x 4 x streams, once out and once in), the implied GB/s and the time as a fraction
of one steady 4-frame cycle of the same model measured in this process (the cycle issues the launches it issued before the
feature existed, so that figure is also the parent's):
  * export + import of 1, 16 and 128 streams from slab A to slab B;
  * resize_streams 1024 -> 1000 (export of 1000 streams, a new slab, import).
One process, straight-line: a step that raises ends the script, nothing is started after it.
usage: python tools/ab_stream_move_probe.py [streams] [cycles] [repeats]"""
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
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
HBM_ACHIEVABLE_GBS = 6300.0                          # float4 copy on this part; a copy reads and writes every byte once


def slab():
    net = pkg.CoStGcn(pkg.ntu_graph().A, pool_size=4, pool_padding=1).eval()
    bench.randomise_(net, 0)
    net.set_max_cycle(4)
    return net.to(dev)


g = torch.Generator(device=dev).manual_seed(1)
x4 = [torch.rand((streams, 3, 25, 2), device=dev, generator=g) for _ in range(4)]
A, B = slab(), slab()
for _ in range(30):                                  # past the stack's delay and the pooling window: both slabs are ready
    A.forward_cycle(x4)
for _ in range(31):                                  # another ring position than A's
    B.forward_cycle(x4)
torch.cuda.synchronize()
assert bool(A.streams_ready().all()) and bool(B.streams_ready().all())


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def cycle_ms(net, frames):
    meds = []
    for _ in range(3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(cycles + 1)]
        for i in range(cycles):
            ev[i].record()
            net.forward_cycle(frames)
        ev[cycles].record()
        torch.cuda.synchronize()
        meds.append(statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(cycles)))
    return statistics.median(meds)


steady = cycle_ms(A, x4)
print(f"STREAM_MOVE_AB steady cycle ({streams} streams, 4 frames): {steady:.4f} ms  {streams * 4 / steady:.0f} k frames/s", flush=True)
record_bytes = A.record_floats() * 4
print(f"STREAM_MOVE_AB record: {A.record_floats()} floats = {record_bytes / 1e6:.3f} MB per stream, {len(A._move_jobs()[0])} jobs per launch", flush=True)

for k in (1, 16, 128):
    k = min(k, streams)
    src, dst = list(range(3, 3 + k)), list(range(streams - k, streams))
    A.export_streams(src)                            # the allocator has seen the size: the timed calls allocate from its cache
    ex, im = [], []
    for _ in range(repeats):
        t_ex, state = timed(lambda: A.export_streams(src))
        t_im, _ = timed(lambda: B.import_streams(state, dst))
        ex.append(t_ex)
        im.append(t_im)
    e, i = statistics.median(ex), statistics.median(im)
    moved = record_bytes * k                         # each direction reads them once and writes them once
    print(f"STREAM_MOVE_AB move {k} streams: export {e:.4f} ms ({2 * moved / e / 1e6:.0f} GB/s read+write, "
          f"{100 * 2 * moved / e / 1e6 / HBM_ACHIEVABLE_GBS:.1f} % of {HBM_ACHIEVABLE_GBS:.0f})  import {i:.4f} ms "
          f"({2 * moved / i / 1e6:.0f} GB/s, {100 * 2 * moved / i / 1e6 / HBM_ACHIEVABLE_GBS:.1f} %)  bytes {moved} out + {moved} in  "
          f"export+import = {(e + i) / steady:.3f} of a cycle", flush=True)
    del state

after = cycle_ms(A, x4)
print(f"STREAM_MOVE_AB steady cycle after the moves: {after:.4f} ms ({100 * (after / steady - 1):+.2f} %)", flush=True)
keep_n = max(1, streams - 24)
t_rs, _ = timed(lambda: B.resize_streams(keep_n, list(range(keep_n))))
moved = record_bytes * keep_n
print(f"STREAM_MOVE_AB resize {streams} -> {keep_n}: {t_rs:.3f} ms (export + bind of a zeroed slab + plan + import; "
      f"{moved} bytes out + {moved} in, {4 * moved / t_rs / 1e6:.0f} GB/s over all four passes)  = {t_rs / steady:.2f} cycles", flush=True)
small = [x[:keep_n].contiguous() for x in x4]
resized = cycle_ms(B, small)
print(f"STREAM_MOVE_AB cycle of the resized slab ({keep_n} streams): {resized:.4f} ms  {keep_n * 4 / resized:.0f} k frames/s", flush=True)
