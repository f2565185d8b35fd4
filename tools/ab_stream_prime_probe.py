#!/usr/bin/env python3
"""Cost of priming streams from buffered history (CoStGcn.prime_state + import_streams) against the only route the tree had
before it: stepping the same history through a warmed staging slab, then export_streams + import_streams.  NTU model
(pool_size=4, pool_padding=0), histories of T = 300 frames, 1, 16 and 64 streams, one process:
  * prime:  prime_state(x_hist) (the clip pass in chunks under prime_budget_bytes + one pack launch per chunk), then
            import_streams into a ready target slab -- HIP events around each call, no sync inside, median of the repeats;
  * stage:  a staging slab of k streams, warmed past _ready_age() beforehand (not timed), then timed: reset_streams(all),
            T / 4 four-frame cycles over the history, export_streams, import_streams into the target;
  * the target slab's steady 4-frame cycle before and after, with nothing being primed (a cycle issues the launches it issued
    before the feature existed; the launch count of one cycle is printed from a counting wrapper around the library).
One process, straight-line: a step that raises ends the script, nothing is started after it.
usage: python tools/ab_stream_prime_probe.py [target_streams] [history_frames] [repeats]"""
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
T = int(sys.argv[2]) if len(sys.argv) > 2 else 300
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
cycles = 40


def slab():
    net = pkg.CoStGcn(pkg.ntu_graph().A, pool_size=4, pool_padding=0).eval()
    bench.randomise_(net, 0)
    net.set_max_cycle(4)
    return net.to(dev)


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


g = torch.Generator(device=dev).manual_seed(1)
x4 = [torch.rand((streams, 3, 25, 2), device=dev, generator=g) for _ in range(4)]
target = slab()
for _ in range(30):
    target.forward_cycle(x4)
torch.cuda.synchronize()
assert bool(target.streams_ready().all())
steady = cycle_ms(target, x4)
print(f"STREAM_PRIME_AB steady cycle ({streams} streams, 4 frames): {steady:.4f} ms  {streams * 4 / steady:.0f} k frames/s", flush=True)
print(f"STREAM_PRIME_AB record {target.record_floats() * 4 / 1e6:.3f} MB per stream; intermediates of the clip pass "
      f"{target.prime_stream_bytes(T) / 1e6:.1f} MB per stream at T = {T}, budget {target.prime_budget_bytes / 2 ** 30:.2f} GiB "
      f"= {max(1, target.prime_budget_bytes // target.prime_stream_bytes(T))} streams per chunk", flush=True)

for k in (1, 16, 64):
    k = min(k, streams)
    hist = torch.rand((k, 3, T, 25, 2), device=dev, generator=g)
    dst = list(range(streams - k, streams))
    state = target.prime_state(hist)                 # warm-up: code objects, the allocator has seen the sizes
    target.import_streams(state, dst)
    del state
    pr, im = [], []
    for _ in range(repeats):
        t_pr, state = timed(lambda: target.prime_state(hist))
        t_im, _ = timed(lambda: target.import_streams(state, dst))
        pr.append(t_pr)
        im.append(t_im)
        del state
    p, i = statistics.median(pr), statistics.median(im)
    # the route of the parent commit: a staging slab of k streams steps the history, then export + import
    stage = slab()
    w = [torch.rand((k, 3, 25, 2), device=dev, generator=g) for _ in range(4)]
    for _ in range(-(-stage._ready_age() // 4)):
        stage.forward_cycle(w)                       # warmed past its ready age: not timed
    frames = [hist[:, :, t].contiguous() for t in range(T)]
    torch.cuda.synchronize()
    all_k = list(range(k))

    def staged():
        stage.reset_streams(all_k)
        for t in range(0, T, 4):
            stage.forward_cycle(frames[t:t + 4])
        target.import_streams(stage.export_streams(all_k), dst)

    staged()                                         # warm-up of the k-stream launches
    torch.cuda.synchronize()
    st = statistics.median(timed(staged)[0] for _ in range(repeats))
    print(f"STREAM_PRIME_AB {k} streams, T = {T}: prime_state {p:.3f} ms + import_streams {i:.3f} ms = {p + i:.3f} ms "
          f"({(p + i) / k:.3f} ms per stream, {(p + i) / steady:.2f} cycles of the target)  |  staging slab (reset, {T // 4} cycles, "
          f"export, import) {st:.3f} ms ({st / k:.3f} ms per stream)  |  ratio staged / primed {st / (p + i):.1f}", flush=True)
    del stage, frames, hist

after = cycle_ms(target, x4)
print(f"STREAM_PRIME_AB steady cycle after the primes: {after:.4f} ms ({100 * (after / steady - 1):+.2f} %)", flush=True)

# launches of one steady cycle: every library entry the cycle calls, counted through a wrapper (the same count as before the
# feature: the cycle's code path has no new branch)
real, count = pkg.native.lib(), {}


class Counting:
    def __getattr__(self, name):
        fn = getattr(real, name)

        def call(*a):
            count[name] = count.get(name, 0) + 1
            return fn(*a)
        return call


pkg.native._lib = Counting()
target.forward_cycle(x4)
pkg.native._lib = real
torch.cuda.synchronize()
print(f"STREAM_PRIME_AB library calls of one steady cycle: {dict(sorted(count.items()))}", flush=True)
