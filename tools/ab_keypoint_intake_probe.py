#!/usr/bin/env python3
"""Cost of the Kinetics keypoint intake (keypoints.py, csrc/keypoints.hip), measured, no bar:
  * the frames entry alone (csk_select_people_frames_f32) at 1024 streams, r = 4, P = 5, V = 18, M = 2: HIP events around
    batches of 200 back-to-back launches, the median batch over 7, per launch; the bytes it must move are computed from the
    shapes (read r N P V 3 words, write r N 3 V M words);
  * the CoStGcn Kinetics-shape online cycle (pool_size=4, pool_padding=0, set_max_cycle(4), 4 frames per cycle) with the
    switch off (fed the selected frames) and on (fed the keypoint frames): two slabs with the same weights in one process,
    warmed past their ready age, timed in alternating rounds of 40 cycles, HIP events per cycle, the median of each round
    and the median over the rounds;
  * the library calls of one steady cycle with the switch off and on (a counting wrapper around the library).
Writes what it measured to profiles/r21_keypoint_intake.md (and prints it).  One process, straight-line: a step that raises
ends the script, nothing is started after it.
usage: python tools/ab_keypoint_intake_probe.py [streams] [rounds] [out.md]"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import _bootstrap  # noqa: E402
import bench  # noqa: E402

pkg = _bootstrap.load()
keypoints, native = pkg.keypoints, pkg.native
dev = "cuda:0"
streams = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r21_keypoint_intake.md")
R, P, V, M = 4, 5, 18, 2
cycles, batch = 40, 200
lines = []


def say(text):
    print("KEYPOINT_AB " + text, flush=True)
    lines.append(text)


def people(n, gen):
    k = torch.rand((n, P, V, 3), device=dev, generator=gen)
    k[..., 2] = torch.where(torch.rand((n, P, V), device=dev, generator=gen) < 1 / 6, torch.zeros((), device=dev), k[..., 2])
    return k


g = torch.Generator(device=dev).manual_seed(1)
k4 = [people(streams, g) for _ in range(R)]

# ---- the frames entry alone ------------------------------------------------------------------------------------------------
dsts = [torch.empty((streams, 3, V, M), device=dev) for _ in range(R)]
src = (ctypes.c_void_p * R)(*[t.data_ptr() for t in k4])
dst = (ctypes.c_void_p * R)(*[t.data_ptr() for t in dsts])
lib, stream = native.lib(), native.stream_of(k4[0])


def launch():
    native.check(lib.csk_select_people_frames_f32(src, dst, R, streams, P, V, M, stream), "csk_select_people_frames_f32")


for _ in range(20):
    launch()
torch.cuda.synchronize()
per_launch = []
for _ in range(7):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(batch):
        launch()
    e1.record()
    torch.cuda.synchronize()
    per_launch.append(e0.elapsed_time(e1) / batch * 1e3)
moved = 4 * R * streams * (P * V * 3 + 3 * V * M)
us = statistics.median(per_launch)
say(f"frames entry alone, {streams} streams, r = {R}, P = {P}, V = {V}, M = {M}: {us:.2f} us per launch back to back (median of 7 "
    f"batches of {batch}; min {min(per_launch):.2f}, max {max(per_launch):.2f}); it reads and writes {moved / 1e6:.2f} MB per launch "
    f"= {moved / us / 1e6:.2f} TB/s at that time (the operands stay in the 256 MiB Infinity Cache between launches)")


# ---- the online cycle, switch off and on, alternating ----------------------------------------------------------------------------
def slab(on):
    net = pkg.CoStGcn(pkg.kinetics_graph().A, (3, 300, V, M), 400, pool_size=4, pool_padding=0).eval()
    bench.randomise_(net, 0)
    net.set_max_cycle(4)
    if on:
        keypoints.set_keypoint_intake(net, P)
    return net.to(dev)


def round_ms(net, frames):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(cycles + 1)]
    for i in range(cycles):
        ev[i].record()
        net.forward_cycle(frames)
    ev[cycles].record()
    torch.cuda.synchronize()
    return statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(cycles))


off, on = slab(False), slab(True)
x4 = [f.contiguous() for f in keypoints.select_people_clip(torch.stack(k4, dim=1), M).unbind(dim=2)]     # what the switch-off slab is fed
for _ in range(30):
    a, b = off.forward_cycle(x4), on.forward_cycle(k4)
torch.cuda.synchronize()
assert bool(off.streams_ready().all()) and bool(on.streams_ready().all())
assert len(a) == len(b) == 1 and torch.equal(a[0], b[0]), "the two slabs must compute the same logits"
t_off, t_on = [], []
for _ in range(rounds):
    t_off.append(round_ms(off, x4))
    t_on.append(round_ms(on, k4))
m_off, m_on = statistics.median(t_off), statistics.median(t_on)
say(f"CoStGcn Kinetics-shape cycle ({streams} streams, {R} frames, native plan), {rounds} alternating rounds of {cycles} cycles, median "
    f"cycle of each round in ms -- switch off: {' '.join(f'{t:.4f}' for t in t_off)}; switch on: {' '.join(f'{t:.4f}' for t in t_on)}")
say(f"median over the rounds: off {m_off:.4f} ms ({streams * R / m_off:.0f} k frames/s), on {m_on:.4f} ms ({streams * R / m_on:.0f} k "
    f"frames/s): {1e3 * (m_on - m_off):+.1f} us per cycle, {100 * (m_on / m_off - 1):+.2f} %; spread of the rounds: off "
    f"{100 * (max(t_off) / min(t_off) - 1):.2f} %, on {100 * (max(t_on) / min(t_on) - 1):.2f} %")
say(f"scratch of the switch: {on.scratch_bytes() - off.scratch_bytes()} bytes ([max_cycle = 4]({streams}, 3, {V}, {M}) fp32); state: "
    f"{on.state_bytes() - off.state_bytes()} bytes")

# ---- library calls of one steady cycle ---------------------------------------------------------------------------------------------
real = native.lib()


class Counting:
    def __init__(self):
        self.count = {}

    def __getattr__(self, name):
        fn = getattr(real, name)

        def call(*args):
            self.count[name] = self.count.get(name, 0) + 1
            return fn(*args)
        return call


for name, net, frames in (("off", off, x4), ("on", on, k4)):
    native._lib = counting = Counting()
    net.forward_cycle(frames)
    native._lib = real
    torch.cuda.synchronize()
    say(f"library calls of one steady cycle, switch {name}: {dict(sorted(counting.count.items()))}")

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("# r21: Kinetics keypoint intake -- measured, no bar\n\n"
            "Written by `tools/ab_keypoint_intake_probe.py` on one MI355X; the numbers are what that run measured, not a verdict.\n"
            "Times are HIP-event times; the two slabs of the cycle comparison ran in one process, in alternating rounds.\n\n")
    f.writelines(f"- {line}\n" for line in lines)
print(f"KEYPOINT_AB wrote {out_path}", flush=True)
