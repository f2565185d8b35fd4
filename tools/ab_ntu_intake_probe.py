#!/usr/bin/env python3
"""Cost of the NTU body intake (ntu_intake.py, csrc/ntu_intake.hip), measured, no bar:
  * the entry alone (csk_ntu_intake_f32) at `clips` clips, P = 4, V = 25, M = 2, 300 output frames, for recordings of T = 70
    (the usual NTU length) and T = 300 frames: HIP events around batches of 50 back-to-back launches, the median batch over 7,
    per launch; the bytes it must move are computed from the shapes (read N T P V 3 words, write N 3 T_out V M words; the two
    reduction passes and the gather read the clip again, from cache or not);
  * the StGcn NTU-shape clip forward with the switch off (fed the selected clip) and on (fed the T = 70 bodies): two models with
    the same weights in one process, timed in alternating rounds of 5 forwards, HIP events per forward, the median of each
    round and the median over the rounds;
  * the library calls of one forward with the switch off and on (a counting wrapper around the library).
Writes what it measured to profiles/r22_ntu_intake.md (and prints it).  One process, straight-line: a step that raises ends the
script, nothing is started after it.
usage: python tools/ab_ntu_intake_probe.py [clips] [rounds] [out.md]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import _bootstrap  # noqa: E402
import bench  # noqa: E402

pkg = _bootstrap.load()
ntu_intake, native = pkg.ntu_intake, pkg.native
dev = "cuda:0"
clips = int(sys.argv[1]) if len(sys.argv) > 1 else 256
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r22_ntu_intake.md")
P, V, M, T_OUT = 4, 25, 2, 300
forwards, batch = 5, 50
lines = []


def say(text):
    print("NTU_AB " + text, flush=True)
    lines.append(text)


def bodies(n, t, gen):
    """Two tracked bodies per clip (slots drawn per clip), the second one appearing late; the other slots all zero."""
    b = torch.zeros((n, t, P, V, 3), device=dev)
    slots = torch.rand((n, P), device=dev, generator=gen).argsort(dim=1)
    late = torch.randint(0, t // 2 + 1, (n,), device=dev, generator=gen)
    x = torch.randn((n, t, 2, V, 3), device=dev, generator=gen)
    x[:, :, 1] *= 0.5
    x[:, :, 1] *= (torch.arange(t, device=dev)[None, :] >= late[:, None])[:, :, None, None]
    idx = torch.arange(n, device=dev)
    b[idx, :, slots[:, 0]] = x[:, :, 0]
    b[idx, :, slots[:, 1]] = x[:, :, 1]
    return b


g = torch.Generator(device=dev).manual_seed(1)
lib = native.lib()

# ---- the entry alone ---------------------------------------------------------------------------------------------------------
clip70 = None
for t in (70, 300):
    b = bodies(clips, t, g)
    clip70 = b if t == 70 else clip70
    out = torch.empty((clips, 3, T_OUT, V, M), device=dev)
    stream = native.stream_of(b)

    def launch():
        native.check(lib.csk_ntu_intake_f32(native.ptr(b), native.ptr(out), clips, t, P, V, M, T_OUT, stream), "csk_ntu_intake_f32")

    for _ in range(10):
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
    moved = 4 * clips * (t * P * V * 3 + 3 * T_OUT * V * M)
    us = statistics.median(per_launch)
    say(f"entry alone, {clips} clips, T = {t} -> {T_OUT} frames, P = {P}, V = {V}, M = {M}: {us:.1f} us per launch back to back (median "
        f"of 7 batches of {batch}; min {min(per_launch):.1f}, max {max(per_launch):.1f}); operands: {moved / 1e6:.1f} MB read once and "
        f"written once = {moved / us / 1e6:.2f} TB/s at that time (the operands stay in the 256 MiB Infinity Cache between launches)")


# ---- the clip forward, switch off and on, alternating ------------------------------------------------------------------------------
def model(on):
    net = pkg.StGcn(pkg.ntu_graph().A, (3, T_OUT, V, M), 60).eval()
    bench.randomise_(net, 0)
    if on:
        ntu_intake.set_ntu_intake(net, bodies_in=P)
    return net.to(dev)


def round_ms(net, x):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(forwards + 1)]
    for i in range(forwards):
        ev[i].record()
        net(x)
    ev[forwards].record()
    torch.cuda.synchronize()
    return statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(forwards))


off, on = model(False), model(True)
selected = ntu_intake.select_bodies_clip(clip70, T_OUT, M)          # what the switch-off model is fed
with torch.no_grad():
    for _ in range(3):
        a, c = off(selected), on(clip70)
    torch.cuda.synchronize()
    assert torch.equal(a, c), "the two models must compute the same logits"
    t_off, t_on = [], []
    for _ in range(rounds):
        t_off.append(round_ms(off, selected))
        t_on.append(round_ms(on, clip70))
m_off, m_on = statistics.median(t_off), statistics.median(t_on)
say(f"StGcn NTU-shape clip forward ({clips} clips of {T_OUT} frames; switch on: fed T = 70 bodies), {rounds} alternating rounds of "
    f"{forwards} forwards, median forward of each round in ms -- switch off: {' '.join(f'{t:.3f}' for t in t_off)}; switch on: "
    f"{' '.join(f'{t:.3f}' for t in t_on)}")
say(f"median over the rounds: off {m_off:.3f} ms, on {m_on:.3f} ms: {1e3 * (m_on - m_off):+.0f} us per forward, "
    f"{100 * (m_on / m_off - 1):+.2f} %; spread of the rounds: off {100 * (max(t_off) / min(t_off) - 1):.2f} %, on "
    f"{100 * (max(t_on) / min(t_on) - 1):.2f} % (the switch-on forward also allocates the selected clip, "
    f"{selected.numel() * 4 / 1e6:.1f} MB)")

# ---- library calls of one forward ------------------------------------------------------------------------------------------------
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


for name, net, x in (("off", off, selected), ("on", on, clip70)):
    native._lib = counting = Counting()
    with torch.no_grad():
        net(x)
    native._lib = real
    torch.cuda.synchronize()
    say(f"library calls of one forward, switch {name}: {dict(sorted(counting.count.items()))}")

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("# r22: NTU body intake -- measured, no bar\n\n"
            "Written by `tools/ab_ntu_intake_probe.py` on one MI355X; the numbers are what that run measured, not a verdict.\n"
            "Times are HIP-event times; the two models of the forward comparison ran in one process, in alternating rounds.\n\n")
    f.writelines(f"- {line}\n" for line in lines)
print(f"NTU_AB wrote {out_path}", flush=True)
