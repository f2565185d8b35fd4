#!/usr/bin/env python3
"""A/B figures of the clip-as-steps work, written to profiles/r24_clip_as_steps.md (or --out):
  head    csk_co_head_clip_f32 against the composition it replaces -- the CSK_PRIME_POOL job of csk_co_prime_pack_f32 (+ the
          copy that puts its [stream][entry] output into [entry][stream] order), csk_co_window_mean_f32 once per prediction,
          csk_fc_f32 -- at N = 256, C = 256, NTU (V 25, 60 classes) and Kinetics (V 18, 400 classes), n_pred in {1, 16, 189}
          (1: CoStGcn's default head at T = 300; 189: CoStGcnMod at T = 300 with pool_size 32), in alternation, median of repeats;
  models  forward_clip_as_steps against clean_state(); forward_steps for CoStGcn (NTU, batch 256, T = 300) and CoStGcnMod
          (batch 64, pool_size 32);
  prime   CoAGcn.prime_state_as_steps + import_streams for 1, 16, 64 streams at T = 300 against stepping a staging slab and
          moving it.
Without --part the script is the driver: every part runs as a child process under its own time limit, in order, and the first
one that fails ends the run; the parts' lines are collected into the report.
usage: python tools/ab_clip_as_steps_probe.py [--out FILE] [--part head|models|prime] [--repeats K]"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARTS = {"head": 300, "models": 420, "prime": 420}          # seconds each part may take


def driver(args):
    lines = ["# r24: a stored clip at the steps' arithmetic -- one-call head, clip-as-steps, CoAGcn priming", "",
             "Written by `tools/ab_clip_as_steps_probe.py`; HIP events, medians of alternating repeats, one MI355X.", ""]
    for part, limit in PARTS.items():
        res = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part,
                              "--repeats", str(args.repeats)], capture_output=True, text=True, cwd=ROOT)
        keep = [ln for ln in res.stdout.splitlines() if ln.startswith("R24 ")]
        lines += [f"## {part}", ""] + [f"- {ln[4:]}" for ln in keep] + [""]
        print("\n".join(keep), flush=True)
        if res.returncode != 0:
            lines += [f"part `{part}` ended with exit status {res.returncode}; nothing was started after it.", ""]
            print(res.stdout[-2000:], res.stderr[-4000:], sep="\n", flush=True)
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    return res.returncode


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def alternate(a, b, repeats):
    """Medians (ms) of ``a`` and ``b`` run in alternation, after one warm-up of each."""
    a(), b()
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(timed(a)[0])
        tb.append(timed(b)[0])
    return statistics.median(ta), statistics.median(tb)


def part_head(repeats):
    import torch
    import _bootstrap
    pkg = _bootstrap.load()
    native, dev = pkg.native, "cuda:0"
    lib = native.lib()
    n, m, c = 256, 2, 256
    g = torch.Generator(device=dev).manual_seed(1)
    for shape, v, classes in (("NTU", 25, 60), ("Kinetics", 18, 400)):
        w, b = torch.randn((classes, c), device=dev, generator=g), torch.randn((classes,), device=dev, generator=g)
        for n_pred, frames, window, first in ((1, 56, 75, 55), (16, 75, 60, 59), (189, 220, 32, 31)):
            h = torch.rand((n * m, c, frames, v), device=dev, generator=g)
            stream = native.stream_of(h)
            entries = torch.empty((frames, n, c), device=dev)
            pooled, logits = torch.empty((n_pred, n, c), device=dev), torch.empty((n_pred, n, classes), device=dev)
            pooled2, logits2 = torch.empty_like(pooled), torch.empty_like(logits)
            packed, ring = torch.empty((n, frames * c), device=dev), torch.zeros((first + n_pred + window, n, c), device=dev)
            job = (native.PrimeJob * 1)(native.PrimeJob(h.data_ptr(), 0, native.PRIME_POOL, c, frames, 0, frames, 0))

            def one():
                native.check(lib.csk_co_head_clip_f32(native.ptr(h), frames, frames, native.ptr(entries), window, first, n_pred, native.ptr(w),
                                                      native.ptr(b), native.ptr(pooled), native.ptr(logits), n, m, c, v, classes, stream), "clip")

            def composed():
                native.check(lib.csk_co_prime_pack_f32(ctypes.byref(job), 1, native.ptr(packed), frames * c, n, m, v, stream), "pack")
                ring[:frames] = packed.view(n, frames, c).permute(1, 0, 2)
                for k in range(n_pred):
                    e = first + k
                    lo = max(0, e + 1 - window)
                    native.check(lib.csk_co_window_mean_f32(native.ptr(ring[lo]), native.ptr(pooled2[k]), n * c, window, e - lo, e - lo + 1,
                                                            stream), "mean")
                native.check(lib.csk_fc_f32(native.ptr(pooled2), native.ptr(w), native.ptr(b), native.ptr(logits2), n_pred * n, c, classes,
                                            stream), "fc")

            t_one, t_cmp = alternate(one, composed, repeats)
            same = torch.equal(logits.view(torch.int32), logits2.view(torch.int32))
            print(f"R24 head {shape} N={n} C={c} frames={frames} window={window} n_pred={n_pred}: one call {t_one:.3f} ms, composed "
                  f"({n_pred + 3} launches) {t_cmp:.3f} ms, composed / one call = {t_cmp / t_one:.2f}, same bits: {same}", flush=True)
            del h


def part_models(repeats):
    import torch
    import _bootstrap
    import bench
    pkg = _bootstrap.load()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(2)
    for name, cls, batch, pool in (("CoStGcn", pkg.CoStGcn, 256, (-1, -1)), ("CoStGcnMod", pkg.CoStGcnMod, 64, (32, 0))):
        net = cls(pkg.ntu_graph().A, pool_size=pool[0], pool_padding=pool[1]).eval()
        bench.randomise_(net, 0)
        net = net.to(dev)
        x = torch.rand((batch, 3, 300, 25, 2), device=dev, generator=g)

        def clip():
            return net.forward_clip_as_steps(x)

        def steps():
            net.clean_state()
            return net.forward_steps(x)

        t_clip, t_steps = alternate(clip, steps, repeats)
        a, b = clip(), steps()
        ratio = float((a - b).abs().max() / b.abs().max())
        print(f"R24 models {name} NTU batch {batch} T=300 pool_size {net.pool_size}: forward_clip_as_steps {t_clip:.1f} ms "
              f"({tuple(a.shape)}), clean_state + forward_steps {t_steps:.1f} ms, steps / clip = {t_steps / t_clip:.1f}, "
              f"max|clip-steps|/max|steps| = {ratio:.2e}", flush=True)
        del net, x


def part_prime(repeats):
    import torch
    import _bootstrap
    import bench
    pkg = _bootstrap.load()
    dev, T, streams = "cuda:0", 300, 64

    def slab():
        net = pkg.CoAGcn(pkg.ntu_graph().A, pool_size=4, pool_padding=0).eval()
        bench.randomise_(net, 0)
        net.set_max_cycle(4)
        return net.to(dev)

    g = torch.Generator(device=dev).manual_seed(3)
    x4 = [torch.rand((streams, 3, 25, 2), device=dev, generator=g) for _ in range(4)]
    target = slab()
    for _ in range(30):
        target.forward_cycle(x4)
    torch.cuda.synchronize()
    for k in (1, 16, 64):
        hist = torch.rand((k, 3, T, 25, 2), device=dev, generator=g)
        dst = list(range(streams - k, streams))
        stage = slab()
        w = [torch.rand((k, 3, 25, 2), device=dev, generator=g) for _ in range(4)]
        for _ in range(-(-stage._ready_age() // 4)):
            stage.forward_cycle(w)                       # warmed past its ready age: not timed
        frames = [hist[:, :, t].contiguous() for t in range(T)]
        all_k = list(range(k))

        def primed():
            target.prime_streams_as_steps(hist, dst)

        def staged():
            stage.reset_streams(all_k)
            for t in range(0, T, 4):
                stage.forward_cycle(frames[t:t + 4])
            target.import_streams(stage.export_streams(all_k), dst)

        t_pr, t_st = alternate(primed, staged, repeats)
        print(f"R24 prime CoAGcn {k} streams T={T}: prime_streams_as_steps {t_pr:.1f} ms ({t_pr / k:.2f} ms per stream), staging slab "
              f"(reset, {T // 4} cycles, export, import) {t_st:.1f} ms, staged / primed = {t_st / t_pr:.1f}", flush=True)
        del stage, frames, hist


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_clip_as_steps.md"))
    ap.add_argument("--part", choices=list(PARTS))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if args.part is None:
        sys.exit(driver(args))
    {"head": part_head, "models": part_models, "prime": part_prime}[args.part](args.repeats)
