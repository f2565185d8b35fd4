#!/usr/bin/env python3
"""S-TR / CoS-TR throughput on one GPU, with ST-GCN / CoST-GCN timed in the same process for context, and the per-kernel
cost of the attention unit (csk_str_unit_f32) from a separate ``rocprofv3 --kernel-trace --stats`` child run.

Prints one JSON line:
  str_clip      STr clip forward, NTU shape (3, 300, 25, 2), batch 256: clips/s (and StGcn's, and the ratio)
  costr_online  CoSTr online, 1024 streams, 4 frames per call (Python step engine): skeleton frames/s (and CoStGcn's
                native-plan rate)
  unit_kernels  per STr layer shape of the unit (N*M = 512 sequences): average time of each of its three launches and
                the achieved fraction of the 157.3 TFLOP/s fp32 MFMA peak for the two GEMM launches
usage: python tools/str_bench.py [--batch 256] [--streams 1024] [--no-profile] [--out DIR]
       (--kernel-pass: the child run under the profiler; not for direct use)
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import _bootstrap  # noqa: E402
import bench  # noqa: E402

pkg = _bootstrap.load()
DEV = "cuda:0"
PEAK = 157.3e12
SHAPE = (3, 300, 25, 2)
# (C_in, C_out, frames) of the unit in STr layers 4-10 (the block stride sits in the temporal conv, after the unit)
UNIT_LAYERS = [(64, 64, 300), (64, 128, 300), (128, 128, 150), (128, 256, 150), (256, 256, 75)]
KERNEL_REPS = 5


def timeit(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def clip_rates(batch, iters):
    A = pkg.ntu_graph().A
    x = torch.rand((batch,) + SHAPE, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    out = {}
    with torch.no_grad():
        for name, cls in (("stgcn", pkg.StGcn), ("str", pkg.STr)):
            net = cls(A, SHAPE, 60).eval()
            bench.randomise_(net, 0)
            net = net.to(DEV)
            dt = timeit(lambda: net(x), iters)
            out[name] = dict(ms_per_step=round(dt * 1e3, 2), clips_per_s=round(batch / dt, 1))
            del net
            torch.cuda.empty_cache()
    out["str_over_stgcn"] = round(out["str"]["clips_per_s"] / out["stgcn"]["clips_per_s"], 3)
    return out


def online_rates(streams, cycles):
    A = pkg.ntu_graph().A
    frames = torch.rand((8, streams) + (3, 25, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    out = {}
    with torch.no_grad():
        for name, cls in (("costgcn_native_plan", pkg.CoStGcn), ("costr", pkg.CoSTr)):
            net = cls(A, SHAPE, 60).eval()
            bench.randomise_(net, 0)
            net = net.to(DEV)
            for c in range(25):                     # 100 frames: past the receptive field, every block emits
                net.forward_cycle([frames[(4 * c + f) % 8] for f in range(4)])
            i = [0]

            def cyc():
                net.forward_cycle([frames[(i[0] + f) % 8] for f in range(4)])
                i[0] += 4
            dt = timeit(cyc, cycles, warm=1)
            out[name] = dict(ms_per_frame_step=round(dt / 4 * 1e3, 3), frames_per_s=round(4 * streams / dt, 1),
                             native_plan="_plan" in net.__dict__)
            del net
            torch.cuda.empty_cache()
    out["costr_over_costgcn"] = round(out["costr"]["frames_per_s"] / out["costgcn_native_plan"]["frames_per_s"], 3)
    return out


def kernel_pass(nm):
    """The unit alone at every STr layer shape, KERNEL_REPS times each, in UNIT_LAYERS order (the parent attributes the
    dispatches by that order)."""
    A = pkg.ntu_graph().A
    with torch.no_grad():
        for ci, co, t in UNIT_LAYERS:
            m = pkg.GcnUnitAttention(ci, co, A).eval()
            bench.randomise_(m, 0)
            m = m.to(DEV)
            x = torch.rand((nm, ci, t, 25), device=DEV)
            for _ in range(KERNEL_REPS):
                m(x)
            torch.cuda.synchronize()
            del m, x
            torch.cuda.empty_cache()


def unit_kernels(out_dir, nm):
    d = os.path.join(out_dir, "str_kernels")
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--kernel-pass", "--nm", str(nm)]
    rc = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
    if rc.returncode != 0:
        return dict(error=f"rocprofv3 child exited {rc.returncode}: {rc.stderr.decode()[-400:]}")
    trace = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)[-1]
    rows = [r for r in csv.DictReader(open(trace)) if "str_gemm_kernel" in r["Kernel_Name"] or "str_attention_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = 3 * KERNEL_REPS
    if len(rows) != per * len(UNIT_LAYERS):
        return dict(error=f"expected {per * len(UNIT_LAYERS)} unit dispatches, traced {len(rows)}")
    table = []
    for li, (ci, co, t) in enumerate(UNIT_LAYERS):
        chunk = rows[li * per:(li + 1) * per]
        us = [[(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in chunk[k::3][1:]] for k in range(3)]   # first rep = warm-up
        avg = [sum(u) / len(u) for u in us]
        cols = nm * t * 25
        f_qkv = 2.0 * cols * ci * (co // 2 + co)
        f_out = 2.0 * cols * co * co
        table.append(dict(layer=f"{ci}->{co} T={t}", qkv_gemm_us=round(avg[0], 1), attention_us=round(avg[1], 1),
                          out_gemm_us=round(avg[2], 1), qkv_gemm_frac=round(f_qkv / (avg[0] * 1e-6) / PEAK, 3),
                          out_gemm_frac=round(f_out / (avg[2] * 1e-6) / PEAK, 3),
                          unit_us=round(sum(avg), 1), gemm_share=round((avg[0] + avg[2]) / sum(avg), 3)))
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=8)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "str_bench"),
                    help="directory for the profiler child run's traces (build/ is not tracked)")
    ap.add_argument("--kernel-pass", action="store_true")
    ap.add_argument("--nm", type=int, default=512)
    a = ap.parse_args()
    if a.kernel_pass:
        return kernel_pass(a.nm)
    res = dict(tool="str_bench", batch=a.batch, streams=a.streams, str_clip=clip_rates(a.batch, a.iters),
               costr_online=online_rates(a.streams, a.cycles))
    if not a.no_profile:
        res["unit_kernels"] = unit_kernels(a.out, a.batch * SHAPE[3])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
