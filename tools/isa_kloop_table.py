#!/usr/bin/env python3
"""Wait table of the MFMA segments of a kernel's K loop, from the device assembly of one .hip file.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude --cuda-device-only -S csrc/tcn_wino.hip -o tcn_wino.s
    python tools/isa_kloop_table.py tcn_wino.s 'tcn_stage_wino_kernelILi25ELb1ELi1ELb0ELb0E' [--seq]

A segment is what lies between `s_setprio 1` and `s_setprio 0`.  Per segment: the MFMAs, the LDS reads (`ds_read*`, with the
wide ones counted apart), the VALU ops, the global loads issued inside it, and every `s_waitcnt` with an lgkmcnt field that sits
behind the segment's first MFMA -- `k@m` = the wait leaves k LDS reads outstanding and stands behind the segment's m-th MFMA.
Waits in front of the first MFMA are listed as `k@0`.  --seq prints the instruction order of each segment as one string
(M mfma, r ds_read_b32, R wider read, v VALU, g global load, wK lgkmcnt(K) wait, W a wait without lgkmcnt field)."""
import re
import sys


def kernel_body(lines, needle):
    start = next(i for i, ln in enumerate(lines) if ln.startswith("_Z") and needle in ln.split(":")[0] and ln.rstrip().split(";")[0].strip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    return start, lines[start:end]


def segments(body):
    seg, out, first = None, [], None
    for off, ln in enumerate(body):
        op = ln.strip().split(" ")[0].split("\t")[0]
        if op == "s_setprio":
            if ln.split()[1] == "1":
                seg, first = [], off
            elif seg is not None:
                out.append((first, seg))
                seg = None
            continue
        if seg is None:
            continue
        if op.startswith("v_mfma"):
            seg.append("M")
        elif op.startswith("ds_read"):
            seg.append("r" if op.endswith("_b32") else "R")
        elif op.startswith("ds_write"):
            seg.append("D")
        elif op.startswith("global_load") or op.startswith("buffer_load"):
            seg.append("g")
        elif op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", ln)
            seg.append(f"w{m.group(1)}" if m else "W")
        elif op.startswith("v_"):
            seg.append("v")
        elif op.startswith("s_cbranch") or op.startswith("s_branch"):
            seg.append("|")
    return out


def main():
    path, needle = sys.argv[1], sys.argv[2]
    lines = open(path).read().splitlines()
    start, body = kernel_body(lines, needle)
    print(f"{lines[start].split(':')[0]}")
    print("| segment (asm line) | MFMA | ds_read b32 / wider | VALU | global loads | lgkmcnt waits behind the first MFMA (left@mfma) | in front |")
    print("|---|---|---|---|---|---|---|")
    for first, seg in segments(body):
        nm = 0
        inside, front = [], []
        for t in seg:
            if t == "M":
                nm += 1
            elif t[0] == "w":
                (inside if nm else front).append(f"{t[1:]}@{nm}")
        print(f"| {start + first + 1} | {seg.count('M')} | {seg.count('r')} / {seg.count('R')} | {seg.count('v')} | {seg.count('g')} | "
              f"{' '.join(inside) or '-'} | {' '.join(front) or '-'} |")
        if "--seq" in sys.argv:
            print("  `" + "".join(t if len(t) == 1 else f"({t})" for t in seg) + "`")


if __name__ == "__main__":
    main()
