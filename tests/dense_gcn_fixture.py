"""Cases, operands, fp64 references and bounds shared by tests/test_gpu_dense_gcn.py and tests/test_dense_gcn_fixture_cpu.py: the
graph conv on a DENSE adjacency (csrc/gcn_dense.hip, gcn_stage_dense_kernel and gcn_stage_kernel of csrc/gcn.hip) and the bare
1 x 1 conv csk_conv1x1_f32, at kernel level.

The operation, from its definition (models/base.py:260-270, models/a_gcn/a_gcn.py:62-69), on doubles:

    y[n, co, t, w] = ReLU( sum_r sum_c W[r, c, co] * ( sum_v x[n, c, t, v] * adj[m, r, v, w] ) + bias[co] + res(x)[n, co, t, w] )

m = 0 (one graph per launch), n (one per segment) or n * frames + t (one per frame); res = x itself (identity, c_in == c_out) or a
fourth 1 x 1 conv W[3].  The kernels get adj as the column-wise values ell_val[m][r][w][v] = adj[m, r, v, w].

exact tier   every operand is a small integer held in fp32: x in [-2, 2], adj in {-1, 0, 1, 2}, W in [-2, 2], bias in [-8, 8].  A
             partial sum of the terms of one output, taken in ANY order and grouping (the aggregation first, as the kernels do, or
             not), is an integer no larger than sum |term|, which admissible() keeps below 2^24: every fp32 operation is exact and
             the expected BITS follow from the exact sum.  Adjacencies are dense, not symmetric and drawn anew for every subset,
             segment and frame, so a transposed read, subset r + 1 for r, the neighbouring segment's or frame's matrix or the wrong
             frame at a tile seam all change the result; both signs occur, so ReLU clips 20 % .. 80 % of a case's outputs.
float tier   every operand uniform in [0.5, 1.5): all terms are positive, nothing cancels and ReLU never clips.  The sum has two
             levels.  (1) The aggregation B = fl(sum_v x adj) is a chain of V fused multiply-adds (or two chains and an add): at
             most V roundings, each relative to a partial sum that is no larger than the final one, so |B - exact| <= V u B.
             (2) The channel mix accumulates the K = R c_in_pad products W B on the matrix pipe (one rounding per accumulation, in
             whatever order), so its error is at most K u sum |W B|; the error of B passes through multiplied by W.  (3) The bias
             and the residual are two more additions.  To first order in u = 2^-24
                 |y - exact| <= (V + R c_in_pad + 2) u sum |term|,
             and bound() uses depth = V + R c_in_pad + 4 (the + 2 covers the second-order terms: depth^2 u^2 < 1e-10 here).  The
             1 x 1 conv has no aggregation: depth = c_in_pad + 3.  The bound is derived, not measured.  margin() shows it to be
             below half of the smallest single term for every float-tier case (c_in is kept small for that), so a lost, doubled or
             misplaced term fails.

Which kernel a case runs is asserted through the host query csk_gcn_stage_f32_route (include/cskel.h) -- the function the launcher
switches on -- not observed on the device.  numpy only; nothing is read from csrc."""
import ctypes
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
f32, f64 = np.float32, np.float64
RES_IDENTITY, RES_CONV = 1, 2
CPAD, MTPAD = 16, 64                       # CSK_CPAD, CSK_MT of include/cskel.h
ALIGNED = 0x10000                          # a 16-byte aligned stand-in pointer for the host-only queries

SPARSE2, TILE16, DENSE2, DENSE128, GENERAL = 1, 2, 3, 4, 5      # families of csk_gcn_stage_f32_route
UNIT = 1000000

# adj: "shared" (adj_seg_stride 0, every joint listed: ell_w = V, src[e] = e), "seg", "frame", or "ell" (a skeleton-like shared
# graph as ELL lists of `ell_w` entries of which ell_cnt[r] count).  x_off / ell_off: operand moved by that many floats off its
# 16-byte alignment.  x_pad / y_pad: floats between the rows of a channel; seg_pad: floats between segments.
Case = namedtuple("Case", "name V c_in c_out frames n_seg res adj route x_off x_pad ell_off y_pad seg_pad ell_w ell_cnt")


def case(name, V, c_in, c_out, frames, n_seg, res, adj, route, x_off=0, x_pad=0, ell_off=0, y_pad=0, seg_pad=0, ell_w=None, ell_cnt=None):
    assert res == RES_CONV or c_in == c_out
    return Case(name, V, c_in, c_out, frames, n_seg, res, adj, route, x_off, x_pad, ell_off, y_pad, seg_pad,
                V if ell_w is None else ell_w, (V, V, V) if ell_cnt is None else tuple(ell_cnt))


def mpad(c_out):
    return -(-c_out // MTPAD) * MTPAD


def cpad(c_in):
    return -(-c_in // CPAD) * CPAD


def tile_rows(c_out):
    """rows of a workgroup tile: 128 where the padded row count allows, else 64"""
    return 128 if mpad(c_out) % 128 == 0 else 64


DENSE2_FT = {18: 7, 25: 5}                 # whole frames of a 128-column tile


def _dense2_cases():
    out = []
    for V, ft in DENSE2_FT.items():
        frames = (1, ft - 1, ft, ft + 1, 2 * ft + 3)
        k = 0
        for c_out in (64, 128):
            for res in (RES_IDENTITY, RES_CONV):
                for adj in ("seg", "frame"):
                    for fi, fr in enumerate(frames):
                        c_in = c_out if res == RES_IDENTITY else (3, 8, 20, 40)[(fi + k) % 4]
                        x_pad = (0, 2)[k % 2] if V == 18 else (0, 1, 3)[k % 3]
                        route = DENSE2 * UNIT + (128 if c_out == 128 else 64) * 1000 + V * 10 + (res == RES_CONV)
                        out.append(case(f"d2-V{V}-co{c_out}-{'id' if res == 1 else 'conv'}-{adj}-T{fr}-ci{c_in}", V, c_in, c_out, fr, 2 + k % 2, res,
                                        adj, route, x_pad=x_pad, y_pad=(0, 3)[(k // 2) % 2], seg_pad=(0, 4)[k % 2]))
                        k += 1
        # the steady state of the two-chunk-ahead prefetch (c_in = 40: five chunks) on the longest run, both tile heights
        for c_out in (64, 128):
            out.append(case(f"d2-V{V}-co{c_out}-conv-seg-ci40-long", V, 40, c_out, 2 * ft + 3, 2, RES_CONV, "seg",
                            DENSE2 * UNIT + c_out * 1000 + V * 10 + 1))
        # c_out below the tile height (both heights), Mpad 192 = three 64-row tiles (130: the last one ragged), two 128-row tiles
        for c_out, mt in ((40, 64), (100, 128), (130, 64), (192, 64), (256, 128)):
            for adj in ("seg", "frame"):
                out.append(case(f"d2-V{V}-co{c_out}-conv-{adj}", V, 20, c_out, 2 * ft + 3, 2, RES_CONV, adj, DENSE2 * UNIT + mt * 1000 + V * 10 + 1,
                                y_pad=(1 if adj == "seg" else 0)))
        out.append(case(f"d2-V{V}-co192-id-frame", V, 192, 192, ft + 1, 2, RES_IDENTITY, "frame", DENSE2 * UNIT + 64000 + V * 10))
        out.append(case(f"d2-V{V}-co40-id-seg", V, 40, 40, ft + 1, 3, RES_IDENTITY, "seg", DENSE2 * UNIT + 64000 + V * 10))
    return out


DENSE2_CASES = _dense2_cases()

# V = 18 launches that gcn_dense.hip does not take (its joint pairs are 8-byte loads): dense128 at c_out = 128, general <64, 5> at 64.
# Operands are those of LEAVE_BASE (the aligned launch, dense2): the same exact reference.
LEAVE_BASE = {co: case(f"leave-base-co{co}", 18, co, co, 8, 2, RES_IDENTITY, "seg", DENSE2 * UNIT + (128 if co == 128 else 64) * 1000 + 180)
              for co in (64, 128)}
LEAVE_CASES = [LEAVE_BASE[co]._replace(name=f"leave-{what}-co{co}", route=(DENSE128 * UNIT if co == 128 else GENERAL * UNIT + 645), **kw)
               for co in (64, 128)
               for what, kw in (("x-off", dict(x_off=1)), ("odd-chan-stride", dict(x_pad=1)), ("ell-off", dict(ell_off=1)))]

# gcn_stage_dense_kernel<128, CONVRES, 8, 3>: 128 / V whole frames per tile; frames = a multiple of that + 1 leaves a one-frame tile
DENSE128_CASES = [
    case("d128-V20-id", 20, 128, 128, 7, 2, RES_IDENTITY, "seg", DENSE128 * UNIT),          # row stride 120 -> 124
    case("d128-V20-conv", 20, 20, 128, 13, 3, RES_CONV, "seg", DENSE128 * UNIT + 1, y_pad=3),
    case("d128-V19-id", 19, 128, 128, 13, 2, RES_IDENTITY, "seg", DENSE128 * UNIT, x_pad=1),  # odd V, stride 116 not padded
    case("d128-V19-conv", 19, 3, 256, 7, 2, RES_CONV, "seg", DENSE128 * UNIT + 1),
    case("d128-V4-id", 4, 128, 128, 33, 2, RES_IDENTITY, "seg", DENSE128 * UNIT),
    case("d128-V4-conv", 4, 8, 100, 1, 3, RES_CONV, "seg", DENSE128 * UNIT + 1),
    case("d128-V32-id", 32, 128, 128, 5, 2, RES_IDENTITY, "seg", DENSE128 * UNIT, y_pad=1),
    case("d128-V32-conv", 32, 40, 128, 4, 2, RES_CONV, "seg", DENSE128 * UNIT + 1),
]

GENERAL_CASES = [
    case("gen-128-3-shared-V25", 25, 128, 128, 7, 2, RES_IDENTITY, "shared", GENERAL * UNIT + 1283),
    case("gen-128-3-frame-V20", 20, 20, 128, 9, 2, RES_CONV, "frame", GENERAL * UNIT + 1283, y_pad=3),
    case("gen-128-4-shared-V40", 40, 20, 128, 5, 2, RES_CONV, "shared", GENERAL * UNIT + 1284),
    case("gen-128-4-seg-V40", 40, 128, 128, 4, 3, RES_IDENTITY, "seg", GENERAL * UNIT + 1284, x_pad=1),
    case("gen-64-5-shared-V20", 20, 64, 64, 14, 2, RES_IDENTITY, "shared", GENERAL * UNIT + 645),
    case("gen-64-5-seg-V20", 20, 3, 64, 27, 3, RES_CONV, "seg", GENERAL * UNIT + 645, x_pad=3, y_pad=1),
    case("gen-64-5-frame-V20", 20, 64, 64, 15, 2, RES_IDENTITY, "frame", GENERAL * UNIT + 645),
    case("gen-64-6-shared-V41", 41, 64, 64, 7, 2, RES_IDENTITY, "shared", GENERAL * UNIT + 646),
    case("gen-64-6-seg-V41", 41, 17, 40, 8, 2, RES_CONV, "seg", GENERAL * UNIT + 646),
]

# the sparse / general boundary: ONE skeleton-like graph (lists of 5 entries per column, all of them non-zero) of which ell_cnt
# entries count -- {1, 1, 4} is the sparse family (route filled in by boundary_routes()), one more entry in a subset is general
BOUNDARY_CASES = [case(f"boundary-{'-'.join(map(str, cnt))}", 25, 64, 64, 11, 2, RES_IDENTITY, "ell", route, ell_w=5, ell_cnt=cnt)
                  for cnt, route in (((1, 1, 4), None), ((2, 1, 4), GENERAL * UNIT + 645), ((1, 1, 5), GENERAL * UNIT + 645))]

EXACT_GROUPS = {f"dense2-{route % UNIT}": [c for c in DENSE2_CASES if c.route == route] for route in sorted({c.route for c in DENSE2_CASES})}
EXACT_GROUPS.update({"leave-dense2": list(LEAVE_BASE.values()) + LEAVE_CASES, "dense128": DENSE128_CASES, "general": GENERAL_CASES,
                     "boundary": BOUNDARY_CASES})

# float tier: one case per kernel family, c_in small enough for margin()
FLOAT_CASES = [
    case("float-dense2-V18", 18, 8, 64, 8, 2, RES_CONV, "frame", DENSE2 * UNIT + 64181, x_pad=2),
    case("float-dense2-V25", 25, 20, 128, 6, 2, RES_CONV, "seg", DENSE2 * UNIT + 128251),
    case("float-dense128", 20, 20, 128, 7, 2, RES_CONV, "seg", DENSE128 * UNIT + 1),
    case("float-general", 20, 20, 64, 14, 2, RES_CONV, "frame", GENERAL * UNIT + 645),
]

# csk_conv1x1_f32: gcn_stage_sparse2_kernel<MT, false, 16, true>, position tiles of 16384 / MT; c_out = 6 inter (inter 8, 16, 64)
Conv = namedtuple("Conv", "name V c_in c_out frames n_seg x_pad y_pad")
CONV_CASES = [Conv(f"conv-V{V}-ci{ci}-co{co}", V, ci, co, fr, 2 + (ci % 2), (ci + co) % 3, ci % 2)
              for V in (18, 25) for co, fr in ((48, 31), (96, 16), (384, 8)) for ci in (3, 16, 17, 40)]
CONV_FLOAT = [Conv("float-conv-64", 18, 17, 48, 31, 2, 1, 0), Conv("float-conv-128", 25, 40, 96, 16, 2, 0, 1)]


def family(route):
    return route // UNIT


# ---- layout -------------------------------------------------------------------------------------------------------------------
def strides(c):
    """(x_chan, x_seg, y_chan, y_seg) in floats"""
    xc = c.frames * c.V + c.x_pad
    yc = c.frames * c.V + c.y_pad
    seg_pad = getattr(c, "seg_pad", 0)
    return xc, c.c_in * xc + seg_pad, yc, c.c_out * yc + seg_pad


def n_matrices(c):
    return {"shared": 1, "ell": 1, "seg": c.n_seg, "frame": c.n_seg * c.frames}[c.adj]


def adj_args(c):
    """(adj_seg_stride, adj_per_frame) of the launch"""
    return (0 if c.adj in ("shared", "ell") else 3 * c.V * c.ell_w), int(c.adj == "frame")


def route_query(lib, c, x=ALIGNED, y=ALIGNED, ell=ALIGNED):
    """csk_gcn_stage_f32_route for the case; stand-in pointers carry the case's misalignment unless real ones are given"""
    if x == ALIGNED:
        x += 4 * c.x_off
    if ell == ALIGNED:
        ell += 4 * c.ell_off
    cnt = (ctypes.c_int32 * 3)(*c.ell_cnt)
    xc, xs, yc, ys = strides(c)
    stride, per_frame = adj_args(c)
    return lib.csk_gcn_stage_f32_route(x, y, ell, ctypes.cast(cnt, ctypes.c_void_p), c.ell_w, stride, per_frame, c.n_seg, c.c_in, c.c_out,
                                       c.frames, c.V, xs, xc, ys, yc, c.res)


def boundary_routes(lib):
    """BOUNDARY_CASES with the sparse case's route as the library reports it (sparse2 or the 16x16x4 tiles: the same sums)"""
    out = []
    for c in BOUNDARY_CASES:
        out.append(c if c.route is not None else c._replace(route=route_query(lib, c)))
    return out


# ---- operands -----------------------------------------------------------------------------------------------------------------
def _draw(rng, tier, shape, lo, hi):
    if tier == "exact":
        return rng.integers(lo, hi + 1, size=shape).astype(f32)
    return (rng.random(size=shape, dtype=f32) + f32(0.5)).astype(f32)


def operands(c, tier):
    """-> dict: x [n, c_in, T, V], adj [matrices, 3, V(v), V(w)] (what the reference sums with), w [R, c_in, c_out], bias [c_out],
    and the ELL image the kernel gets: ell_src [3, V(w), ell_w] int32, ell_val [matrices, 3, V(w), ell_w].  adj = "ell": the entries
    e >= ell_cnt[r] of ell_val are NaN (their ell_src stays a joint: a kernel may load them, none may add them); ell_val_full is the
    same graph with the drawn values in those places."""
    rng = np.random.default_rng(np.random.SeedSequence([c.V, c.c_in, c.c_out, c.frames, c.n_seg, c.res, len(c.adj), c.ell_w]))
    R = 4 if c.res == RES_CONV else 3
    x = _draw(rng, tier, (c.n_seg, c.c_in, c.frames, c.V), -2, 2)
    w = _draw(rng, tier, (R, c.c_in, c.c_out), -2, 2)
    bias = _draw(rng, tier, (c.c_out,), -8, 8)
    nm = n_matrices(c)
    if c.adj == "ell":
        src = rng.integers(0, c.V, size=(3, c.V, c.ell_w)).astype(np.int32)
        val = np.where(rng.random((1, 3, c.V, c.ell_w)) < 0.5, 1, -1) * rng.integers(1, 3, size=(1, 3, c.V, c.ell_w))
        val = val.astype(f32) if tier == "exact" else _draw(rng, tier, (1, 3, c.V, c.ell_w), 0, 0)
        adj = np.zeros((1, 3, c.V, c.V), dtype=f64)
        for r in range(3):
            for wj in range(c.V):
                for e in range(c.ell_cnt[r]):                     # the entries that count
                    adj[0, r, src[r, wj, e], wj] += val[0, r, wj, e]
        full = np.asarray(val, dtype=f32)                         # the graph before its tails are poisoned
        val = full.copy()
        for r in range(3):
            val[0, r, :, c.ell_cnt[r]:] = np.nan                  # an entry past ell_cnt must not be read into a sum
        return dict(x=x, w=w, bias=bias, adj=np.asarray(adj), ell_src=src, ell_val=val, ell_val_full=full)
    else:
        adj = _draw(rng, tier, (nm, 3, c.V, c.V), -1, 2)
        src = np.broadcast_to(np.arange(c.V, dtype=np.int32), (3, c.V, c.V)).copy()
        val = np.ascontiguousarray(np.swapaxes(adj, 2, 3))        # [m][r][w][v]
    return dict(x=x, w=w, bias=bias, adj=np.asarray(adj), ell_src=src, ell_val=np.asarray(val, dtype=f32))


def pack_w(w, bias):
    """[R, c_in, c_out] -> the packed image [R][c_in_pad][c_out_pad] and bias [c_out_pad], zero padded"""
    R, ci, co = w.shape
    img = np.zeros((R, cpad(ci), mpad(co)), dtype=f32)
    img[:, :ci, :co] = w
    b = np.zeros(mpad(co), dtype=f32)
    b[:co] = bias
    return img, b


def strided(t, chan_stride, seg_stride, fill=np.nan):
    """[n, C, T, V] -> flat buffer with the strides, `fill` between rows and segments; the last row ends the buffer"""
    n, C, T, V = t.shape
    size = (n - 1) * seg_stride + (C - 1) * chan_stride + T * V
    flat = np.full(size, fill, dtype=f32)
    for s in range(n):
        for ch in range(C):
            o = s * seg_stride + ch * chan_stride
            flat[o: o + T * V] = t[s, ch].reshape(-1)
    return flat


def unstrided(flat, shape, chan_stride, seg_stride):
    """-> (tensor [n, C, T, V], mask of the flat positions that belong to no row)"""
    n, C, T, V = shape
    out = np.empty(shape, dtype=flat.dtype)
    pad = np.ones(flat.shape, dtype=bool)
    for s in range(n):
        for ch in range(C):
            o = s * seg_stride + ch * chan_stride
            out[s, ch] = flat[o: o + T * V].reshape(T, V)
            pad[o: o + T * V] = False
    return out, pad


def out_size(c):
    xc, xs, yc, ys = strides(c)
    return (c.n_seg - 1) * ys + (c.c_out - 1) * yc + c.frames * c.V


# ---- reference ----------------------------------------------------------------------------------------------------------------
def _adj_nt(c, adj, dtype):
    """adj [matrices, 3, V, V] -> [n, T, 3, V, V]: the matrix of every (segment, frame)"""
    a = np.asarray(adj, dtype=dtype)
    if c.adj in ("shared", "ell"):
        return np.broadcast_to(a[0], (c.n_seg, c.frames) + a.shape[1:])
    if c.adj == "seg":
        return np.broadcast_to(a[:, None], (c.n_seg, c.frames) + a.shape[1:])
    return a.reshape((c.n_seg, c.frames) + a.shape[1:])


def reference(c, ops, relu=True):
    """-> (y [n, c_out, T, V] in fp64, sum |term| per output): the definition, on doubles"""
    x, w, b = f64(ops["x"]), f64(ops["w"]), f64(ops["bias"])
    a = _adj_nt(c, ops["adj"], f64)
    agg = np.einsum("nctv,ntrvw->nrctw", x, a)
    y = np.einsum("rcm,nrctw->nmtw", w[:3], agg) + b[None, :, None, None]
    mag = np.einsum("rcm,nrctw->nmtw", np.abs(w[:3]), np.einsum("nctv,ntrvw->nrctw", np.abs(x), np.abs(a))) + np.abs(b)[None, :, None, None]
    if c.res == RES_CONV:
        y += np.einsum("cm,nctw->nmtw", w[3], x)
        mag += np.einsum("cm,nctw->nmtw", np.abs(w[3]), np.abs(x))
    else:
        y += x
        mag += np.abs(x)
    return (np.maximum(y, 0.0) if relu else y), mag


def conv_operands(c, tier):
    rng = np.random.default_rng(np.random.SeedSequence([7, c.V, c.c_in, c.c_out, c.frames]))
    return dict(x=_draw(rng, tier, (c.n_seg, c.c_in, c.frames, c.V), -3, 3), w=_draw(rng, tier, (1, c.c_in, c.c_out), -3, 3),
                bias=_draw(rng, tier, (c.c_out,), -8, 8))


def conv_reference(c, ops):
    """csk_conv1x1_f32: y = W x + bias, no adjacency, no residual, no ReLU -> (y fp64, sum |term|)"""
    x, w, b = f64(ops["x"]), f64(ops["w"][0]), f64(ops["bias"])
    return (np.einsum("cm,nctw->nmtw", w, x) + b[None, :, None, None],
            np.einsum("cm,nctw->nmtw", np.abs(w), np.abs(x)) + np.abs(b)[None, :, None, None])


# ---- admissibility and the bound ------------------------------------------------------------------------------------------------
def is_integral_f32(a):
    a = np.asarray(a)
    return bool(np.all(a == np.round(a)) and np.all(a.astype(f32).astype(f64) == a.astype(f64)))


def admissible_exact(c, ops, y_pre, mag, relu=True):
    """exact tier: integer operands, every partial sum below 2^24 (on sum |term|), ReLU clips 20 % .. 80 %"""
    for k in ("x", "w", "bias") + (("ell_val",) if "ell_val" in ops else ()):
        a = np.asarray(ops[k])
        assert is_integral_f32(a[~np.isnan(a)] if k == "ell_val" else a), (c.name, k)      # NaN: the tails past ell_cnt alone
    if "ell_val_full" in ops:
        assert is_integral_f32(ops["ell_val_full"]) and all(np.isnan(ops["ell_val"][0, r, :, c.ell_cnt[r]:]).all() and
                                                            not np.isnan(ops["ell_val"][0, r, :, :c.ell_cnt[r]]).any() for r in range(3)), c.name
    assert float(mag.max()) < 2 ** 24, (c.name, float(mag.max()))
    if relu:
        share = float((y_pre < 0).mean())
        assert 0.2 <= share <= 0.8, (c.name, share)


def depth(c):
    if isinstance(c, Conv):
        return cpad(c.c_in) + 3
    return c.V + (4 if c.res == RES_CONV else 3) * cpad(c.c_in) + 4


def bound(c, mag):
    """depth * 2^-24 * sum |term|, per output (module docstring)"""
    return depth(c) * U * f64(mag)


def smallest_term(c, ops):
    """the smallest single term of any output of a float-tier case: a product W x adj, a residual term, the bias"""
    x, w, b = (float(np.abs(ops[k]).min()) for k in ("x", "w", "bias"))
    if isinstance(c, Conv):
        return min(w * x, b)
    a = float(np.abs(ops["adj"]).min())
    return min(w * x * a, b, w * x if c.res == RES_CONV else x)


def margin(c, ops, mag):
    """-> (bound, smallest term): a float-tier case is admissible when bound < smallest term / 2"""
    return float(bound(c, mag).max()), smallest_term(c, ops)


# ---- a plain fp32 model with seeded defects -----------------------------------------------------------------------------------
DEFECTS = ("transposed", "next_subset", "next_matrix", "lost_product", "tile_last_frame")


def model_f32(c, ops, defect=None, tile_frames=None):
    """The stage in plain fp32 (aggregation first, then the channel mix, bias, residual, ReLU) with ONE defect:
    transposed       adj[m, r, w, v] read for adj[m, r, v, w]
    next_subset      subset r + 1 (mod 3) read for r
    next_matrix      the neighbouring segment's / frame's matrix (index + 1, the last one wraps)
    lost_product     one product x adj dropped from the aggregation of one output column
    tile_last_frame  the last frame of every tile of `tile_frames` frames aggregates nothing"""
    x, w, b = ops["x"], ops["w"], ops["bias"]
    adj = np.asarray(ops["adj"], dtype=f32)
    if defect == "transposed":
        adj = np.swapaxes(adj, 2, 3)
    if defect == "next_subset":
        adj = np.roll(adj, -1, axis=1)
    if defect == "next_matrix":
        assert adj.shape[0] > 1
        adj = np.roll(adj, -1, axis=0)
    a = np.array(_adj_nt(c, adj, f32))
    agg = np.einsum("nctv,ntrvw->nrctw", x, a).astype(f32)
    if defect == "lost_product":
        prod = x[0, 0, 0, :, None] * a[0, 0, 1]                   # [v, w] of (segment 0, subset 1, channel 0, frame 0)
        v, wj = np.unravel_index(np.argmax(np.abs(prod)), prod.shape)
        assert prod[v, wj] != 0 and np.abs(w[1, 0]).max() > 0
        agg[0, 1, 0, 0, wj] -= prod[v, wj]
    if defect == "tile_last_frame":
        agg[:, :, :, tile_frames - 1:: tile_frames] = 0
    y = np.einsum("rcm,nrctw->nmtw", w[:3], agg).astype(f32) + b[None, :, None, None]
    y = y + (np.einsum("cm,nctw->nmtw", w[3], x).astype(f32) if c.res == RES_CONV else x)
    return np.maximum(y, 0).astype(f32)
