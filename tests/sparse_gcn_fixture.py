"""Cases, tile geometry, bound and seeded-defect model for the graph conv on a skeleton-SPARSE shared adjacency, at kernel level:
gcn_stage_sparse2_kernel<MT, CONVRES, 8> of csrc/gcn.hip (csk_gcn_stage_f32), its SPLIT form and gcn_reduce_kernel
(csk_gcn_stage_splitk_f32).  Shared by tests/test_gpu_sparse_gcn.py and tests/test_sparse_gcn_fixture_cpu.py.  Case, operands (adj =
"ell": lists of ell_w entries per column of which ell_cnt[r] count, the rest NaN), packing, layout, the fp64 reference and the
admissibility checks are those of tests/dense_gcn_fixture.py; there is no second reference.

What the tables are built to reach was read off the kernel and is PROVEN on the CPU (test_sparse_gcn_fixture_cpu.py) from the
definitions restated here -- tiles(), staging form, span, chunks -- and through the host queries csk_gcn_stage_f32_route /
csk_gcn_stage_splitk_f32_route, the functions the launcher switches on:

position tiles   NT = 16384 / MT positions (256 at MT 64, 128 at MT 128), NOT frame aligned: a tile stages the whole frames ta .. tb it
                 touches, span = (tb - ta + 1) V positions per channel row.  Q = frames V around one tile: 255 / 256 / 258 at MT 64 and
                 126 / 128 / 129 at MT 128 (127 and 257 are primes above 64: no frames x V gives them), a single ragged tile with
                 Q < 64, one frame, last tiles of 1, 2 and 3 positions, and runs long enough for the tile that starts at the frame
                 offset with the widest span (12 frames = 300 positions at V = 25 / MT 64, tile 4 of 52 frames; 7 frames at MT 128,
                 tile 8 of 47 frames; 16 / 8 frames at V = 18).  ldb reaches both staging limits: 320 (V = 40 and 64, MT 64) and 160
                 of 192 (V = 32, MT 128).  V = 18, 25 and the odd 17 / 19 / 21 / 37 / 43 / 51.
staging forms    16-byte vectors where ta V + 4 ceil(span / 4) <= Q and c_in >= 8 (with span % 4 != 0 it reads up to three positions
                 of the next frame), element-wise otherwise (the last tile of a segment, c_in = 3); both inside multi-chunk K loops,
                 the vector form also with x one float off 16-byte alignment and with an odd channel stride.
K loop           c_in 3, 8, 16, 17, 40, 64, 128, 256: 17 and 40 leave clamped padding rows under zero packed weights, 40 and more
                 run four or more 8-channel chunks (the steady state of the two-ahead prefetch).
epilogue         full (m0 + MT <= c_out) and ragged row tiles: c_out 40, 64, 100, 128, 130 (three 64-row tiles, the last ragged),
                 192, 256 (two 128-row tiles); identity and conv residual; y_pad 0 / 1 / 3, seg_pad 0 / 4, n_seg 1 / 2 / 3 / 5 (grids
                 that are no multiple of the 8 XCDs).  NOT covered: the slow epilogue addressing (fast_epi == 0) needs channel strides of
                 2^27 floats or more -- half a GiB per channel row.
adjacency        ell_cnt (1,1,4), (1,1,3), (1,0,4), (0,1,2), (0,0,0), (1,1,1) at ell_w = 1; ell_w = 5 with NaN tails; sources random,
                 not symmetric, different per subset and column, duplicates allowed.
split-K          cper = round_up(ceil(c_in_pad / ksplit), 8) channels per range, ranges = ceil(c_in / cper): single-chunk ranges (256
                 channels, ksplit 32), a short last range (128, ksplit 6: 5 x 24 + 8), fewer ranges than asked (40, ksplit 4: three),
                 ragged c_out 70, and a request that collapses to one range (c_in 3, ksplit 4: the unsplit kernel, no reduction); both
                 tile heights, both residuals, V 18 and 25, odd y_pad (the partial rows use y_chan_stride).

exact tier   as in dense_gcn_fixture: integer operands, any order of summation gives the same bits; a split launch therefore equals
             its unsplit twin bit for bit as well.
float tier   operands in [0.5, 1.5).  The depth of THIS kernel: the aggregation of a subset is one multiply and at most three fused
             multiply-adds (4 roundings, whatever V is), the channel mix accumulates R c_in_pad products, bias and residual are two
             more additions, the reduction of a split launch adds one partial sum per range, + 2 for the second-order terms:
                 depth = 4 + R c_in_pad + 2 + ranges + 2        (ranges = 0 for an unsplit launch)
             and |y - fp64| <= depth 2^-24 sum |term|.  Derived, not measured; below half of the smallest term for c_in <= 40.
numpy only; nothing is read from csrc."""
import ctypes
from collections import namedtuple

import numpy as np

from tests import dense_gcn_fixture as dx
from tests.dense_gcn_fixture import RES_CONV, RES_IDENTITY, SPARSE2, UNIT, f32, f64

KCG = 8                                    # channels per K chunk of gcn_stage_sparse2_kernel<.., .., 8>
SPLIT_BIT, SPLIT_MT128, SPLIT_CONVRES, SPLIT_RANGES_SHIFT = 1 << 30, 1 << 29, 1 << 28, 23      # csk_gcn_stage_splitk_f32_route


def sparse_route(c):
    return SPARSE2 * UNIT + dx.tile_rows(c.c_out) * 10 + (c.res == RES_CONV)


def sp(V, frames, c_in, c_out, res, n_seg, cnt=(1, 1, 4), ell_w=5, **kw):
    name = (f"V{V}-T{frames}-ci{c_in}-co{c_out}-{'id' if res == RES_IDENTITY else 'conv'}-n{n_seg}-cnt{''.join(map(str, cnt))}w{ell_w}"
            + "".join(f"-{k}{v}" for k, v in sorted(kw.items())))
    c = dx.case(name, V, c_in, c_out, frames, n_seg, res, "ell", None, ell_w=ell_w, ell_cnt=cnt, **kw)
    return c._replace(route=sparse_route(c))


I, C = RES_IDENTITY, RES_CONV
UNSPLIT_CASES = [
    # ---- <64, false>: identity residual, 64-row tiles of 256 positions
    sp(17, 15, 64, 64, I, 2),                                              # Q = 255
    sp(32, 8, 64, 64, I, 1, (1, 1, 3), 4),                                 # Q = 256
    sp(43, 6, 64, 64, I, 3, ell_w=4, x_pad=1, y_pad=1),                    # Q = 258: a last tile of 2 positions
    sp(19, 27, 64, 64, I, 2, (1, 0, 4), x_off=1, y_pad=3, seg_pad=4),      # Q = 513: a last tile of 1 position
    sp(25, 52, 64, 64, I, 2, x_pad=3),                                     # tile 4 spans 12 frames
    sp(18, 72, 64, 64, I, 1, (1, 1, 3), 3),                                # tile 4 spans 16 frames
    sp(40, 20, 40, 40, I, 5, (0, 1, 2), 4, seg_pad=4),                     # ldb = 320, tile 2 spans all of it; ragged rows
    sp(25, 2, 192, 192, I, 3, (0, 0, 0), 1),                               # Q = 50: one ragged tile; three 64-row tiles
    sp(25, 1, 64, 64, I, 2, (1, 1, 1), 1),                                 # one frame
    sp(18, 3, 64, 64, I, 2, ell_w=4, y_pad=1),
    # ---- <64, true>: conv residual
    sp(25, 52, 8, 64, C, 2, x_off=1),
    sp(18, 72, 40, 130, C, 1, (1, 1, 3), x_pad=1, y_pad=1),                # three row tiles, the last ragged
    sp(37, 7, 17, 40, C, 3, ell_w=4, y_pad=3, seg_pad=4),                  # Q = 259: a last tile of 3 positions
    sp(25, 11, 3, 64, C, 2),                                               # c_in = 3: element-wise staging in every tile
    sp(21, 13, 16, 192, C, 2, (1, 0, 4)),
    sp(25, 4, 256, 64, C, 1, ell_w=4),                                     # 32 chunks
    sp(18, 1, 128, 40, C, 5, (0, 0, 0), 1),
    sp(51, 5, 17, 64, C, 1, (1, 1, 1), 1),                                 # Q = 255
    sp(64, 9, 16, 64, C, 1, (0, 1, 2), x_pad=1),                           # ldb = 320 again
    # ---- <128, false>: identity residual, 128-row tiles of 128 positions
    sp(18, 7, 128, 128, I, 2, (1, 1, 3), 3),                               # Q = 126
    sp(32, 4, 128, 128, I, 3, y_pad=1),                                    # Q = 128; ldb = 160
    sp(43, 3, 128, 128, I, 1, ell_w=4, x_pad=1),                           # Q = 129: a last tile of 1 position
    sp(25, 47, 128, 128, I, 2, x_off=1, seg_pad=4),                        # tile 8 spans 7 frames
    sp(26, 5, 256, 256, I, 2, (1, 0, 4), 4, y_pad=3),                      # Q = 130: a last tile of 2 positions; two row tiles
    sp(25, 2, 256, 256, I, 1, (0, 1, 2)),
    sp(18, 1, 128, 128, I, 5, (1, 1, 1), 1),
    sp(18, 40, 128, 128, I, 1, (1, 1, 3), x_pad=3),
    # ---- <128, true>
    sp(25, 47, 40, 128, C, 1, ell_w=4, x_pad=1, y_pad=1),
    sp(37, 7, 17, 100, C, 2, seg_pad=4),                                   # Q = 259: a last tile of 3 positions; ragged rows
    sp(32, 9, 8, 256, C, 3, (1, 1, 3), 4),
    sp(25, 6, 3, 128, C, 2, y_pad=3),
    sp(19, 27, 16, 100, C, 1, (0, 1, 2), x_off=1),
    sp(25, 1, 64, 128, C, 2, (0, 0, 0), 1),
    sp(18, 3, 128, 256, C, 1, (1, 1, 1), 1),
    sp(18, 40, 64, 128, C, 2, (1, 0, 4)),
]

# a split launch: the case (its route is the unsplit twin's), the ranges asked for
Split = namedtuple("Split", "c ksplit")
SPLIT_CASES = [
    Split(sp(25, 3, 256, 256, I, 2, y_pad=1), 32),                         # <128, false>: 32 single-chunk ranges
    Split(sp(18, 9, 128, 128, I, 1, (1, 1, 3), 4, y_pad=3), 6),            # <128, false>: 5 x 24 + 8
    Split(sp(25, 11, 64, 64, I, 3), 4),                                    # <64, false>: 4 x 16
    Split(sp(25, 21, 64, 64, I, 1, x_off=1), 8),                           # <64, false>: 8 single-chunk ranges, three position tiles
    Split(sp(18, 15, 40, 40, I, 1, (1, 0, 4), seg_pad=4), 4),              # <64, false>: three ranges, ragged rows
    Split(sp(25, 11, 40, 70, C, 2, ell_w=4, y_pad=1), 4),                  # <128, true>: three ranges, ragged c_out 70
    Split(sp(25, 6, 17, 128, C, 3, (0, 1, 2)), 3),                         # <128, true>: two ranges of 16, 15 of them padding rows
    Split(sp(18, 15, 128, 64, C, 2, (1, 1, 3), x_pad=1, y_pad=1), 6),      # <64, true>: 5 x 24 + 8
    Split(sp(18, 4, 256, 130, C, 1, ell_w=4), 32),                         # <64, true>: 32 single-chunk ranges, three row tiles
    Split(sp(25, 6, 3, 64, C, 2, y_pad=1), 4),                             # collapses to one range: the unsplit kernel
]

# float tier: one case per instantiation, four unsplit, four split and the collapsed request.  c_in <= 40 keeps the bound far below
# half a term; <128, false> alone cannot have that (an identity residual on 128-row tiles means c_in = c_out >= 65) and runs at 72
# channels, where the CPU test shows the margin to hold all the same
FLOAT_CASES = [sp(25, 11, 40, 40, I, 2, x_pad=1), sp(18, 15, 17, 64, C, 2, (1, 1, 3), y_pad=1),
               sp(25, 6, 72, 72, I, 2, seg_pad=4), sp(25, 11, 40, 100, C, 2, ell_w=4)]
FLOAT_SPLITS = [Split(sp(25, 11, 40, 40, I, 2, y_pad=1), 4), Split(sp(18, 15, 24, 64, C, 2, (1, 1, 3)), 3),
                Split(sp(18, 9, 72, 72, I, 2, (1, 1, 3), 4), 3), Split(sp(25, 6, 40, 100, C, 2, y_pad=3), 5),
                Split(sp(25, 6, 3, 64, C, 2, y_pad=1), 4)]
FLOAT_MAX_C_IN = {sparse_route(FLOAT_CASES[2]): 72}          # per unsplit route; every other one: 40


# ---- geometry, from the definitions -----------------------------------------------------------------------------------------------
def cper_ranges(c_in, ksplit):
    """(channels per range, ranges that hold a channel) of a request for ksplit ranges"""
    cper = -(-(-(-dx.cpad(c_in) // ksplit)) // KCG) * KCG
    return cper, (-(-c_in // cper) if ksplit > 1 else 1)


def split_route(c, ksplit):
    """what csk_gcn_stage_splitk_f32_route must say"""
    cper, ranges = cper_ranges(c.c_in, ksplit)
    if ranges == 1:
        return sparse_route(c)
    return (SPLIT_BIT | (SPLIT_MT128 if dx.tile_rows(c.c_out) == 128 else 0) | (SPLIT_CONVRES if c.res == RES_CONV else 0)
            | (ranges - 1) << SPLIT_RANGES_SHIFT | cper // 8)


def split_query(lib, c, ksplit, x=dx.ALIGNED, y=dx.ALIGNED, ell=dx.ALIGNED, partial=dx.ALIGNED):
    if x == dx.ALIGNED:
        x += 4 * c.x_off
    cnt = (ctypes.c_int32 * 3)(*c.ell_cnt)
    xc, xs, yc, ys = dx.strides(c)
    return lib.csk_gcn_stage_splitk_f32_route(x, y, ell, ctypes.cast(cnt, ctypes.c_void_p), c.ell_w, c.n_seg, c.c_in, c.c_out, c.frames, c.V,
                                              xs, xc, ys, yc, c.res, ksplit, partial)


def chunks_of_ranges(c, ksplit):
    """8-channel chunks each range walks: the last one gets what is left of c_in_pad"""
    cper, ranges = cper_ranges(c.c_in, ksplit)
    return [min(dx.cpad(c.c_in) - k * cper, cper) // KCG for k in range(ranges)]


def ldb(V, mt):
    nt = 16384 // mt
    return -(-(((nt + V - 2) // V + 1) * V) // 4) * 4


Tile = namedtuple("Tile", "q0 qend ta tb span vec")


def tiles(c):
    """the position tiles of one segment: first / last frame touched, staged span, 16-byte staging form or not"""
    nt, Q = 16384 // dx.tile_rows(c.c_out), c.frames * c.V
    out = []
    for q0 in range(0, Q, nt):
        qend = min(q0 + nt, Q)
        ta, tb = q0 // c.V, (qend - 1) // c.V
        span = (tb - ta + 1) * c.V
        out.append(Tile(q0, qend, ta, tb, span, ta * c.V + 4 * -(-span // 4) <= Q and c.c_in >= KCG))
    return out


def max_span(V, mt):
    """the widest span a full tile of the (V, MT) class can have, over every frame offset a tile start k NT can fall on"""
    nt = 16384 // mt
    return max(((k * nt % V + nt - 1) // V + 1) * V for k in range(V))


def workgroups(c, ksplit=1):
    mt = dx.tile_rows(c.c_out)
    return len(tiles(c)) * (dx.mpad(c.c_out) // mt) * c.n_seg * cper_ranges(c.c_in, ksplit)[1]


def row_tiles(c):
    """(full, ragged) row tiles of the epilogue"""
    mt = dx.tile_rows(c.c_out)
    full = sum(m0 + mt <= c.c_out for m0 in range(0, dx.mpad(c.c_out), mt))
    return full, dx.mpad(c.c_out) // mt - full


# ---- the bound ------------------------------------------------------------------------------------------------------------------------
def depth(c, ksplit=1):
    ranges = cper_ranges(c.c_in, ksplit)[1]
    return 4 + (4 if c.res == RES_CONV else 3) * dx.cpad(c.c_in) + 2 + (ranges if ranges > 1 else 0) + 2


def bound(c, mag, ksplit=1):
    return depth(c, ksplit) * dx.U * f64(mag)


def smallest_term(c, ops):
    """the smallest single term of any output of a float-tier case: W x times an entry that counts, a residual term, the bias"""
    x, w, b = (float(np.abs(ops[k]).min()) for k in ("x", "w", "bias"))
    val = ops["ell_val"]
    a = min([float(np.abs(val[0, r, :, :c.ell_cnt[r]]).min()) for r in range(3) if c.ell_cnt[r]] or [np.inf])
    return min(w * x * a, b, w * x if c.res == RES_CONV else x)


def margin(c, ops, mag, ksplit=1):
    return float(bound(c, mag, ksplit).max()), smallest_term(c, ops)


# ---- a plain fp32 model with seeded defects ---------------------------------------------------------------------------------------------
DEFECTS = ("past_cnt", "seam_first", "seam_last", "next_subset", "lost_product", "pad_duplicate", "split_dropped", "res_row4", "tail_unwritten")


def applies(defect, c, ksplit=1):
    if defect == "past_cnt":
        return any(n < c.ell_w for n in c.ell_cnt)
    if defect in ("seam_first", "seam_last"):
        return any(t.q0 % c.V for t in tiles(c)) and sum(c.ell_cnt) > 0
    if defect in ("next_subset", "lost_product"):
        return c.ell_cnt[1] > 0
    if defect == "pad_duplicate":
        return c.c_in % dx.CPAD != 0
    if defect == "split_dropped":
        return cper_ranges(c.c_in, ksplit)[1] > 1
    if defect == "res_row4":
        return c.res == RES_IDENTITY
    return True


def model_f32(c, ops, defect=None, ksplit=1):
    """The stage in plain fp32 (the aggregation of every subset first, then the channel mix range by range, bias, residual, ReLU)
    with ONE defect:
    past_cnt        the entry e = ell_cnt[r] of every column of one subset counted (its drawn value, not the NaN put there)
    seam_first      at a tile seam inside a frame, the tile's first (partial) frame aggregates from the NEXT frame
    seam_last       ... the previous tile's last (partial) frame aggregates from the frame BEFORE
    next_subset     subset r + 1 (mod 3) read for r
    lost_product    one product val x dropped from one aggregated value
    pad_duplicate   every padding channel contributes the last real channel's row once more
    split_dropped   one channel range of a split launch contributes nothing
    res_row4        the identity residual taken from row + 4
    tail_unwritten  the last 1 .. 3 positions of every segment not written (they keep the NaN the output starts with)"""
    x, w, b = ops["x"], ops["w"], ops["bias"]
    adj = np.asarray(ops["adj"], dtype=f32).copy()                         # [1, 3, V(v), V(w)]
    if defect == "past_cnt":
        r = next(r for r in (2, 1, 0) if c.ell_cnt[r] < c.ell_w)
        e = c.ell_cnt[r]
        for wj in range(c.V):
            adj[0, r, ops["ell_src"][r, wj, e], wj] += ops["ell_val_full"][0, r, wj, e]
    if defect == "next_subset":
        adj = np.roll(adj, -1, axis=1)
    agg = np.einsum("nctv,rvw->nrctw", x, adj[0]).astype(f32)
    if defect in ("seam_first", "seam_last"):
        t = next(t for t in tiles(c) if t.q0 % c.V)
        fr, wj = divmod(t.q0, c.V)                                         # the frame the seam cuts: columns wj .. of it open the tile
        other = np.einsum("ncv,rvw->nrcw", x[:, :, (fr + 1) % c.frames if defect == "seam_first" else fr - 1], adj[0]).astype(f32)
        assert c.frames > 1
        if defect == "seam_first":
            agg[:, :, :, fr, wj:] = other[..., wj:]
        else:
            agg[:, :, :, fr, :wj] = other[..., :wj]
    if defect == "lost_product":
        prod = x[0, 0, 0, :, None] * adj[0, 1]                             # [v, w] of (segment 0, subset 1, channel 0, frame 0)
        v, wj = np.unravel_index(np.argmax(np.abs(prod)), prod.shape)
        assert prod[v, wj] != 0 and np.abs(w[1, 0]).max() > 0
        agg[0, 1, 0, 0, wj] -= prod[v, wj]
    R = 4 if c.res == RES_CONV else 3
    ops_r = np.concatenate([agg, x[:, None]], axis=1)[:, :R]               # the conv residual rides along as a fourth subset
    cper, ranges = cper_ranges(c.c_in, ksplit)
    y = np.zeros((c.n_seg, c.c_out, c.frames, c.V), dtype=f32)
    for k in range(ranges):
        if defect == "split_dropped" and k == ranges - 1:
            continue
        lo, hi = k * cper, min((k + 1) * cper, c.c_in)
        y = y + np.einsum("rcm,nrctw->nmtw", w[:R, lo:hi], ops_r[:, :, lo:hi]).astype(f32)
    if defect == "pad_duplicate":
        y = y + f32(dx.cpad(c.c_in) - c.c_in) * np.einsum("rm,nrtw->nmtw", w[:R, -1], ops_r[:, :, -1]).astype(f32)
    y = y + b[None, :, None, None]
    if c.res == RES_IDENTITY:
        y = y + (np.roll(x, -4, axis=1) if defect == "res_row4" else x)
    y = np.maximum(y, 0).astype(f32)
    if defect == "tail_unwritten":
        y.reshape(c.n_seg, c.c_out, -1)[:, :, -((c.frames * c.V - 1) % 3 + 1):] = np.nan
    return y
