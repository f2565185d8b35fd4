"""Exact-arithmetic cases for the slot-balanced 16x16x4 tile family of csrc/step16.hip: the temporal step (csk_tcn_step_f32 ->
tcn_step16_kernel<NB, E, HS, TAIL>) and the graph conv on channel-major frames (csk_gcn_stage_f32 -> gcn16_kernel<NB, F, CONVRES, 8>).

Every operand is an integer-valued fp32 number -- weights in +-{1..4} (never 0), activations in {1..7}, bias and residual values
small integers, adjacency values in {1, 2, 3} with at most 1 / 1 / 4 non-zeros per column, no BatchNorm (scale exactly 1: the
images are packed with ``fold.pack_conv_weight(w, ones)``, ``fold.pad_vec`` and ``fold.ell_from_dense``) -- and for every
output  sum |w| |x| + |bias| + |res| < 2**24.  Every partial sum of such an output, in ANY order and with or without fused
multiply-adds, is then an integer below 2**24 and exact in fp32: the kernel must reproduce the fp64 reference
(``torch.nn.functional.conv2d`` / ``einsum`` on doubles) bit for bit, tolerance 0.  A lost, duplicated or misrouted product, a
wrong ring slot, a wrong residual frame, a skipped bias or a column that landed in the wrong emission changes an integer and
cannot hide in rounding.  ``admissible`` asserts both conditions; no error bound is introduced anywhere.

Which instantiation a launch runs is host arithmetic: ``step_tile`` / ``gcn_tile`` ask the library (csk_tcn_step_f32_tile,
csk_gcn_stage_f32_tile; no GPU).  The small cases run NB = 18 (at most 256 tiles: 16 x 18 columns cost less than 16 x 25); the
NB = 25 temporal instantiations need more than 256 narrow tiles, so ``WIDE`` repeats a P = 100 case along the position axis up to
the smallest P at which the query answers 25 (positions are independent: the reference is the small case's, repeated).

Layouts, ring rotation and slot arguments are those of tests/step_split_fixture.py (``channel_major``, ``ring_of``,
``launch_geometry``): ring slots that hold no frame are NaN, positions between N V and P are NaN, the output ring has one spare slot.
CPU only: nothing here touches a device."""
import ctypes
from dataclasses import dataclass, replace

import torch
import torch.nn.functional as F

import _bootstrap
from tests import step_split_fixture as ssf

pkg = _bootstrap.load()
from continual_skeletons_amd import fold  # noqa: E402

RES_MODE = {"none": 0, "ident": 1, "conv": 2}
EXACT = float(2 ** 24)


def _ints(g, shape, lo, hi):
    """integers lo .. hi (inclusive) as fp32"""
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _weights(g, shape):
    """+-{1..4}, never 0; three in four positive, so that most outputs survive a ReLU"""
    sign = torch.where(torch.rand(shape, generator=g) < 0.75, 1.0, -1.0)
    return _ints(g, shape, 1, 4) * sign


# ---- temporal step ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class StepCase:
    c: int                      # channels of the post-GCN ring
    co: int
    V: int
    N: int
    head_step: int              # 1, or 2: a stride-2 block (emission j reads ring slots 2 j .. 2 j + 8)
    n_emit: int
    res: str                    # "none" | "ident" | "conv"
    c_res: int
    wrap: bool                  # the window of the first emission wraps the end of the ring; the residual and output rings wrap
    relu: bool
    seed: int

    @property
    def id(self):
        return (f"c{self.c}-o{self.co}-hs{self.head_step}-e{self.n_emit}-{self.res}{self.c_res or ''}-v{self.V}n{self.N}"
                f"{'-wrap' if self.wrap else ''}{'-relu' if self.relu else ''}")

    # what step_split_fixture.launch_geometry reads of a case
    @property
    def case(self):
        return self

    @property
    def stride(self):
        return self.head_step

    @property
    def T(self):                # frames in the ring: exactly n_emit full 9-frame windows
        return self.head_step * (self.n_emit - 1) + 9

    @property
    def t_lo(self):             # clip output of emission 0 (its window is frames 0 .. 8)
        return -(-4 // self.head_step)

    @property
    def P(self):
        return (self.N * self.V + 3) // 4 * 4

    @property
    def res_frames(self):       # residual frame of emission j: the centre of its window
        return [self.head_step * (self.t_lo + j) for j in range(self.n_emit)]


@dataclass
class StepOps:
    x: torch.Tensor             # (N, c, T, V)
    w: torch.Tensor             # (co, c, 9, 1)
    bias: torch.Tensor          # (co,)
    x_res: torch.Tensor         # (N, c_res, T, V) or None
    w_res: torch.Tensor         # (co, c_res, 1, 1) or None


def step_ops(sc, real=False):
    """the case's operands: integers (the exact cases), or -- ``real`` -- torch.rand activations with fan-in scaled normal
    weights and small biases (the launch-size invariance test: no reference, two launches compared with each other)"""
    g = torch.Generator().manual_seed(1000 + sc.seed)
    shape_x, shape_w = (sc.N, sc.c, sc.T, sc.V), (sc.co, sc.c, 9, 1)
    shape_xr, shape_wr = (sc.N, sc.c_res, sc.T, sc.V), (sc.co, sc.c_res, 1, 1)
    if real:
        return StepOps(torch.rand(shape_x, generator=g), torch.randn(shape_w, generator=g) * (1.0 / (9 * sc.c)) ** 0.5,
                       torch.rand(sc.co, generator=g) * 0.2 - 0.1, None if sc.res == "none" else torch.rand(shape_xr, generator=g),
                       torch.randn(shape_wr, generator=g) * (1.0 / sc.c_res) ** 0.5 if sc.res == "conv" else None)
    return StepOps(_ints(g, shape_x, 1, 7), _weights(g, shape_w), _ints(g, (sc.co,), -8, 8),
                   None if sc.res == "none" else _ints(g, shape_xr, 1, 7), _weights(g, shape_wr) if sc.res == "conv" else None)


def _step_sum(sc, x, w, bias, x_res, w_res):
    y = F.conv2d(x, w, stride=(sc.head_step, 1)) + bias[None, :, None, None]       # no padding: output j is the window 2 j .. 2 j + 8
    assert y.shape[2] == sc.n_emit
    if sc.res == "ident":
        y = y + x_res[:, :, sc.res_frames]
    elif sc.res == "conv":
        y = y + F.conv2d(x_res[:, :, sc.res_frames], w_res)
    return y


def step_reference(sc, ops):
    """-> (N, co, n_emit, V) fp64: the emitting steps on doubles"""
    d = [None if t is None else t.double() for t in (ops.x, ops.w, ops.bias, ops.x_res, ops.w_res)]
    y = _step_sum(sc, *d)
    return torch.relu(y) if sc.relu else y


def step_admissible(sc, ops):
    """the whole admissibility condition: integer operands, and sum |w| |x| + |bias| + |res| < 2**24 for every output"""
    for t in (ops.x, ops.w, ops.bias, ops.x_res, ops.w_res):
        assert t is None or (t.dtype == torch.float32 and torch.equal(t, t.round()))
    assert bool((ops.w != 0).all()) and (ops.w_res is None or bool((ops.w_res != 0).all()))
    bound = _step_sum(sc, *[None if t is None else t.double().abs() for t in (ops.x, ops.w, ops.bias, ops.x_res, ops.w_res)])
    assert float(bound.max()) < EXACT
    return float(bound.max())


def step_launch(sc, ops, wide_P=None):
    """host tensors and scalar arguments of the csk_tcn_step_f32 launch.  ``wide_P``: the case's positions (P == N V) repeated along
    the position axis up to wide_P positions -- position p of the wide launch is position p % P of the case"""
    P = sc.P
    g = ssf.launch_geometry(sc)
    idx = None
    if wide_P is not None:
        assert P == sc.N * sc.V and wide_P % 4 == 0
        idx = torch.arange(wide_P) % P

    def wide(t):
        return t if idx is None else t[..., idx].contiguous()

    one = torch.ones(sc.co, dtype=torch.float64)
    ring = wide(ssf.ring_of(ssf.channel_major(ops.x, P), g["slots"], g["rot"]))
    xres = None if ops.x_res is None else wide(ssf.ring_of(ssf.channel_major(ops.x_res, P), g["x_slots"], g["x_rot"]))
    t = dict(ring=ring, w=fold.pack_conv_weight(ops.w, one), xres=xres,
             wres=None if ops.w_res is None else fold.pack_conv_weight(ops.w_res, one), bias=fold.pad_vec(ops.bias))
    return t, dict(g, P=wide_P or P)


def step_handed_integers(sc, ops):
    """every operand handed to the kernel equals its own .round() (NaN marks slots and positions that hold nothing)"""
    t, _ = step_launch(sc, ops)
    for v in t.values():
        if v is not None:
            real = v[~torch.isnan(v)]
            assert torch.equal(real, real.round())
    assert float(t["w"].abs().sum()) == float(ops.w.abs().sum())                # the image holds the weights and zeros


def _cycle(seq, i):
    return seq[i % len(seq)]


def build_step_cases():
    """The (head_step, n_emit) forms -- E = 4: (1, 4 | 8); E = 2: (1, 2 | 6); E = 2, HS = 2: (2, 2 | 4); E = 1: (1 | 2, 1 | 3), the larger
    n_emit with more than one emission group (j0 = bz E) -- crossed with the channel counts: 16, 32 (no padding rows), 4, 6, 12, 24
    (TAIL: a partial chunk, a chunk of padding only) and 16 with a conv residual of 3 or 24 channels (TAIL by the residual alone).
    Residual mode, wrap, positions (100, 72: one partial tile; 428: several tiles, the last one partial), c_out (64, 256: one and
    four m-tiles) and ReLU rotate over the list."""
    cs, i = [], 0
    forms = ((1, 4), (1, 8), (1, 2), (1, 6), (2, 2), (2, 4), (1, 1), (1, 3), (2, 1), (2, 3))
    chans = ((16, None), (32, None), (4, None), (6, None), (12, None), (24, None), (16, 3), (16, 24))
    for fi, (hs, n_emit) in enumerate(forms):
        for ci, (c, tail_res) in enumerate(chans):
            k = fi + ci                                                       # walks every rotation against every form and count
            co = _cycle((64, 256), k // 2 + ci)
            V, N = _cycle(((25, 4), (18, 4), (25, 17)), k)
            if tail_res:
                res, c_res = "conv", tail_res
            else:
                res = _cycle(("none", "ident", "conv") if hs == 1 else ("none", "conv"), k)
                # (no padding rows in the residual either where the case is to stay on the fast instantiation)
                c_res = 0 if res == "none" else co if res == "ident" else _cycle((16, 32) if c % 16 == 0 else (3, 16, 24), k)
            cs.append(StepCase(c, co, V, N, hs, n_emit, res, c_res, wrap=(k + fi // 2) % 2 == 1, relu=i % 3 != 0, seed=i))
            i += 1
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), "duplicate case"
    return cs


STEP_CASES = build_step_cases()


@dataclass(frozen=True)
class WideCase:
    sc: StepCase                # P = 100 = N V: no padding positions

    @property
    def id(self):
        return f"{self.sc.id}-wide"


def build_wide():
    """one P = 100 case per NB = 25 instantiation (E, HS, TAIL), C_out = 256 (four m-tiles); between them every residual mode,
    both wrap flags and launches of more than one emission group"""
    w = []
    for i, (c, hs, n_emit, res, c_res, wrap) in enumerate((
            (16, 1, 8, "ident", 256, True),        # (4, 1, 0), two emission groups
            (12, 1, 4, "conv", 24, False),         # (4, 1, 1)
            (32, 1, 6, "none", 0, False),          # (2, 1, 0), three emission groups
            (16, 1, 2, "conv", 3, True),           # (2, 1, 1): TAIL by the residual alone
            (16, 2, 4, "conv", 16, True),          # (2, 2, 0), two emission groups
            (6, 2, 2, "none", 0, False),           # (2, 2, 1)
            (32, 1, 3, "none", 0, True),           # (1, 1, 0), three emission groups
            (24, 2, 3, "conv", 24, False))):       # (1, 1, 1), head_step 2
        w.append(WideCase(StepCase(c, 256, 25, 4, hs, n_emit, res, c_res, wrap, relu=i % 2 == 0, seed=500 + i)))
    return w


WIDE = build_wide()


def step_tile(sc, P=None, lib=None):
    """csk_tcn_step_f32_tile for the case's launch (at P positions): NB * 1000 + E * 100 + HS * 10 + TAIL"""
    lib = lib or pkg.native.lib()
    g = ssf.launch_geometry(sc)
    return lib.csk_tcn_step_f32_tile(g["slots"], sc.head_step, sc.n_emit, g["x_slots"] if sc.res != "none" else 0, g["out_slots"], sc.c,
                                     sc.co, sc.P if P is None else P, 9, RES_MODE[sc.res], sc.c_res, 1)


def tile_positions(tile):
    """positions of one emission in a tile of the instantiation"""
    return 16 * (tile // 1000) // (tile // 100 % 10)


_wide_P = {}


def wide_P(wc):
    """the smallest P (a multiple of 4, > 100) at which the launch of the case takes the NB = 25 tiles AND ends in a partial tile
    -- asked of the library, not written down"""
    if wc.id not in _wide_P:
        lib = pkg.native.lib()
        for P in range(104, 1 << 17, 4):
            t = step_tile(wc.sc, P, lib)
            if t // 1000 == 25 and P % tile_positions(t):
                _wide_P[wc.id] = P
                break
        else:
            raise AssertionError(f"{wc.id}: no launch below 2**17 positions takes the 25-block tiles")
    return _wide_P[wc.id]


def smallest_P25(wc):
    """the smallest P at which the query answers NB = 25 at all (reported; wide_P adds the partial last tile)"""
    lib = pkg.native.lib()
    return next(P for P in range(104, 1 << 17, 4) if step_tile(wc.sc, P, lib) // 1000 == 25)


# ---- graph conv ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GcnCase:
    ci: int
    co: int
    V: int
    n_seg: int                  # frames of a cycle = segments of the launch
    skel: int                   # skeletons per frame (the "frames" argument of csk_gcn_stage_f32 on channel-major frames)
    seed: int
    base_skel: int = 0          # > 0: skeleton s of the launch is skeleton s % base_skel of the case with base_skel skeletons

    @property
    def id(self):
        return f"g{self.ci}-{self.co}-v{self.V}-f{self.n_seg}-s{self.skel}"

    @property
    def res(self):
        return "ident" if self.ci == self.co else "conv"

    @property
    def P(self):
        return (self.skel * self.V + 3) // 4 * 4

    @property
    def base(self):
        return replace(self, skel=self.base_skel, base_skel=0) if self.base_skel else self


@dataclass
class GcnOps:
    x: torch.Tensor             # (n_seg, ci, skel, V)
    w: torch.Tensor             # (R, ci, co): the three subsets (+ the conv gcn_residual)
    bias: torch.Tensor          # (co,)
    A: torch.Tensor             # (3, V, V)


def adjacency(V):
    """an integer skeleton-sparse adjacency: subset 0 one entry per column (not the diagonal), subset 1 one entry in four columns of
    five, subset 2 zero to four entries per column; values 1, 2, 3"""
    A = torch.zeros((3, V, V))
    for w in range(V):
        A[0, (7 * w + 3) % V, w] = 1 + w % 3
        if w % 5:
            A[1, (w + V // 2) % V, w] = 1 + (w + 1) % 3
        for k in range(w % 5):
            A[2, (w + 1 + 3 * k) % V, w] = 1 + (w + k) % 3
    per_col = (A != 0).sum(1)
    assert [int(per_col[i].max()) for i in range(3)] == [1, 1, 4]
    return A


def gcn_ops(gc):
    """operands of the case with its OWN skeleton count (gc.base for a repeated case)"""
    assert not gc.base_skel
    g = torch.Generator().manual_seed(2000 + gc.seed)
    R = 3 if gc.res == "ident" else 4
    return GcnOps(_ints(g, (gc.n_seg, gc.ci, gc.skel, gc.V), 1, 7), _weights(g, (R, gc.ci, gc.co)), _ints(g, (gc.co,), -8, 8),
                  adjacency(gc.V))


def _gcn_sum(gc, x, w, bias, A):
    y = torch.einsum("rco,fcsv,rvw->fosw", w[:3], x, A) + bias[None, :, None, None]
    return y + (x if gc.res == "ident" else torch.einsum("co,fcsw->fosw", w[3], x))


def gcn_reference(gc, ops):
    """-> (n_seg, co, skel, V) fp64: ReLU(sum_r W_r . (x A_r) + bias + gcn_residual(x)) on doubles"""
    return torch.relu(_gcn_sum(gc, ops.x.double(), ops.w.double(), ops.bias.double(), ops.A.double()))


def gcn_admissible(gc, ops):
    for t in (ops.x, ops.w, ops.bias, ops.A):
        assert t.dtype == torch.float32 and torch.equal(t, t.round())
    assert bool((ops.w != 0).all()) and set(ops.A.unique().tolist()) <= {0.0, 1.0, 2.0, 3.0}
    bound = _gcn_sum(gc, ops.x.double(), ops.w.double().abs(), ops.bias.double().abs(), ops.A.double())
    assert float(bound.max()) < EXACT
    return float(bound.max())


def gcn_launch(gc, ops):
    """host tensors of the csk_gcn_stage_f32 launch on channel-major frames: x [n_seg][ci][P], position s V + v; positions past
    skel V are NaN.  ``ops`` are the operands of gc.base"""
    b = gc.base
    xs = ops.x if not gc.base_skel else ops.x[:, :, torch.arange(gc.skel) % b.skel]
    x = torch.full((gc.n_seg, gc.ci, gc.P), float("nan"))
    x[:, :, : gc.skel * gc.V] = xs.reshape(gc.n_seg, gc.ci, gc.skel * gc.V)
    R, cp, mp = ops.w.shape[0], fold._ceil_to(gc.ci, fold.KC), fold._ceil_to(gc.co, fold.MT)
    w = torch.zeros((R, cp, mp))
    w[:, : gc.ci, : gc.co] = ops.w
    src, val, cnt, ew = fold.ell_from_dense(ops.A)
    return dict(x=x, w=w, bias=fold.pad_vec(ops.bias), ell_src=src, ell_val=val, ell_cnt=cnt, ell_w=ew)


def gcn_handed_integers(gc, ops):
    t = gcn_launch(gc, ops)
    for name in ("x", "w", "bias", "ell_val"):
        real = t[name][~torch.isnan(t[name])]
        assert torch.equal(real, real.round())
    assert t["ell_cnt"].tolist() == [1, 1, 4] and t["ell_w"] == 4


def gcn_expand(gc, want):
    """reference of gc.base (n_seg, co, base_skel, V) -> the launch's: skeleton s is skeleton s % base_skel"""
    return want if not gc.base_skel else want[:, :, torch.arange(gc.skel) % gc.base_skel]


# V = 25 (NB 25) and V = 18 (NB 18) x F = 4, 2, 1 (n_seg 4 | 8, 2 | 6, 1 | 3: one and more segment groups) x identity (64 -> 64,
# 16 -> 16) and conv gcn_residual (3 -> 64, 12 -> 24, 128 -> 256); 7 and 3 skeletons leave a ragged last tile, 4 (V = 25, F = 4: 100
# positions) and 16 (F = 1: 400 / 288 positions) are a single whole tile.  The policy keeps the 32x32x2 kernel at these sizes.
GCN_CASES = [GcnCase(ci, co, V, n_seg, skel, seed=i) for i, (ci, co, V, n_seg, skel) in enumerate((
    (64, 64, 25, 4, 7), (64, 64, 25, 4, 4), (16, 16, 25, 2, 3), (64, 64, 25, 1, 16), (16, 16, 25, 6, 7),
    (3, 64, 25, 8, 7), (12, 24, 25, 6, 3), (128, 256, 25, 3, 7), (3, 64, 25, 1, 3), (12, 24, 25, 4, 4),
    (16, 16, 18, 8, 7), (64, 64, 18, 6, 3), (64, 64, 18, 3, 16), (16, 16, 18, 2, 7),
    (12, 24, 18, 4, 7), (3, 64, 18, 2, 3), (128, 256, 18, 1, 7), (3, 64, 18, 3, 3), (12, 24, 18, 8, 4)))]
# production sizes the policy itself hands to the family: 4 frames of 2048 skeletons (2047: a ragged last tile), 64 -> 64 and
# 3 -> 64, repeating a 7-skeleton case
GCN_PRODUCTION = [GcnCase(ci, 64, V, 4, skel, seed=100 + i, base_skel=7)
                  for i, (ci, V, skel) in enumerate((ci, V, skel) for V in (25, 18) for ci in (64, 3) for skel in (2048, 2047))]

ALIGNED = ctypes.c_void_p(1 << 12)       # a 16-byte aligned address for the queries (never dereferenced)


def gcn_tile(gc, lib=None, x=ALIGNED, y=ALIGNED):
    """csk_gcn_stage_f32_tile for the plain call on channel-major frames: 0 or NB * 1000 + F * 100 + CONVRES * 10"""
    lib = lib or pkg.native.lib()
    cnt = (ctypes.c_int32 * 3)(1, 1, 4)
    P = gc.P
    return lib.csk_gcn_stage_f32_tile(x, y, ctypes.cast(cnt, ctypes.c_void_p), 4, 0, 0, gc.n_seg, gc.ci, gc.co, gc.skel, gc.V, gc.ci * P, P,
                                      gc.co * P, P, RES_MODE[gc.res])
