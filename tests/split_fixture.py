"""Fixtures that pin the six piece products of the "bf16x3" kernels (csrc/split_core.h: hh, hm, mh, mm, hl, lh).

The mode splits every fp32 operand into three bf16 pieces h + m + l and accumulates six piece products in fp32.  A lost
second-order product (mm, hl, lh) moves a result by a few 1e-6 relative -- far below the suite's absolute 1e-4 and, on random
data, below the rounding noise of a long fp32 accumulation.  The fixtures here make such a loss visible:

* designed operands (``designed``): every element is built from its pieces, all positive -- h on the bf16 grid in [1, 1.25),
  m = 2^-9 (1 + j 2^-7) with j in 64..127, l = i 2^-23 with i in 32..63 -- so a lost product removes same-signed terms from
  every output (it cannot average out), and the three pieces of an element are known without running any split;
* sparse "hot" weights: non-zero in a few (tap slot, 16-channel chunk) pairs only, everything else exactly zero, so an output
  is the result of few fp32 accumulations and a fault confined to one slot, chunk, weight stage or ping-pong parity is not
  diluted by healthy ones.  Weights are scaled by a power of two (exact for every piece) to keep the outputs O(1).

Everything a test asserts against is computed from the fixture, never from the kernel (``analyse``):
  want    the fp64 product of the designed fp32 operands (``conv64``: the convolution sum written out as an einsum per tap)
  six     the fp64 sum of the six piece products the kernel is meant to form
  D       the smallest relative deviation, over all non-zero outputs, between ``six`` and ``six`` without one second-order
          product (minimum over mm, hl, lh); the tolerance of a case is D / 2, relative per output
  bound   a rounding-mode-agnostic worst case of the fp32 accumulation, (6 n_hot + 16) 2^-24 sum|terms| / |output|: 6
          accumulating MFMAs per hot pair, each at most one unit in the last place of the running sum (all terms positive: the
          running sum never exceeds the output), plus 16 units for the summation inside the matrix instruction and the
          epilogue.  A sparse case is admissible only if bound <= D / 2; that caps n_hot at 3.
``restate32`` is the same arithmetic in sequential fp32 (products of bf16 pieces are exact in fp32), in the kernel's order:
one 16-channel dot product per matrix instruction, added to the running sum.
"""
import json
import math
import os
from dataclasses import dataclass
from typing import Tuple

import torch
import torch.nn.functional as F

from tests.helpers import REF_CAP, _report_path

KS = 16                       # channels per chunk (csrc/split_core.h)
MT = 64                       # row padding of the operand images (CSK_MT)
K_TCN, PAD_TCN = 9, 4
UNIT = 2.0 ** -24
SIX = ((0, 2), (2, 0), (1, 1), (1, 0), (0, 1), (0, 0))      # (weight piece, activation piece) in the kernel's order: hl lh mm mh hm hh
SECOND = {"hl": (0, 2), "lh": (2, 0), "mm": (1, 1)}
MAX_HOT = 3


def designed(shape, seed):
    """-> (x fp32, (h, m, l) fp32) with x == h + m + l exactly and every piece bf16-exact (module docstring)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, 32, shape, generator=g).double()
    j = torch.randint(64, 128, shape, generator=g).double()
    i = torch.randint(32, 64, shape, generator=g).double()
    h = 1.0 + a * 2.0 ** -7
    m = 2.0 ** -9 * (1.0 + j * 2.0 ** -7)
    l = i * 2.0 ** -23
    x = h + m + l
    assert torch.equal(x.float().double(), x)
    return x.float(), (h.float(), m.float(), l.float())


def tap_order(stride, k=K_TCN):
    """tap of every slot of the class-major weight image: residue classes of the taps modulo the stride, side by side"""
    return sorted(range(k), key=lambda r: (r % stride, r)) if k > 1 else [0]


def n_chunks(c):
    return -(-c // KS)


def t_out_of(t_in, stride):
    return (t_in + 2 * PAD_TCN - K_TCN) // stride + 1


@dataclass(frozen=True)
class Case:
    """One launch.  ``hot``: the non-zero (slot, chunk) pairs of the main weights -- slot = tap slot of the class-major image
    (tcn) or adjacency subset (gcn); ``dense``: all of them.  ``res``: "none", "ident" or "conv"; ``res_hot``: the non-zero
    chunks of the 1 x 1 residual conv image.  ``c_res``: channels of the residual input of a tcn stage (the block input)."""
    kernel: str
    ci: int
    co: int
    V: int
    T: int
    N: int
    stride: int = 1
    hot: Tuple[Tuple[int, int], ...] = ()
    res: str = "none"
    res_hot: Tuple[int, ...] = ()
    c_res: int = 0
    dense: bool = False

    @property
    def id(self):
        hot = "dense" if self.dense else "+".join(f"s{s}c{c}" for s, c in self.hot) or "zero"
        res = "" if self.res == "none" else "-" + self.res + ("".join(f"c{c}" for c in self.res_hot))
        cres = f"r{self.c_res}" if self.kernel == "tcn" and self.res == "conv" else ""
        return f"{self.kernel}-{self.ci}{cres}to{self.co}-s{self.stride}-V{self.V}T{self.T}N{self.N}-{hot}{res}"

    @property
    def template(self):
        """row-tile template of the launch: 128 when the padded row count is a multiple of 128 (tcn_split.hip), else 64"""
        return 128 if (-(-self.co // MT) * MT) % 128 == 0 else 64

    @property
    def n_hot(self):
        """accumulation phases an output goes through: hot main pairs, hot residual chunks, the identity add"""
        return len(self.hot) + len(self.res_hot) + (1 if self.res == "ident" else 0)

    @property
    def t_out(self):
        return t_out_of(self.T, self.stride) if self.kernel == "tcn" else self.T


# ---- case matrix ------------------------------------------------------------------------------------------------------
def _tcn_onehot(ci, co, stride, V, T, N):
    return [Case("tcn", ci, co, V, T, N, stride, hot=((s, c),)) for c in range(n_chunks(ci)) for s in range(K_TCN)]


def _gcn_onehot(ci, co, V, T, N):
    res = "ident" if ci == co else "conv"
    main = [Case("gcn", ci, co, V, T, N, hot=((r, c),), res=res) for c in range(n_chunks(ci)) for r in range(3)]
    phase2 = [Case("gcn", ci, co, V, T, N, res="conv", res_hot=(c,)) for c in range(n_chunks(ci))] if res == "conv" else []
    return main + phase2


def build_cases():
    cs = []
    # one-hot sweep of the temporal conv: every (tap slot, chunk) alone; several position tiles with a ragged last one, two segments
    cs += _tcn_onehot(64, 64, 1, 25, 45, 2)            # 64-row template, 1125 positions per segment
    cs += _tcn_onehot(64, 128, 1, 25, 21, 2)           # 128-row template, 525 positions
    cs += _tcn_onehot(128, 64, 2, 25, 90, 2)           # stride 2: class-major slots, even T
    cs += _tcn_onehot(128, 256, 2, 25, 41, 2)          # stride 2, two row tiles, odd T
    cs += _tcn_onehot(20, 12, 1, 25, 9, 1)             # ragged: the last chunk holds 4 channels, 12 of 64 rows
    cs += _tcn_onehot(130, 70, 2, 18, 13, 2)           # ragged: the last chunk holds 2 channels, 70 of 128 rows
    # T: a single frame (only the centre tap sees data), T < K (zero padding on both sides of every window)
    for ci, co, stride in ((64, 64, 1), (64, 128, 1), (128, 128, 2)):
        centre = tap_order(stride).index(4)
        cs += [Case("tcn", ci, co, 25, 1, 3, stride, hot=((s, 1),)) for s in sorted({0, centre, 8})]
        cs += [Case("tcn", ci, co, 25, 5, 2, stride, hot=((s, n_chunks(ci) - 1),)) for s in range(K_TCN)]
    # few-hot: neighbouring weight stages of a chunk, the hand-over to the next chunk's tile, both ping-pong parities
    for ci, co, stride, T in ((64, 64, 1, 45), (128, 256, 2, 41)):
        for hot in (((2, 0), (3, 0)), ((8, 0), (0, 1)), ((5, 1), (6, 2)), ((1, 0), (4, 0), (7, 0)), ((8, 1), (0, 2), (3, 2)),
                    ((2, 2), (5, 3), (8, 3))):
            cs.append(Case("tcn", ci, co, 25, T, 2, stride, hot=hot))
    # the K = 1 residual conv image alone (main conv weights zero), per chunk; then beside a hot main pair
    for ci, co, c_res, stride, V, T in ((128, 128, 64, 2, 25, 41), (64, 64, 64, 2, 25, 90), (128, 128, 64, 1, 25, 21), (12, 12, 20, 2, 18, 13)):
        cs += [Case("tcn", ci, co, V, T, 2, stride, res="conv", res_hot=(c,), c_res=c_res) for c in range(n_chunks(c_res))]
    cs.append(Case("tcn", 128, 128, 25, 41, 2, 2, hot=((7, 5),), res="conv", res_hot=(2,), c_res=64))
    cs.append(Case("tcn", 64, 64, 25, 90, 2, 2, hot=((0, 3),), res="conv", res_hot=(0,), c_res=64))
    # identity residual: alone (the output is x_res, bit for bit) and beside a hot pair
    cs.append(Case("tcn", 64, 64, 25, 45, 2, 1, res="ident", c_res=64))
    cs += [Case("tcn", 64, 64, 25, 45, 2, 1, hot=(h,), res="ident", c_res=64) for h in ((0, 0), (4, 1), (8, 3))]
    cs.append(Case("tcn", 128, 128, 25, 21, 2, 1, hot=((4, 7),), res="ident", c_res=128))
    cs.append(Case("tcn", 128, 128, 25, 1, 3, 1, hot=((4, 0),), res="ident", c_res=128))
    # graph conv: one-hot over (subset, chunk), the conv gcn_residual phase alone, both joint counts; one frame; few-hot
    for V, T in ((25, 21), (18, 30)):
        for ci, co in ((64, 128), (128, 128), (128, 256)):
            cs += _gcn_onehot(ci, co, V, T, 2)
    cs += [Case("gcn", 64, 128, 25, 1, 3, hot=((r, 3 - r),), res="conv") for r in range(3)]
    cs.append(Case("gcn", 64, 128, 18, 1, 3, res="conv", res_hot=(1,)))
    cs.append(Case("gcn", 128, 128, 18, 1, 3, hot=((1, 4),), res="ident"))
    for hot in (((2, 0), (0, 1)), ((0, 3), (1, 3), (2, 3))):
        cs.append(Case("gcn", 128, 256, 25, 21, 2, hot=hot, res="conv"))
    cs.append(Case("gcn", 64, 128, 25, 21, 2, hot=((1, 2),), res="conv", res_hot=(3,)))
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), "duplicate case"
    return cs


CASES = build_cases()
# the only dense comparisons: one per kernel, C_in 64 (K = 576 and K = 192)
DENSE = [Case("tcn", 64, 64, 25, 21, 2, 1, dense=True), Case("gcn", 64, 128, 25, 21, 2, res="conv", dense=True)]


def assert_matrix_covered(cases, dense):
    """every tap slot, chunk, tile template, stride, residual kind and graph-conv phase appears in the case list"""
    tcn = [c for c in cases if c.kernel == "tcn"]
    gcn = [c for c in cases if c.kernel == "gcn"]
    assert all(c.n_hot <= MAX_HOT and not c.dense for c in cases)
    assert [(c.kernel, c.ci, c.dense) for c in dense] == [("tcn", 64, True), ("gcn", 64, True)]
    onehot = {}
    for c in tcn:
        if len(c.hot) == 1 and c.res == "none":
            onehot.setdefault((c.ci, c.co, c.stride), set()).add(c.hot[0])
    for (ci, co, stride), want_template in (((64, 64, 1), 64), ((64, 128, 1), 128), ((128, 64, 2), 64), ((128, 256, 2), 128),
                                            ((20, 12, 1), 64), ((130, 70, 2), 128)):
        assert onehot[(ci, co, stride)] == {(s, ch) for s in range(9) for ch in range(n_chunks(ci))}, (ci, co, stride)
        assert next(c for c in tcn if (c.ci, c.co) == (ci, co)).template == want_template
    assert len(onehot[(64, 64, 1)]) == 36 and len(onehot[(128, 256, 2)]) == 72 and len(onehot[(130, 70, 2)]) == 81
    assert {c.template for c in tcn} == {64, 128} and {c.stride for c in tcn} == {1, 2}
    assert {c.res for c in tcn} == {"none", "ident", "conv"}
    for template in (64, 128):                                  # the K = 1 residual image alone, every chunk, stride 2, both templates
        alone = {c.res_hot for c in tcn if c.res == "conv" and not c.hot and c.stride == 2 and c.c_res == 64 and c.template == template}
        assert alone == {(0,), (1,), (2,), (3,)}
    assert any(c.res == "ident" and not c.hot for c in tcn) and any(c.res == "ident" and c.hot for c in tcn)
    assert {len(c.hot) for c in tcn} >= {0, 1, 2, 3}
    few = [c.hot for c in tcn if len(c.hot) > 1]
    stage = lambda h: 3 * h[1] + h[0] // 3                        # weight stage of a (slot, chunk) pair; its LDS buffer is stage & 1
    assert any(stage(b) == stage(a) + 1 and a[1] == b[1] for a, b, *_ in few)        # next stage, same activation tile
    assert any(stage(b) == stage(a) + 1 and b[1] == a[1] + 1 for a, b, *_ in few)    # next stage, next chunk's tile
    assert all(len({stage(h) for h in hot}) == len(hot) for hot in few)
    assert {stage(h) & 1 for hot in few for h in hot} == {0, 1}
    assert {c.T for c in tcn} >= {1, 5} and {c.N for c in tcn} >= {1, 2, 3}
    assert any(c.t_out * c.V > 2 * 32768 // c.template and (c.t_out * c.V) % (32768 // c.template) for c in tcn)   # > 2 tiles, ragged
    shapes = {(c.ci, c.co, c.V) for c in gcn}
    assert shapes == {(ci, co, V) for ci, co in ((64, 128), (128, 128), (128, 256)) for V in (18, 25)}
    for ci, co, V in shapes:
        mine = [c for c in gcn if (c.ci, c.co, c.V) == (ci, co, V)]
        assert {c.hot[0] for c in mine if len(c.hot) == 1 and not c.res_hot} >= {(r, ch) for r in range(3) for ch in range(n_chunks(ci))}
        if ci != co:                                             # phase 2: the conv gcn_residual on its own
            assert {c.res_hot for c in mine if not c.hot} >= {(ch,) for ch in range(n_chunks(ci))}
    assert {c.res for c in gcn} == {"ident", "conv"} and {c.T for c in gcn} >= {1} and {len(c.hot) for c in gcn} >= {0, 1, 2, 3}
    assert any(c.T * c.V > 512 and (c.T * c.V) % 256 for c in gcn)


# ---- fixtures ---------------------------------------------------------------------------------------------------------
def permutations(V):
    """the three adjacency subsets: identity and two permutations of the joints (0/1, one non-zero per column)"""
    idx = torch.arange(V)
    a = torch.zeros(3, V, V)
    for r, src in enumerate((idx, (idx + 1) % V, (idx * 7 + 3) % V)):       # 7 is coprime to 18 and to 25
        assert sorted(src.tolist()) == list(range(V))
        a[r, src, idx] = 1.0                                               # agg_r[..., w] = x[..., src[w]]
    return a


class Group:
    """One accumulation phase of a launch as a convolution: weight (C_out, C, k) and input (N, C, T, V), given as fp32 values
    and as their designed pieces; ``blocks``: the (tap, first channel, end channel) ranges in the order the kernel walks them."""

    def __init__(self, w, wp, x, xp, stride, pad, blocks):
        self.w, self.wp, self.x, self.xp, self.stride, self.pad, self.blocks = w, wp, x, xp, stride, pad, blocks


class Fixture:
    pass


def _seed(case, salt):
    return 1000003 * salt + 7919 * case.ci + 104729 * case.co + 31 * case.V + 17 * case.T + 5 * case.N + case.stride + 13 * case.c_res


def _scale_exp(n_terms):
    """weights are scaled by 2^-e: the smallest e >= 0 with n_terms * 1.25^2 * 2^-e (+ 1.25 for a residual) under REF_CAP"""
    return max(0, math.ceil(math.log2(max(n_terms, 1) * 1.5625 / (REF_CAP - 2.0))))


def build(case):
    """-> Fixture: designed operands of the case, masked to its hot pairs and scaled (module docstring)."""
    fx = Fixture()
    fx.case = case
    ci, co, V, T, N = case.ci, case.co, case.V, case.T, case.N
    k = K_TCN if case.kernel == "tcn" else 3
    slots = tap_order(case.stride) if case.kernel == "tcn" else [0, 1, 2]
    w, wp = designed((co, ci, k), _seed(case, 1))
    x, xp = designed((N, ci, T, V), _seed(case, 2))
    mask = torch.zeros(co, ci, k)
    if case.dense:
        mask[:] = 1.0
    for s, c in case.hot:
        assert 0 <= s < k and 0 <= c < n_chunks(ci)
        mask[:, KS * c: KS * (c + 1), slots[s]] = 1.0
    per_chunk = lambda c_total, c: min(KS, c_total - KS * c)
    n_terms = ci * k if case.dense else sum(per_chunk(ci, c) for _, c in case.hot)
    c_r = case.c_res if case.kernel == "tcn" else ci
    n_terms += sum(per_chunk(c_r, c) for c in case.res_hot)
    fx.e = _scale_exp(n_terms)
    sc = 2.0 ** -fx.e
    fx.w = w * mask * sc
    fx.wp = tuple(p * mask * sc for p in wp)
    fx.x, fx.xp = x, xp
    fx.addend, fx.groups = None, []
    fx.w_res = fx.w_resp = fx.x_res = fx.x_resp = None
    if case.kernel == "tcn":
        order = [(slots[s], KS * c, min(KS * (c + 1), ci)) for c in range(n_chunks(ci)) for s in range(k)]
        fx.groups.append(Group(fx.w, fx.wp, x, xp, case.stride, PAD_TCN, order))
        if case.res != "none":
            fx.x_res, fx.x_resp = designed((N, case.c_res, T, V), _seed(case, 3))
        if case.res == "ident":
            assert case.c_res == co and case.stride == 1
            fx.addend = fx.x_res
    else:
        fx.adj = permutations(V)
        src = [fx.adj[r].argmax(0) for r in range(3)]                      # source joint of every output joint
        xe = torch.cat([x[..., s] for s in src], 1)                       # (N, 3 ci, T, V): the aggregated input of subset r at r * ci
        xep = tuple(torch.cat([p[..., s] for s in src], 1) for p in xp)
        flat = lambda t: t.permute(0, 2, 1).reshape(co, 3 * ci, 1)        # (co, ci, 3) -> channels r * ci + c, one tap
        order = [(0, r * ci + KS * c, r * ci + min(KS * (c + 1), ci)) for c in range(n_chunks(ci)) for r in range(3)]
        fx.groups.append(Group(flat(fx.w), tuple(flat(p) for p in fx.wp), xe, xep, 1, 0, order))
        if case.res == "ident":
            assert ci == co
            fx.addend = x
        elif case.res == "conv":
            fx.x_res, fx.x_resp = x, xp
    if case.res == "conv":
        c_r = fx.x_res.shape[1]
        wr, wrp = designed((co, c_r, 1), _seed(case, 4))
        rmask = torch.zeros(co, c_r, 1)
        for c in case.res_hot:
            assert 0 <= c < n_chunks(c_r)
            rmask[:, KS * c: KS * (c + 1)] = 1.0
        fx.w_res, fx.w_resp = wr * rmask * sc, tuple(p * rmask * sc for p in wrp)
        order = [(0, KS * c, min(KS * (c + 1), c_r)) for c in range(n_chunks(c_r))]
        fx.groups.append(Group(fx.w_res, fx.w_resp, fx.x_res, fx.x_resp, case.stride, 0, order))
    return fx


# ---- arithmetic of a fixture ------------------------------------------------------------------------------------------------
def _window(x, tap, stride, pad, t_out):
    """the input frames tap + stride * t - pad of every output frame t, zero outside [0, T)"""
    xz = F.pad(x, (0, 0, pad, pad))
    return xz[:, :, tap: tap + stride * (t_out - 1) + 1: stride]


def conv64(w, x, stride, pad):
    """out[n, o, t, v] = sum_r sum_c w[o, c, r] * x[n, c, stride t + r - pad, v] in fp64 (zero outside [0, T)): the
    convolution sum written out, one einsum per tap; taps and channels whose weights are all zero are left out."""
    co, c, k = w.shape
    n, _, t_in, v = x.shape
    t_out = (t_in + 2 * pad - k) // stride + 1
    out = torch.zeros((n, co, t_out, v), dtype=torch.float64)
    w64, x64 = w.double(), x.double()
    for r in range(k):
        ch = torch.nonzero(w64[:, :, r].abs().sum(0)).flatten()
        if ch.numel():
            out += torch.einsum("oc,nctv->notv", w64[:, ch, r], _window(x64[:, ch], r, stride, pad, t_out))
    return out


def analyse(fx):
    """-> dict: want, six, nz (outputs that have terms), D, tol = D / 2, bound, drops (six without mm / hl / lh)."""
    case = fx.case
    add = 0.0 if fx.addend is None else fx.addend.double()
    want = sum(conv64(g.w, g.x, g.stride, g.pad) for g in fx.groups) + add
    prod = {pq: sum(conv64(g.wp[pq[0]], g.xp[pq[1]], g.stride, g.pad) for g in fx.groups) for pq in SIX}
    six = sum(prod.values()) + add
    sum_abs = sum(conv64(g.w.abs(), g.x.abs(), g.stride, g.pad) for g in fx.groups)
    with_terms = sum_abs > 0                                                                   # outputs that products reach
    nz = with_terms if fx.addend is None else torch.ones_like(with_terms)
    out = dict(want=want, six=six, nz=nz, with_terms=with_terms, drops={}, D=None, tol=0.0, bound=0.0)
    if not bool(with_terms.any()):
        return out                  # nothing is multiplied: the output is the residual (or zero), bit for bit
    devs = []
    for name, pq in SECOND.items():
        out["drops"][name] = six - prod[pq]
        devs.append((prod[pq][with_terms] / six[with_terms]).abs().min())
    out["D"] = float(min(devs))
    out["tol"] = out["D"] / 2
    sum_abs = sum_abs + (0.0 if fx.addend is None else fx.addend.double().abs())
    out["bound"] = float(((6 * case.n_hot + 16) * UNIT * sum_abs[nz] / want[nz].abs()).max())      # (all terms positive: the ratio is 1)
    return out


def restate32(fx):
    """The six piece products accumulated in fp32 the way the kernel issues them: phases in turn, chunk by chunk, slot by slot,
    hl lh mm mh hm hh; per matrix instruction the (up to) 16 channel products are summed sequentially in fp32 and that sum is
    added to the accumulator; then the identity residual.  A product of two bf16 values is exact in fp32."""
    assert fx.groups
    acc = None
    for g in fx.groups:
        co, c, k = g.w.shape
        n, _, t_in, v = g.x.shape
        t_out = (t_in + 2 * g.pad - k) // g.stride + 1
        if acc is None:
            acc = torch.zeros((n, co, t_out, v), dtype=torch.float32)
        for tap, lo, hi in g.blocks:
            if not bool(g.w[:, lo:hi, tap].any()):
                continue            # zero weights add exact zeros
            wins = [_window(p[:, lo:hi], tap, g.stride, g.pad, t_out) for p in g.xp]
            for a, b in SIX:
                dot = torch.zeros_like(acc)
                for ch in range(hi - lo):
                    dot = dot + g.wp[a][:, lo + ch, tap].view(1, co, 1, 1) * wins[b][:, ch: ch + 1]
                acc = acc + dot
    if fx.addend is not None:
        acc = acc + fx.addend
    return acc


def rel_err(got, ref, where):
    """largest |got - ref| / |ref| over the outputs selected by ``where``"""
    if not bool(where.any()):
        return 0.0
    return float(((got.double() - ref)[where] / ref[where]).abs().max())


def check_case(got, an, **info):
    """Assert a kernel output against the analysis of its fixture: exactly zero where no term reaches an output, within
    tol = D / 2 relative at every other output, |want| <= REF_CAP; one JSON line in the parity report (tests/helpers.py)."""
    want, nz = an["want"], an["nz"]
    got = torch.as_tensor(got).double()
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape), info)
    ref = float(want.abs().max())
    err_rel = rel_err(got, want, nz)
    signed = float(((got - want)[nz] / want[nz]).mean()) if bool(nz.any()) else 0.0      # a one-sided mean shows a systematic loss
    stray = int((got[~nz] != 0).sum())
    path = _report_path()
    if path:
        try:
            with open(path, "a") as f:
                f.write(json.dumps(dict(test=os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], max_abs_err=float((got - want).abs().max()),
                                        absmax_ref=ref, tol=an["tol"], tol_kind="relative per output, D / 2", max_rel_err=err_rel, mean_signed_rel_err=signed,
                                        D=an["D"], bound=an["bound"], stray_nonzeros=stray, n=int(want.numel()), mode="bf16x3", **info)) + "\n")
        except OSError:
            pass
    assert ref <= REF_CAP, f"fixture not O(1): |want| max = {ref:.3g} {info}"
    assert stray == 0, f"{stray} outputs that no term reaches are not exactly zero {info}"
    assert err_rel <= an["tol"], f"max relative error {err_rel:.3e} > D / 2 = {an['tol']:.3e} {info}"
    return err_rel


def pack_images(fx, fold):
    """-> (w_split, w_res_split or None): the operand images of the launch, packed by fold.pack_conv_weight_split with a unit
    scale (no rounding on the way in: the CPU tests compare the images with the designed pieces bit for bit)."""
    case = fx.case
    one = torch.ones(case.co, dtype=torch.float64)
    w_img = fold.pack_conv_weight_split(fx.w, one, case.stride if case.kernel == "tcn" else 1)
    r_img = fold.pack_conv_weight_split(fx.w_res, one) if fx.w_res is not None else None
    return w_img, r_img
