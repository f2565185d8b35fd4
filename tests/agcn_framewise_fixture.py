"""Cases, operands, the fp64 definition and the error bound shared by tests/test_gpu_agcn_framewise.py and
tests/test_agcn_framewise_fixture_cpu.py: the adaptive graph-conv stage applied per frame (csrc/agcn_framewise.hip,
csk_agcn_stage_framewise_f32; models/coa_gcn/coa_gcn.py:11-14, the step form of the module).  For frame t of segment n, from the FOLDED
operands (embedding weights W_e / b_e in E's channel order a_0 a_1 a_2 b_0 b_1 b_2, a_sum = A + graph_attn, stage weights W [R][C_out][C_in]
with the BN folded, bias):

    E          = W_e x[n, :, t, :] + b_e
    l_i[v, w]  = sum_k Ea_i[k, v] Eb_i[k, w] / inter
    adj_i      = softmax over v of l_i + a_sum_i
    y[n, :, t, w] = ReLU( sum_i W_i (x[n, :, t, :] adj_i)[:, w] + bias + res ),   res = x (identity) or W_3 x (conv)

Two tiers of operands.
  exact     x in {-1, 0, 1}; the a_i rows have zero weights and a bias in {-1, 0, 1}, so Ea does not depend on v and every logit column
            is uniform: the softmax is 1 / V whatever the hardware exponential does (exp(0) = 1, the column sum V, one IEEE
            division: r = fl(1 / V)).  a_sum = q - r with q in {0, 1, 2, 3} / 32 -- exact in fp32, both are multiples of 2^-28 below
            2^-4 -- so adj = fl(r + a_sum) = q.  Stage weights in {-1, 0, 1}, integer bias: every sum is a multiple of 1 / 32 below
            2^24 / 32 in any order (admissible() asserts it): the output is exact and compared BIT FOR BIT.
  positive  every operand positive (x, W_e, b_e, a_sum, W, bias): no cancellation anywhere, so relative errors add up.  With
            u = 2^-24, nz the most non-zero weights of an embedding row (zero products add no rounding error):
              eE = (nz + 2) u                      the embedding row: nz products, nz adds, the bias add
              eL = 2 eE + (inter + 1) u            a logit sum of inter products of two embeddings; the scale 1 / inter is a power of two
              dl = eL Lmax;  dd = 2 dl + u span;  re = 2 u span + 2 u + dd;  rho = 2 re + (V + 1) u + 2 u
                                                   the softmax, term for term as tests/agcn_attention_fixture.py derives it (there dl
                                                   is 2 u Lmax: exact embeddings), Lmax / span the largest logit / column span of the case
              eA = rho + u                         adj = p + a_sum, both positive
              eB = eA + (V + 1) u                  the aggregation over V joints (x exact)
              eY = eB + (R C_in + 3) u             the channel mix over R C_in terms, bias and residual adds
            bound = 1.05 eY y (5 % for the second-order terms).  It is derived, not measured; ReLU is the identity on these cases.
numpy only; nothing is read from csrc."""
from collections import namedtuple

import numpy as np

from tests import agcn_attention_fixture as att

U = att.U
f32, f64 = np.float32, np.float64
FT = att.FT                                             # frames per tile of the kernel: 128 // V
INTERS = (16, 32, 64)

Case = namedtuple("Case", "name n_seg c_in c_out T V conv_res seg_pad")


def _cases():
    out, k = [], 0
    for V in (18, 25):
        ts = (1, FT[V] - 1, FT[V], FT[V] + 1, 2 * FT[V] + 3)
        # the four layer shapes with every T; the other residual form of each inter (and layer 1: C_in = 3) with the two longest
        for c_in, c_out, conv, full in ((64, 64, False, True), (64, 128, True, True), (128, 128, False, True), (256, 256, False, True),
                                        (256, 256, True, False), (3, 64, True, False), (64, 64, True, False), (128, 128, True, False)):
            for T in ts if full else ts[3:]:
                out.append(Case(f"fw-V{V}-c{c_in}x{c_out}-{'conv' if conv else 'ident'}-T{T}-n{(1, 3)[k % 2]}", (1, 3)[k % 2], c_in, c_out, T, V, conv, 0))
                k += 1
        # one case with a gap behind every segment of x and y (even V: the gap keeps rows 8-byte aligned)
        out.append(Case(f"fw-V{V}-c64x64-ident-T{FT[V] + 1}-n3-strided", 3, 64, 64, FT[V] + 1, V, False, 6))
    return out


CASES = _cases()
# one case per instantiation for the bitwise frame-independence test: the longest of each
PER_INSTANTIATION = {}
for _c in CASES:
    _key = (_c.c_out // 4, _c.V, _c.conv_res)
    if _key not in PER_INSTANTIATION or _c.T > PER_INSTANTIATION[_key].T:
        PER_INSTANTIATION[_key] = _c


def inter_of(c):
    return c.c_out // 4


def route_of(c):
    """what csk_agcn_stage_framewise_f32_route reports: INTER * 1000 + V * 10 + CONVRES"""
    return inter_of(c) * 1000 + c.V * 10 + int(c.conv_res)


ALL_ROUTES = sorted(i * 1000 + V * 10 + r for i in INTERS for V in (18, 25) for r in (0, 1))


# ---- operands -------------------------------------------------------------------------------------------------------------------
def _rng(c, tier):
    return np.random.default_rng(np.random.SeedSequence([17, c.n_seg, c.c_in, c.c_out, c.T, c.V, int(c.conv_res), c.seg_pad, len(tier)]))


def operands(c, tier):
    """-> dict(x [n, c_in, T, V], we [6 inter, c_in], be, a_sum [3, V(v), V(w)], W [R, c_out, c_in], bias [c_out]) in fp32, + adj_exact
    [3, V, V] on the exact tier (the adjacency every frame gets by construction)"""
    rng, inter, V = _rng(c, tier), inter_of(c), c.V
    R = 4 if c.conv_res else 3
    rows = 6 * inter
    we, be = np.zeros((rows, c.c_in), dtype=f32), np.zeros(rows, dtype=f32)
    if tier == "exact":
        x = rng.integers(-1, 2, size=(c.n_seg, c.c_in, c.T, V)).astype(f32)
        be[: 3 * inter] = rng.integers(-1, 2, size=3 * inter)
        for r in range(3 * inter, rows):
            ch = rng.choice(c.c_in, size=2, replace=False)
            we[r, ch[0]] = rng.choice((-1, 1))
            if r % 2:
                we[r, ch[1]] = rng.choice((-1, 1))
            else:
                be[r] = rng.integers(-1, 2)
        q = (rng.integers(0, 4, size=(3, V, V)) / 32.0).astype(f32)
        r_ = f32(1) / f32(V)
        a_sum = (q - r_).astype(f32)
        assert np.array_equal(f64(a_sum), f64(q) - f64(r_)) and np.array_equal((r_ + a_sum).astype(f32), q)
        W = rng.integers(-1, 2, size=(R, c.c_out, c.c_in)).astype(f32) * (rng.random((R, c.c_out, c.c_in)) < 0.3)
        bias = rng.integers(-2, 3, size=c.c_out).astype(f32)
        return dict(x=x, we=we, be=be, a_sum=a_sum, W=W.astype(f32), bias=bias, adj_exact=q)
    x = rng.random((c.n_seg, c.c_in, c.T, V), dtype=f32)
    for r in range(rows):
        ch = rng.choice(c.c_in, size=2, replace=False)
        we[r, ch] = (rng.random(2, dtype=f32) + f32(0.5))
        be[r] = rng.random(dtype=f32)
    a_sum = (rng.random((3, V, V), dtype=f32) * f32(0.05)).astype(f32)
    W = (rng.random((R, c.c_out, c.c_in), dtype=f32) / f32(c.c_in)).astype(f32)
    bias = rng.random(c.c_out, dtype=f32)
    return dict(x=x, we=we, be=be, a_sum=a_sum, W=W, bias=bias)


def stage_image(W, bias):
    """[R][c_out][c_in] -> the packed image csk_gcn_stage_f32 takes, [R][c_in_pad][c_out_pad], and the padded bias"""
    R, co, ci = W.shape
    img = np.zeros((R, att.cpad(ci), att.mpad(co)), dtype=f32)
    img[:, :ci, :co] = np.transpose(W, (0, 2, 1))
    b = np.zeros(att.mpad(co), dtype=f32)
    b[:co] = bias
    return img, b


# ---- the definition, fp64 ----------------------------------------------------------------------------------------------------------
DEFECTS = ("neighbour_frame", "softmax_wrong_index", "dropped_subset", "no_a_sum")


def logits(ops, inter):
    """-> l [n, 3, T, V(v), V(w)] fp64"""
    E = att.embed(ops["x"], ops["we"], ops["be"])
    n, _, T, V = E.shape
    ea, eb = E[:, : 3 * inter].reshape(n, 3, inter, T, V), E[:, 3 * inter:].reshape(n, 3, inter, T, V)
    return np.einsum("niktv,niktw->nitvw", ea, eb) / inter


def definition(ops, inter, conv_res, defect=None, adj=None):
    """y [n, c_out, T, V] in fp64 (``adj`` [3, V, V]: that adjacency for every frame instead of the attention -- the exact tier).  One seeded
    defect: the attention of frame t + 1 used for frame t; the softmax over w instead of v; subset 2 left out of the sum; a_sum left out"""
    x, W = f64(ops["x"]), f64(ops["W"])
    if adj is None:
        l = logits(ops, inter)
        ax = 4 if defect == "softmax_wrong_index" else 3
        e = np.exp(l - l.max(axis=ax, keepdims=True))
        A = e / e.sum(axis=ax, keepdims=True)
        if defect != "no_a_sum":
            A = A + f64(ops["a_sum"])[None, :, None]
        if defect == "neighbour_frame":
            A = np.roll(A, -1, axis=2)
    else:
        A = np.broadcast_to(f64(adj)[None, :, None], (x.shape[0], 3, x.shape[2]) + adj.shape[1:])
    agg = np.einsum("nctv,nitvw->nictw", x, A)
    nsub = 2 if defect == "dropped_subset" else 3
    y = np.einsum("ioc,nictw->notw", W[:nsub], agg[:, :nsub]) + f64(ops["bias"])[None, :, None, None]
    y = y + (np.einsum("oc,nctw->notw", W[3], x) if conv_res else x)
    return np.maximum(y, 0.0)


def bound(c, ops, y):
    """the positive tier's bound (module docstring), elementwise on the fp64 result y"""
    inter, V = inter_of(c), c.V
    l = logits(ops, inter)
    lmax = float(np.abs(l).max())
    span = float((l.max(axis=3) - l.min(axis=3)).max())
    nz = int((ops["we"] != 0).sum(axis=1).max())
    eE = (nz + 2) * U
    eL = 2 * eE + (inter + 1) * U
    dl = eL * lmax
    dd = 2 * dl + U * span
    re = 2 * U * span + 2 * U + dd
    rho = 2 * re + (V + 1) * U + 2 * U
    eB = rho + U + (V + 1) * U
    eY = eB + ((4 if c.conv_res else 3) * c.c_in + 3) * U
    return 1.05 * eY * np.abs(y)


def admissible(c, ops):
    """exact tier: uniform logit columns, and every sum a multiple of 1 / 32 below 2^24 / 32 in any order"""
    l = logits(ops, inter_of(c))
    assert float((l.max(axis=3) - l.min(axis=3)).max()) == 0.0
    mag = (c.V * 3 / 32.0) * np.abs(f64(ops["W"][:3])).sum(axis=(0, 2)).max() + np.abs(f64(ops["W"][3:])).sum(axis=(0, 2)).max() + 3.0
    assert mag * 32 < 2 ** 24
    return mag


# ---- the head's index map, restated from the step rule -------------------------------------------------------------------------------
def head_map_by_stepping(emitted, flushed, pool_size, pool_padding, pad_end):
    """Simulate the continual head (continual.py: _head_step / _flush): ``emitted`` feature frames arrive one by one, with pad_end the
    ``flushed`` further ones the block flush releases and then ``pool_padding`` zero entries.  -> (feature frames taken, [(first,
    last) entry of the window behind every prediction])"""
    feats, preds = 0, []
    total = emitted + ((flushed + pool_padding) if pad_end else 0)
    for _ in range(total):
        feats += 1
        if feats >= pool_size - pool_padding:
            preds.append((feats - min(feats, pool_size), feats - 1))
    return emitted + (flushed if pad_end else 0), preds
