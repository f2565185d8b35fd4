"""Cases, operands, fp64 references, error bounds and a seeded-defect host model for the stage-wise pin of the S-TR attention unit
(csrc/str.hip, csk_str_unit_f32): shared by tests/test_gpu_str_unit.py and tests/test_str_unit_fixture_cpu.py.  The three launches

    qkv = w_qkv^T (s_in x + t_in) + b_qkv                                  str_gemm_kernel<MI, 1, 0, 0>, MI in {2, 4}
    o[h dvh + d, i] = sum_j softmax_j(sum_e q[h dkh + e, i] k[h dkh + e, j]) v[h dvh + d, j]     str_attention_kernel<V, DKH>
    y   = ReLU(w_out^T o + b_out (+ res_scale x))                          str_gemm_kernel<2, 0, RES, 1>

leave qkv [n_seg][2 dk + dv][frames V] at scratch offset 0 and o [n_seg][dv][frames V] behind it (include/cskel.h), so every stage is
judged on its own image.  The tests call the C ABI with the packed operands built here (w [K][Mpad], rows >= M zero).

Exact operands (form "designed").  Everything is an integer, so fp32 is exact in any order (admissible() asserts sum |term| < 2^24
for every sum of every stage, in units of 2^-4 behind the softmax).  The channels of x^ = s_in x + t_in are: dkh selectors
(x^[e, i] = +-1 if e == i mod dkh else 0), max(dkh, 4) patterns B_e[j] in {-1, 0, 1}, one id channel (a distinct integer per column
of the launch), one constant 1 (it takes back the bias of the q / k rows), and noise channels in pairs (c, c') with x^[c'] = -x^[c] and
equal weights, partners half the noise range apart: they cancel in every row, but only if every chunk is summed exactly once.
q rows carry +-1 on their selector, k rows +-128 on a pattern that differs per head, so a logit is 128 s B[j]: for every
(frame, head, query) the maximum is attained on the tie set J = {j: B[j] = s} of 2^n keys and every other logit lies >= 128 below;
exp(-128) < 2^-150 rounds to 0 in fp32 and in fp64 (asserted), exp(0) = 1, the sum is 2^n, the weights are 2^-n and
o = 2^-n sum_{j in J} v_j exactly.  v row r holds id(column) + NC r, NC above every id: distinct per (row, joint, frame, segment).
w_out has +-1 entries, as many per row as the 2^24 budget allows (all of them in the small cases), one all-zero row, integer
b_out / res_scale: y before the ReLU is negative, zero and positive in every case (asserted).  Forms "onehot1" / "onehot3": the QKV
GEMM resp. the projection with one-hot weights, every output element the copy of ONE input element with a unique id.

Rounding cases.  Real operands, O(1) activations; flavour "peaked" scales the q / k rows to logits of about +-6, "flat" to about
+-0.5 (there the exponential's own error is the largest share of the bound).  Each stage is judged on its ACTUAL input (stage 2 on
the qkv image read back, stage 3 on the o image read back, both taken as exact fp32 inputs of the fp64 definition).  With u = 2^-24,
g(n) = n u / (1 - n u):
  * GEMM stages: |err| <= g(K + 2) (sum_k |w| |x^| + |b| + |res_scale x|): K for the products and the accumulation, 2 for the affine
    fma and the bias add (QKV) resp. the bias add and the residual fma (projection); the ReLU is 1-Lipschitz.
  * attention, per (frame, head, query i), A_j = sum_e |q_e| |k_ej|, l the exact logits, d = l - max l, e = exp(d), p = e / sum e:
      dl_j = (DKH + 1) u A_j                                       the fma chain of the logit
      dd_j = dl_j + max dl + u (|d_j| + dl_j + max dl)             the computed maximum and the subtraction
      re_j = expm1(dd_j) + EXPF_REL exp(dd_j)                      the argument's error through exp, and expf's own error
      rs   = R + g(V - 1) (1 + R),  R = sum re_j e_j / sum e_j     the V-term sum of positive terms
      rho_j = (1 + re_j) (1 + u)^2 / (1 - rs) - 1                  the division and the product
      bound = sum_j p_j |v_j| (rho_j + g(V) (1 + rho_j))           the V-term fma chain of the weighted sum
    EXPF_REL = EXPF_ULPS * 2 u is the one term the code does not give.  No HIP math-accuracy table ships in the ROCm tree this was
    written against, so EXPF_ULPS = 2: the convention tests/agcn_attention_fixture.py uses for the hardware exponential.
The bounds are derived, not measured.  numpy only; nothing is read from csrc."""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
EXPF_ULPS = 2
EXPF_REL = EXPF_ULPS * 2 * U
f32, f64 = np.float32, np.float64
NH, MT, NT, KC = 8, 64, 256, 16

Case = namedtuple("Case", "c_in c_out V n_seg frames layout has_res")
CASES = [
    Case(32, 32, 18, 1, 1, "dense", 1),        # M = 48 of 64 rows, one wave stores, both grids 1
    Case(16, 32, 25, 3, 11, "ring", 0),        # one chunk; 275 columns, frame 10 straddles column 256
    Case(16, 32, 18, 1, 128, "dense", 0),      # 2304 columns = 9 full tiles
    Case(64, 64, 25, 1, 1, "ring", 1),         # MI = 4, M = 96 of 128 rows
    Case(48, 64, 18, 3, 15, "dense", 0),       # three chunks; 270 columns, frame 14 straddles column 256
    Case(64, 64, 25, 3, 41, "ring", 1),        # 1025 columns: the last tile holds one column
    Case(32, 64, 25, 1, 80, "dense", 0),       # 2000 columns: both grids 8
    Case(128, 128, 18, 1, 1, "dense", 1),      # M = 192: three full 64-row tiles
    Case(48, 128, 25, 1, 11, "ring", 0),
    Case(128, 128, 25, 3, 41, "dense", 1),
    Case(256, 256, 25, 3, 41, "ring", 1),      # the largest launch: 3 x 1025 x 384, K = 256
    Case(32, 256, 18, 1, 1, "dense", 0),
    Case(48, 256, 18, 3, 15, "ring", 0),
]
ROUND = [(c, "peaked") for c in CASES] + [(c, "flat") for c in CASES if c.c_out <= 64 and c.frames * c.V <= 300]


def name(c, tag=None):
    return f"{c.c_in}to{c.c_out}-V{c.V}-seg{c.n_seg}-f{c.frames}-{c.layout}-{'res' if c.has_res else 'nores'}" + (f"-{tag}" if tag else "")


def dims(c):
    """-> dk, dkh, dvh, M (rows of qkv), ncols"""
    dk = c.c_out // 4
    return dk, dk // NH, c.c_out // NH, 2 * dk + c.c_out, c.frames * c.V


def mpad(m):
    return -(-m // MT) * MT


# ---- the selection, restated ----------------------------------------------------------------------------------------------------
def gemm_tiling(affine, M, ncols, n_seg):
    """-> (MI, row tiles, column tiles, grid): 128-row tiles for the QKV launch where the packed width is a multiple of 128"""
    wide = affine and M > 64 and mpad(M) % 128 == 0
    mtiles, ctiles = mpad(M) // (128 if wide else 64), -(-ncols // NT)
    return (4 if wide else 2), mtiles, ctiles, mtiles * ctiles * n_seg


def select(c):
    """what csk_str_unit_f32_route must say: [MI, mtiles, ctiles, grid | V, DKH, grid | RES, MI, mtiles, ctiles, grid]"""
    dk, dkh, dvh, M, ncols = dims(c)
    return list(gemm_tiling(True, M, ncols, c.n_seg)) + [c.V, dkh, c.n_seg * c.frames] + [int(bool(c.has_res))] + \
        list(gemm_tiling(False, c.c_out, ncols, c.n_seg))


def instantiations(c):
    r = select(c)
    return ("gemm", r[0], 1, 0, 0), ("att", r[4], r[5]), ("gemm", r[8], 0, r[7], 1)


def tile_kinds(c):
    """the tile kinds the two GEMM launches of the case hold"""
    dk, dkh, dvh, M, ncols = dims(c)
    kinds = set()
    for affine, rows, K in ((True, M, c.c_in), (False, c.c_out, c.c_out)):
        mi, mtiles, ctiles, grid = gemm_tiling(affine, rows, ncols, c.n_seg)
        if rows < mtiles * 32 * mi:
            kinds.add("ragged_rows")
            if mi == 4 and rows > (mtiles - 1) * 128 + 64:
                kinds.add("ragged_rows_upper_half")
        if ncols % NT:
            kinds.add("ragged_cols")
        else:
            kinds.add("full_cols")
        if ncols % NT == 1:
            kinds.add("one_column_tile")
        if ncols < 64:
            kinds.add("one_wave_stores")
        if any((f * c.V) // NT != ((f + 1) * c.V - 1) // NT for f in range(c.frames)):
            kinds.add("frame_straddles_seam")
        if K == KC:
            kinds.add("one_chunk")
        if (K // KC) % 2 and K > KC:
            kinds.add("odd_chunks")
        kinds.add("grid_1" if grid == 1 else "grid_mult_8" if grid % 8 == 0 else "grid_rem_8")
    return kinds


def strides(c, ncols, layout, extra):
    """(segment stride, channel stride), as tests/test_gpu_str_hardening.py builds them"""
    if layout == "dense":
        return c * ncols, ncols
    chan = (ncols + 3) // 4 * 4 + extra
    return c * chan + 2 * extra, chan


def xy_strides(c):
    ncols = c.frames * c.V
    return strides(c.c_in, ncols, c.layout, 12), strides(c.c_out, ncols, c.layout, 4)


def body(n, C, ncols, st):
    return (n - 1) * st[0] + (C - 1) * st[1] + ncols


def place(t3, st, fill=np.nan, dtype=f32):
    """[n, C, ncols] -> flat buffer with the strides, `fill` in between"""
    n, C, ncols = t3.shape
    flat = np.full(body(n, C, ncols, st), fill, dtype=dtype)
    flat[index(n, C, ncols, st)] = t3
    return flat


def index(n, C, ncols, st):
    return (np.arange(n)[:, None, None] * st[0] + np.arange(C)[None, :, None] * st[1] + np.arange(ncols)[None, None, :])


# ---- operands -------------------------------------------------------------------------------------------------------------------
def _rng(c, *key):
    return np.random.default_rng(np.random.SeedSequence([c.c_in, c.c_out, c.V, c.n_seg, c.frames, int(c.layout == "ring"), c.has_res] + [int(k) for k in key]))


SIZES = {18: [(16, 2), (8, 4), (1, 8), (4, 1), (2, 16), (8, 8)], 25: [(16, 8), (8, 4), (1, 16), (4, 1), (2, 16), (16, 2)]}


def _pack(w_rows, b_rows):
    """w [M][K], b [M] -> packed [K][Mpad], [Mpad]"""
    M, K = w_rows.shape
    w = np.zeros((K, mpad(M)), dtype=f32)
    w[:, :M] = w_rows.T
    b = np.zeros(mpad(M), dtype=f32)
    b[:M] = b_rows
    return w, b


def exact_operands(c, form="designed"):
    """-> dict: x [n, K, ncols], w_qkv, b_qkv, s_in, t_in, w_out, b_out, res_scale (None without the skip); J [n, 8, T, V(i), V(j)] the
    designed tie sets (designed / onehot3); g = log2 of the largest tie set"""
    dk, dkh, dvh, M, ncols = dims(c)
    K, V, n, T, co = c.c_in, c.V, c.n_seg, c.frames, c.c_out
    rng = _rng(c, 1)
    if form == "onehot1":
        x = (np.arange(n * K * ncols, dtype=f64) + 1).reshape(n, K, ncols)
        wr = np.zeros((M, K))
        wr[np.arange(M), (7 * np.arange(M) + 3) % K] = 1
        w_qkv, b_qkv = _pack(wr, np.zeros(M))
        w_out, b_out = _pack(np.zeros((co, co)), np.ones(co))
        return dict(x=x.astype(f32), w_qkv=w_qkv, b_qkv=b_qkv, s_in=np.ones((K, V), f32), t_in=np.zeros((K, V), f32), w_out=w_out, b_out=b_out,
                    res_scale=np.zeros(co, f32) if c.has_res else None, src=(7 * np.arange(M) + 3) % K)
    nsel, npat = dkh, max(dkh, 4)
    idc, one = nsel + npat, nsel + npat + 1
    ndes = (one + 2) // 2 * 2
    half = (K - ndes) // 2
    assert half >= 1, "the case has no room for noise channels"
    i = np.arange(V)
    sig = np.where((i[None, None, :] // dkh + np.arange(T)[None, :, None] + np.arange(n)[:, None, None]) % 2 == 0, 1, -1)      # [n, T, V]
    xh = np.zeros((n, K, T, V))
    for e in range(nsel):
        xh[:, e] = sig * (i % dkh == e)
    B = np.zeros((n, T, npat, V))
    for s in range(n):
        for t in range(T):
            for e in range(npat):
                a, b = SIZES[V][(e + t + s) % 6]
                perm = rng.permutation(V)
                B[s, t, e, perm[:a]], B[s, t, e, perm[a:a + b]] = 1, -1
    xh[:, nsel:nsel + npat] = np.transpose(B, (0, 2, 1, 3))
    xh[:, idc] = (np.arange(n * T * V) + 1).reshape(n, T, V)
    xh[:, one] = 1
    xh[:, ndes:ndes + half] = rng.integers(-3, 4, size=(n, half, T, V))
    xh[:, ndes + half:] = -xh[:, ndes:ndes + half]
    s_in = rng.choice((-1.0, 1.0), size=(K, V))
    t_in = rng.integers(-2, 3, size=(K, V)).astype(f64)
    s_in[ndes + half:], t_in[ndes + half:] = -s_in[ndes:ndes + half], -t_in[ndes:ndes + half]
    x = s_in[None, :, None, :] * (xh - t_in[None, :, None, :])
    NC = n * T * V + 1
    wr, br = np.zeros((M, K)), np.zeros(M)
    tq, sk = rng.choice((-1, 1), size=(NH, dkh)), rng.choice((-1, 1), size=(NH, dkh))
    for h in range(NH):
        for d in range(dkh):
            wr[h * dkh + d, d] = tq[h, d]
            wr[dk + h * dkh + d, nsel + (d + h) % npat] = 128 * sk[h, d]
    br[:2 * dk] = rng.integers(-3, 4, size=2 * dk)
    wr[:2 * dk, one] = -br[:2 * dk]
    wr[2 * dk:, idc] = 1
    br[2 * dk:] = NC * np.arange(co)
    noise = rng.integers(-2, 3, size=(M, half))
    wr[:, ndes:ndes + half], wr[:, ndes + half:] = noise, noise
    w_qkv, b_qkv = _pack(wr, br)
    J = np.zeros((n, NH, T, V, V), dtype=bool)
    for h in range(NH):
        for q in range(V):
            d = q % dkh
            want = tq[h, d] * sk[h, d] * sig[:, :, q]                                  # [n, T]
            J[:, h, :, q, :] = B[:, :, (d + h) % npat, :] == want[:, :, None]
    g = int(np.log2(J.sum(-1).max()))
    # the projection
    omax = NC * co
    rs = rng.integers(-2, 3, size=co).astype(f64) if c.has_res else None
    bo = rng.integers(-8, 9, size=co).astype(f64)
    if form == "onehot3":
        wo = np.zeros((co, co))
        wo[np.arange(co), (5 * np.arange(co) + 1) % co] = 1
        bo[:] = 0
        rs = np.zeros(co) if c.has_res else None
    else:
        nnz = int(max(1, min(co, (2 ** (24 - g) - 2 * (NC + 4) - 16) // omax)))
        pos = np.argsort(rng.random((co, co)), axis=1)[:, :nnz]
        wo = np.zeros((co, co))
        np.put_along_axis(wo, pos, rng.choice((-1.0, 1.0), size=(co, nnz)), axis=1)
        z = co // 2
        wo[z], bo[z] = 0, 0
        if rs is not None:
            rs[z] = 0
    w_out, b_out = _pack(wo, bo)
    return dict(x=x.reshape(n, K, ncols).astype(f32), w_qkv=w_qkv, b_qkv=b_qkv, s_in=s_in.astype(f32), t_in=t_in.astype(f32), w_out=w_out,
                b_out=b_out, res_scale=None if rs is None else rs.astype(f32), J=J, g=g, form=form, src=(5 * np.arange(co) + 1) % co)


def round_operands(c, flavour):
    dk, dkh, dvh, M, ncols = dims(c)
    K, V, n, co = c.c_in, c.V, c.n_seg, c.c_out
    rng = _rng(c, 2, flavour == "flat")
    x = rng.uniform(-1, 1, size=(n, K, ncols))
    s_in = rng.uniform(0.5, 1.5, size=(K, V)) * rng.choice((-1.0, 1.0), size=(K, V))
    t_in = rng.uniform(-0.5, 0.5, size=(K, V))
    wr = rng.standard_normal((M, K)) * np.sqrt(1.5 / K)                  # x^ has variance of about 2 / 3: rows of O(1)
    wr[:2 * dk] *= np.sqrt({"peaked": 3.0, "flat": 0.25}[flavour]) / dkh ** 0.25
    br = rng.uniform(-0.25, 0.25, size=M)
    br[:2 * dk] *= 0.25
    w_qkv, b_qkv = _pack(wr, br)
    w_out, b_out = _pack(rng.standard_normal((co, co)) / np.sqrt(co), rng.uniform(-0.5, 0.5, size=co))
    rs = rng.uniform(0.5, 1.5, size=co).astype(f32) if c.has_res else None
    return dict(x=x.astype(f32), w_qkv=w_qkv, b_qkv=b_qkv, s_in=s_in.astype(f32), t_in=t_in.astype(f32), w_out=w_out, b_out=b_out, res_scale=rs)


# ---- references and bounds ------------------------------------------------------------------------------------------------------
def gamma(n):
    return n * U / (1 - n * U)


def qkv64(c, ops):
    """-> (qkv [n, M, ncols] fp64, bound, sum |term|)"""
    dk, dkh, dvh, M, ncols = dims(c)
    n, K, T, V = c.n_seg, c.c_in, c.frames, c.V
    xh = f64(ops["x"]).reshape(n, K, T, V) * f64(ops["s_in"])[None, :, None, :] + f64(ops["t_in"])[None, :, None, :]
    w, b = f64(ops["w_qkv"])[:, :M], f64(ops["b_qkv"])[:M]
    out = np.einsum("km,nktv->nmtv", w, xh, optimize=True) + b[None, :, None, None]
    mag = np.einsum("km,nktv->nmtv", np.abs(w), np.abs(xh), optimize=True) + np.abs(b)[None, :, None, None]
    return out.reshape(n, M, ncols), (gamma(K + 2) * mag).reshape(n, M, ncols), mag.reshape(n, M, ncols)


def _heads(c, qkv):
    dk, dkh, dvh, M, ncols = dims(c)
    n, T, V = c.n_seg, c.frames, c.V
    a = f64(qkv).reshape(n, M, T, V)
    return a[:, :dk].reshape(n, NH, dkh, T, V), a[:, dk:2 * dk].reshape(n, NH, dkh, T, V), a[:, 2 * dk:].reshape(n, NH, dvh, T, V)


def logits64(c, qkv):
    """-> (l [n, 8, T, V(i), V(j)], sum |q| |k|)"""
    q, k, v = _heads(c, qkv)
    return np.einsum("nhdti,nhdtj->nhtij", q, k), np.einsum("nhdti,nhdtj->nhtij", np.abs(q), np.abs(k))


def o64(c, qkv):
    """qkv [n, M, ncols] (taken as exact) -> (o [n, dv, ncols] fp64, bound)"""
    dk, dkh, dvh, M, ncols = dims(c)
    q, k, v = _heads(c, qkv)
    l, A = logits64(c, qkv)
    dl = (dkh + 1) * U * A
    dlmax = dl.max(-1, keepdims=True)
    d = l - l.max(-1, keepdims=True)
    dd = dl + dlmax + U * (np.abs(d) + dl + dlmax)
    e = np.exp(d)
    re = np.expm1(dd) + EXPF_REL * np.exp(dd)
    S = e.sum(-1, keepdims=True)
    R = (re * e).sum(-1, keepdims=True) / S
    rs = R + gamma(c.V - 1) * (1 + R)
    p = e / S
    rho = (1 + re) * (1 + U) ** 2 / (1 - rs) - 1
    o = np.einsum("nhtij,nhdtj->nhdti", p, v)
    bnd = np.einsum("nhtij,nhdtj->nhdti", p * (rho + gamma(c.V) * (1 + rho)), np.abs(v))
    return o.reshape(c.n_seg, c.c_out, ncols), bnd.reshape(c.n_seg, c.c_out, ncols)


def y64(c, ops, o):
    """o [n, dv, ncols] (taken as exact) -> (y fp64, bound, y before the ReLU, sum |term|)"""
    co = c.c_out
    w, b = f64(ops["w_out"])[:, :co], f64(ops["b_out"])[:co]
    pre = np.einsum("km,nkc->nmc", w, f64(o), optimize=True) + b[None, :, None]
    mag = np.einsum("km,nkc->nmc", np.abs(w), np.abs(f64(o)), optimize=True) + np.abs(b)[None, :, None]
    if ops["res_scale"] is not None:
        r = f64(ops["res_scale"])[None, :, None] * f64(ops["x"])
        pre, mag = pre + r, mag + np.abs(r)
    return np.maximum(pre, 0), gamma(co + 2) * mag, pre, mag


def is_f32(a):
    return bool(np.array_equal(f64(f32(a)), f64(a), equal_nan=True))


def admissible(c, ops):
    """every sum of every stage of an exact case: integer terms (multiples of 2^-g behind the softmax) with sum |term| < 2^24 units, the
    logits tie on 2^n keys with every other one >= 128 below, exp(-128) is 0 in fp32 and below half the smallest denormal in fp64"""
    assert float(np.exp(f32(-128))) == 0.0 and np.exp(f64(-128)) < 2.0 ** -150
    dk, dkh, dvh, M, ncols = dims(c)
    x, s, t = f64(ops["x"]).reshape(c.n_seg, c.c_in, c.frames, c.V), f64(ops["s_in"])[None, :, None, :], f64(ops["t_in"])[None, :, None, :]
    for a in (x, s, t, ops["w_qkv"], ops["b_qkv"], ops["w_out"], ops["b_out"]) + ((ops["res_scale"],) if ops["res_scale"] is not None else ()):
        assert np.array_equal(a, np.round(a))
    assert float((np.abs(x * s) + np.abs(t)).max()) < 2 ** 24
    qkv, _, mag = qkv64(c, ops)
    assert float(mag.max()) < 2 ** 24 and is_f32(qkv)
    if "J" not in ops:
        return
    l, A = logits64(c, qkv)
    assert float(A.max()) < 2 ** 24
    top = l.max(-1, keepdims=True)
    tie = l == top
    assert float((top - np.where(tie, -np.inf, l)).min()) >= 128
    cnt = tie.sum(-1)
    assert np.array_equal(cnt & (cnt - 1), np.zeros_like(cnt)) and int(cnt.max()) == 2 ** ops["g"]
    q, k, v = _heads(c, qkv)
    assert float(np.einsum("nhtij,nhdtj->nhdti", f64(tie), np.abs(v)).max()) < 2 ** 24
    o, _ = o64(c, qkv)
    unit = 2.0 ** -ops["g"]
    assert np.array_equal(o / unit, np.round(o / unit)) and is_f32(o)
    y, _, pre, mag = y64(c, ops, o)
    assert float(mag.max()) / unit < 2 ** 24 and is_f32(y)
    assert ops["form"] != "designed" or ((pre < 0).any() and (pre == 0).any() and (pre > 0).any())


# ---- an op-for-op fp32 host model of the three launches, with seeded defects -----------------------------------------------------------
DEFECTS = {
    1: ("drop_last_chunk", "chunk_twice", "sv_tile_local", "no_shift", "bias_next_row", "store_row_ge_M", "store_surplus_col", "swap_halves_mi4"),
    2: ("k_next_head", "v_offset_dk", "frame_wrong_seg", "no_norm", "exp_rel_2^-18"),
    3: ("res_scale_by_col", "res_y_strides", "no_relu", "bias_after_relu"),
}


def _fma(a, b, c_):
    return f32(f64(a) * f64(b) + f64(c_))


def model_gemm(src, s_st, w, bias, K, M, ncols, V, n_seg, mi, dst, d_st, affine=None, res=None, relu=False, defect=None):
    """str_gemm_kernel on flat buffers: src rows at seg s_st[0] + k s_st[1] + col, dst likewise.  Tiles of 32 mi rows x 256 columns, 16-row
    chunks, the staging column clamped into the row, rows >= M and columns >= ncols not stored.  affine = (s_in, t_in) [K][V];
    res = (flat, strides, res_scale).  Writes dst in place."""
    MTl, Mp = 32 * mi, w.shape[1]
    mtiles, ctiles, nk = Mp // MTl, -(-ncols // NT), K // KC
    tid = np.arange(NT)
    for seg in range(n_seg):
        for ct in range(ctiles):
            col0 = ct * NT
            scol = np.minimum(col0 + tid, ncols - 1)
            sv = (tid if defect == "sv_tile_local" else scol) % V
            for mt in range(mtiles):
                m0 = mt * MTl
                acc = np.zeros((MTl, NT), dtype=f32)
                for kc in range(nk - 1 if defect == "drop_last_chunk" else nk):
                    k0 = (0 if defect == "chunk_twice" and kc == 1 else kc) * KC
                    rows = k0 + np.arange(KC)
                    X = src[seg * s_st[0] + rows[:, None] * s_st[1] + scol[None, :]]
                    if affine is not None:
                        sh = affine[1][rows[:, None], sv[None, :]]
                        X = _fma(X, affine[0][rows[:, None], sv[None, :]], np.zeros_like(sh) if defect == "no_shift" else sh)
                    acc = (acc + w[rows, m0:m0 + MTl].T @ X).astype(f32)
                m = m0 + np.arange(MTl)
                if defect == "swap_halves_mi4" and mi == 4:
                    acc = np.roll(acc, 64, axis=0)
                bm = np.minimum(m + 1, Mp - 1) if defect == "bias_next_row" else m
                val = acc if defect == "bias_after_relu" else (acc + bias[bm][:, None]).astype(f32)
                col = col0 + tid
                rowok = np.ones(MTl, bool) if defect == "store_row_ge_M" else m < M
                colok = np.ones(NT, bool) if defect == "store_surplus_col" else col < ncols
                mm, cc = np.minimum(m, M - 1), np.minimum(col, ncols - 1)
                if res is not None:
                    rflat, r_st, rscale = res
                    if defect == "res_y_strides":
                        r_st = d_st
                    ridx = np.minimum(seg * r_st[0] + mm[:, None] * r_st[1] + cc[None, :], rflat.size - 1)
                    sc = rscale[np.minimum(col, M - 1)][None, :] if defect == "res_scale_by_col" else rscale[mm][:, None]
                    val = _fma(np.broadcast_to(sc, val.shape), rflat[ridx], val)
                if relu and defect != "no_relu":
                    val = np.where(np.isnan(val), val, np.maximum(val, f32(0)))
                if defect == "bias_after_relu":
                    val = (val + bias[bm][:, None]).astype(f32)
                idx = seg * d_st[0] + m[:, None] * d_st[1] + col[None, :]
                ok = rowok[:, None] & colok[None, :] & (idx < dst.size)
                dst[idx[ok]] = val[ok]


def model_attention(c, qkv, defect=None):
    """str_attention_kernel: qkv [n, M, ncols] fp32 -> o [n, dv, ncols] fp32, the operations in the kernel's order"""
    dk, dkh, dvh, M, ncols = dims(c)
    n, T, V = c.n_seg, c.frames, c.V
    a = np.asarray(qkv, dtype=f32).reshape(n, M, T, V)
    if defect == "frame_wrong_seg":
        a = np.roll(a, -1, axis=0)
    q, k = a[:, :dk].reshape(n, NH, dkh, T, V), a[:, dk:2 * dk].reshape(n, NH, dkh, T, V)
    v0 = dk if defect == "v_offset_dk" else 2 * dk
    v = a[:, v0:v0 + c.c_out].reshape(n, NH, dvh, T, V)
    if defect == "k_next_head":
        k = np.roll(k, -1, axis=1)
    l = np.zeros((n, NH, T, V, V), dtype=f32)
    for d in range(dkh):
        l = _fma(q[:, :, d, :, :, None], k[:, :, d, :, None, :], l)
    e = np.exp((l - l.max(-1, keepdims=True)).astype(f32)).astype(f32)
    if defect == "exp_rel_2^-18":                   # a j-uniform relative error cancels in the normalisation: the sign follows the
        sgn = np.where(v[:, :, 0] >= 0, 1, -1)      # head's first v row at the key
        e = (e * (1 + 2.0 ** -18 * sgn[:, :, :, None, :])).astype(f32)
    s = np.zeros(e.shape[:-1], dtype=f32)
    for j in range(V):
        s = (s + e[..., j]).astype(f32)
    p = e if defect == "no_norm" else (e * (f32(1) / s)[..., None]).astype(f32)
    o = np.zeros((n, NH, dvh, T, V), dtype=f32)
    for j in range(V):
        o = _fma(p[:, :, None, :, :, j], v[:, :, :, :, None, j], o)
    return o.reshape(n, c.c_out, ncols)


def scratch_floats(c):
    dk, dkh, dvh, M, ncols = dims(c)
    return c.n_seg * (M + c.c_out) * ncols


def model_stage(c, ops, stage, defect=None, qkv=None, o=None):
    """one launch of the unit on NaN-filled flat buffers -> the flat image of the stage: 1 and 2 the whole scratch (qkv resp. o given as
    [n, rows, ncols] inputs of stage 2 / 3), 3 the y buffer"""
    dk, dkh, dvh, M, ncols = dims(c)
    xs, ys = xy_strides(c)
    n = c.n_seg
    if stage == 1:
        scratch = np.full(scratch_floats(c), np.nan, dtype=f32)
        model_gemm(place(ops["x"], xs), xs, ops["w_qkv"], ops["b_qkv"], c.c_in, M, ncols, c.V, n, select(c)[0], scratch, (M * ncols, ncols),
                   affine=(ops["s_in"], ops["t_in"]), defect=defect)
        return scratch
    if stage == 2:
        scratch = np.full(scratch_floats(c), np.nan, dtype=f32)
        scratch[: n * M * ncols] = np.asarray(qkv, dtype=f32).reshape(-1)
        scratch[n * M * ncols:] = model_attention(c, qkv, defect).reshape(-1)
        return scratch
    y = np.full(body(n, c.c_out, ncols, ys), np.nan, dtype=f32)
    res = None if ops["res_scale"] is None else (place(ops["x"], xs), xs, ops["res_scale"])
    model_gemm(np.asarray(o, dtype=f32).reshape(-1), (c.c_out * ncols, ncols), ops["w_out"], ops["b_out"], c.c_out, c.c_out, ncols, c.V, n, 2,
               y, ys, res=res, relu=True, defect=defect)
    return y


def expected_image(c, stage, ref, bnd=None, qkv=None):
    """the flat image model_stage / the device must hold: (values with NaN wherever nothing belongs, bound with 0 there)"""
    dk, dkh, dvh, M, ncols = dims(c)
    n = c.n_seg
    bnd = np.zeros_like(ref) if bnd is None else bnd
    if stage == 3:
        ys = xy_strides(c)[1]
        return place(f64(ref), ys, dtype=f64), place(f64(bnd), ys, 0.0, dtype=f64)
    want, b = np.full(scratch_floats(c), np.nan), np.zeros(scratch_floats(c))
    if stage == 1:
        want[: n * M * ncols], b[: n * M * ncols] = f64(ref).reshape(-1), f64(bnd).reshape(-1)
    else:
        want[: n * M * ncols] = f64(qkv).reshape(-1)
        want[n * M * ncols:], b[n * M * ncols:] = f64(ref).reshape(-1), f64(bnd).reshape(-1)
    return want, b


def worst(got, want, bnd):
    """largest err / bound over a flat image; inf where finiteness differs (a missing or a surplus store) or a zero bound is missed"""
    got, miss = f64(got), np.isnan(want)
    if not np.array_equal(np.isfinite(got), ~miss):
        return float("inf")
    err = np.abs(got[~miss] - want[~miss])
    b = bnd[~miss]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0
