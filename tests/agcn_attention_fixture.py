"""Cases, operands, the fp64 reference and the error bound shared by tests/test_gpu_agcn_attention.py and
tests/test_agcn_attention_fixture_cpu.py: the A-GCN adaptive adjacency (csrc/agcn.hip; models/a_gcn/a_gcn.py:53-63)

    adj[n][i][v, w] = softmax over v of ( sum_{k, t} Ea_i[k, t, v] Eb_i[k, t, w] / (inter T) ) + a_sum[i][v, w]

written as ell_val[n][i][w][v].  csk_agcn_attention_f32 reads the embeddings E (channels i inter + k = a_i, (3 + i) inter + k = b_i);
csk_agcn_embed_attention_f32 forms them itself, E = W x + b, rows in pair-major order.

Operands.  E is integer valued with |E| <= 2: every logit sum S is an integer with |S| <= 4 K, K = inter T <= 2^22 / 4, exact in fp32
in any summation order (admissible() asserts sum |term| < 2^24), and the logits lie in [-4, 4]: a span of at most 8.  For the fused
entry x is in {-1, 0, 1} and a weight row has two entries +-1 (bias 0) or one entry +-1 and a bias in {-1, 0, 1}, so that E is
again an integer with |E| <= 2 and exact.  a_sum is uniform in [-0.5, 0.5).

The bound, per element, with u = 2^-24, l the exact logit, Lmax = max |l|, span = max l - min l of the column, p the exact softmax:
  * lg = fl(S / K), or S * fl(1 / inter) in the step forms: two roundings at most, |lg - l| <= 2 u Lmax =: dl
  * d = fl(lg - max lg): |d - exact| <= 2 dl + u span =: dd
  * e = sm_exp(d): the header of agcn.hip states a relative error <= |d| 2^-23 = 2 u span; one more ulp (2 u) is allowed for the
    hardware exponential's own rounding; the error of d passes through as a relative error dd:  re = 2 u span + 2 u + dd
  * the column sum of V positive terms: relative error <= re + (V - 1) u;  sm_rcp: u;  the product e * rs: u
    => relative error of the softmax value  rho = 2 re + (V + 1) u, plus 2 u for the second-order terms
  * the final add: u |p + a_sum|
    bound = rho p + u (p + |a_sum|)
It is derived, not measured.  At V = 32 and a span of 8 rho is about 120 u = 7e-6.  The peaked-attention test of
tests/test_gpu_agcn_parity.py covers large spans.  numpy only; nothing is read from csrc."""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
f32, f64 = np.float32, np.float64
CPAD, MTPAD = 16, 64

# ---- csk_agcn_attention_f32 -----------------------------------------------------------------------------------------------------
# clip form: E (n, 6 inter, T, V) with e_chan_stride = T V + chan_pad; `off` floats off 16-byte alignment (rows 4-byte aligned)
Att = namedtuple("Att", "name n inter T V chan_pad off")
ATT_CLIP = [Att(f"att-T{T}-i{inter}-V{V}", n, inter, T, V, pad, off) for T, inter, V, n, pad, off in (
    (1, 16, 25, 3, 0, 0), (2, 3, 18, 2, 1, 1), (63, 6, 18, 2, 0, 1), (64, 3, 25, 2, 3, 0), (65, 16, 31, 2, 0, 1), (130, 6, 32, 2, 1, 1),
    (130, 20, 18, 2, 0, 0), (65, 20, 25, 3, 2, 1), (2, 16, 2, 3, 0, 1), (64, 6, 31, 2, 0, 0), (63, 3, 32, 2, 1, 0), (1, 20, 18, 5, 0, 1))]
# step form: `groups` channel-major frames (6 inter, P) of `spg` skeletons each, P = spg V + 3 rounded up to 4; a gap between groups
Step = namedtuple("Step", "name groups spg inter V group_pad")
ATT_STEP = [Step("step-3x3-i16-V25", 3, 3, 16, 25, 8), Step("step-2x5-i6-V18", 2, 5, 6, 18, 4), Step("step-1x7-i20-V32", 1, 7, 20, 32, 0),
            Step("step-5x1-i3-V2", 5, 1, 3, 2, 12)]

# ---- csk_agcn_embed_attention_f32: agcn_embed_attention_kernel<INTER, NP, V, CLIP>, 128 / V frames per tile ----------------------
Emb = namedtuple("Emb", "name n c_in inter frames V per_frame x_pad")
FT = {18: 7, 25: 5}


def _emb_cases():
    out, k = [], 0
    for inter in (16, 32, 64):
        for V in (18, 25):
            for per_frame in (1, 0):
                for fi, fr in enumerate((1, FT[V], FT[V] + 1, 3 * FT[V] + 2)):
                    c_in = (3, 16, 40)[(fi + k) % 3]
                    out.append(Emb(f"emb-i{inter}-V{V}-{'frame' if per_frame else 'clip'}-T{fr}-ci{c_in}", 2 + k % 2, c_in, inter, fr, V, per_frame,
                                   (0, 2)[k % 2] if V == 18 else (0, 1)[k % 2]))
                k += 1
    return out


EMB_CASES = _emb_cases()


def instantiation(c):
    """(INTER, NP, V, CLIP) of the kernel a fused case runs: three pairs per workgroup at inter 16, one otherwise"""
    return c.inter, 3 if c.inter == 16 else 1, c.V, not c.per_frame


def cpad(c):
    return -(-c // CPAD) * CPAD


def mpad(m):
    return -(-m // MTPAD) * MTPAD


# ---- operands -------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(np.random.SeedSequence([int(k) for k in key]))


def a_sum_of(rng, V):
    return (rng.random((3, V, V), dtype=f32) - f32(0.5)).astype(f32)


def att_operands(n, inter, T, V, seed):
    """-> E [n, 6 inter, T, V] integers in [-2, 2], a_sum [3, V(v), V(w)]"""
    rng = _rng(11, n, inter, T, V, seed)
    return rng.integers(-2, 3, size=(n, 6 * inter, T, V)).astype(f32), a_sum_of(rng, V)


def emb_operands(c):
    """-> x [n, c_in, frames, V] in {-1, 0, 1}; w [6 inter, c_in], b [6 inter] in the order of E's channels (a_0, a_1, a_2, b_0, b_1, b_2);
    a_sum"""
    rng = _rng(13, c.n, c.c_in, c.inter, c.frames, c.V, c.per_frame)
    x = rng.integers(-1, 2, size=(c.n, c.c_in, c.frames, c.V)).astype(f32)
    rows = 6 * c.inter
    w, b = np.zeros((rows, c.c_in), dtype=f32), np.zeros(rows, dtype=f32)
    for r in range(rows):
        ch = rng.choice(c.c_in, size=2, replace=False)
        w[r, ch[0]] = rng.choice((-1, 1))
        if r % 2:
            w[r, ch[1]] = rng.choice((-1, 1))
        else:
            b[r] = rng.integers(-1, 2)
    return x, w, b, a_sum_of(rng, c.V)


def embed(x, w, b):
    """E = W x + b, [n, rows, frames, V], exact in fp64"""
    return np.einsum("rc,nctv->nrtv", f64(w), f64(x)) + f64(b)[None, :, None, None]


def pair_major(w, b, inter):
    """E's channel order -> the fused entry's packed image [c_in_pad][rows_pad], rows i 2 inter + k = a_i[k], i 2 inter + inter + k = b_i[k]"""
    rows, c_in = w.shape
    order = [h * 3 * inter + i * inter + k for i in range(3) for h in (0, 1) for k in range(inter)]
    img = np.zeros((cpad(c_in), mpad(rows)), dtype=f32)
    img[:c_in, :rows] = w[order].T
    bias = np.zeros(mpad(rows), dtype=f32)
    bias[:rows] = b[order]
    return img, bias


def conv_image(w, b):
    """the same weights as csk_conv1x1_f32 takes them: [1][c_in_pad][rows_pad] in E's channel order"""
    rows, c_in = w.shape
    img = np.zeros((cpad(c_in), mpad(rows)), dtype=f32)
    img[:c_in, :rows] = w.T
    bias = np.zeros(mpad(rows), dtype=f32)
    bias[:rows] = b
    return img, bias


# ---- reference and bound --------------------------------------------------------------------------------------------------------
def logits_sum(E, inter):
    """E [n, 6 inter, T, V] -> (S [n, 3, V(v), V(w)] = sum_{k, t} Ea Eb, sum |term|), fp64"""
    E = f64(E)
    n, _, T, V = E.shape
    ea, eb = E[:, : 3 * inter].reshape(n, 3, inter, T, V), E[:, 3 * inter:].reshape(n, 3, inter, T, V)
    return np.einsum("niktv,niktw->nivw", ea, eb), np.einsum("niktv,niktw->nivw", np.abs(ea), np.abs(eb))


def reference(E, a_sum, inter, K=None):
    """-> (ell_val [n, 3, V(w), V(v)] fp64, bound of the same shape)"""
    S, _ = logits_sum(E, inter)
    K = inter * E.shape[2] if K is None else K
    l = S / K
    d = l - l.max(axis=2, keepdims=True)
    e = np.exp(d)
    p = e / e.sum(axis=2, keepdims=True)
    V = E.shape[3]
    lmax = np.abs(l).max(axis=2, keepdims=True)
    span = -d.min(axis=2, keepdims=True)
    dl = 2 * U * lmax
    dd = 2 * dl + U * span
    re = 2 * U * span + 2 * U + dd
    rho = 2 * re + (V + 1) * U + 2 * U
    a = f64(a_sum)[None]
    bnd = rho * p + U * (p + np.abs(a))
    return np.swapaxes(p + a, 2, 3), np.broadcast_to(np.swapaxes(bnd, 2, 3), (E.shape[0], 3, V, V))


def per_frame_view(E):
    """[n, C, frames, V] -> [n frames, C, 1, V]: every frame a sample of its own (T = 1)"""
    n, C, T, V = E.shape
    return np.ascontiguousarray(np.transpose(E, (0, 2, 1, 3))).reshape(n * T, C, 1, V)


def admissible(E, inter):
    """integer embeddings, every logit sum below 2^24 in any order, spans of at most 8"""
    assert np.array_equal(E, np.round(E)) and float(np.abs(E).max()) <= 2
    S, mag = logits_sum(E, inter)
    assert float(mag.max()) < 2 ** 24
    l = S / (inter * E.shape[2])
    assert float((l.max(axis=2) - l.min(axis=2)).max()) <= 8.0
    return float((l.max(axis=2) - l.min(axis=2)).max())


# ---- a plain fp32 model with seeded defects -------------------------------------------------------------------------------------
DEFECTS = ("transposed", "next_subset", "next_segment", "wrong_divisor", "lost_k_row")


def model_f32(E, a_sum, inter, defect=None):
    """softmax(Ea^T Eb / K) + a_sum in plain fp32 with ONE defect: the output written [v][w] instead of [w][v]; pair i + 1 for i;
    the next sample's embeddings; a divisor of inter (T forgotten; inter + 1 at T = 1); the last (k, t) row left out of the logits"""
    E = np.asarray(E, dtype=f32)
    n, _, T, V = E.shape
    if defect == "next_segment":
        E = np.roll(E, -1, axis=0)
    ea, eb = E[:, : 3 * inter].reshape(n, 3, inter, T, V), E[:, 3 * inter:].reshape(n, 3, inter, T, V)
    if defect == "next_subset":
        ea, eb = np.roll(ea, -1, axis=1), np.roll(eb, -1, axis=1)
    S = np.einsum("nikv,nikw->nivw", ea.reshape(n, 3, inter * T, V), eb.reshape(n, 3, inter * T, V)).astype(f32)
    if defect == "lost_k_row":
        S = S - np.einsum("niv,niw->nivw", ea[:, :, -1, -1], eb[:, :, -1, -1]).astype(f32)
    K = f32(inter * T)
    if defect == "wrong_divisor":
        K = f32(inter if T > 1 else inter + 1)
    l = (S / K).astype(f32)
    e = np.exp((l - l.max(axis=2, keepdims=True)).astype(f32)).astype(f32)
    p = (e * (f32(1) / e.sum(axis=2, keepdims=True, dtype=f32))).astype(f32)
    out = (p + a_sum[None]).astype(f32)
    return out if defect == "transposed" else np.swapaxes(out, 2, 3)
