"""Cases, operands, fp64 references and the error bound shared by tests/test_gpu_head_kernels.py and tests/test_head_fixture_cpu.py.

The kernels either side of the block stack (csrc/head.hip, and the spatial pool and window mean of csrc/step.hip) are sums with a
divide, a scale or a bias at the end, and one fma per element for the input permute + data_bn.  Two tiers of operands pin them:

exact tier   small signed integers.  Every partial sum, in any order, is an integer (or a dyadic with a fixed denominator) below
             2^24, so the fp32 result does not depend on the summation order and the expected BITS follow from the exact sum: a
             pool is fp32(fp32(S) / fp32(divisor)) * fp32(scale), an FC is the integer sum itself.  The continual head's rows
             are a constant k plus a zero-sum permutation, which makes the spatial mean exactly k, the window mean (window a
             power of two) an exact dyadic and the FC exact again.
float tier   uniform in [0.5, 1.5): every term is positive, so a lost or doubled term cannot cancel.  The result is compared with
             fp64 under bound() = (n_terms + 4) * 2^-24 * sum |term_i|: recursive fp32 summation in ANY order is within
             (n - 1) u sum |a_i| of the exact sum, the + 4 leaves room for the divide, the scale and the bias add.  The bound is
             derived, not measured; it is smaller than half of the smallest term as long as n_terms <= 600 (margin()), so a
             dropped, doubled or misplaced term fails.  Larger shapes are exact tier only.

The references are written from the operations' definitions (models/st_gcn/st_gcn.py:49-64, models/base.py:73-101); nothing is
read from csrc.  numpy only; check_bound alone borrows the report path of tests/helpers.py when it is called."""
import json
import os

import numpy as np

U = 2.0 ** -24                 # unit roundoff of fp32
MAX_FLOAT_TERMS = 600

# ---- case tables ------------------------------------------------------------------------------------------------------------
POOL_TV = (1, 63, 64, 65, 75, 449, 480, 511, 512, 513, 1025, 1875)      # csk_pool_fc_f32 (logits = NULL), csk_pool_scaled_f32
POOL_M = (1, 2, 3)
POOL_NC = ((1, 1), (3, 5), (2, 7))
POOL_SCALES = (1.0, 0.75)
POOL_FLOAT_TV = (64, 75, 150)
POOL_FLOAT_M = 2
POOL_FC_CASE = dict(n=2, m=2, c=8, tv=50, classes=5)                    # csk_pool_fc_f32 with logits, exact

FC_C = (1, 3, 4, 5, 70, 256)                                            # csk_fc_f32, both tiers
FC_CLASSES = (1, 60, 63, 64, 65, 400)
FC_N = (1, 3)

SPATIAL_MV = (1, 36, 50, 64, 65, 130)                                   # csk_co_spatial_pool_f32
SPATIAL_NC = ((3, 5), (2, 7))
WINDOWS = (1, 2, 4, 9, 10, 17, 75)                                      # csk_co_window_mean_f32
WINDOW_ELEMS = 2 * 133                                                  # n_elem of the ring: more than one 256-thread block

# csk_co_head_step_f32: (n, C, MV, classes, window)
HEAD_EXACT = ((2, 256, 50, 60, 16), (3, 70, 36, 11, 4), (1, 65, 50, 65, 8), (2, 516, 18, 3, 16))
HEAD_FLOAT = ((2, 64, 50, 60, 10), (1, 70, 36, 400, 17), (2, 256, 25, 7, 75))

# csk_input_norm_f32: (N, C, T, V, M)
NORM_DENSE = ((2, 3, 5, 25, 2), (1, 2, 7, 18, 1), (3, 4, 1, 25, 3))
NORM_STRIDED = (2, 3, 5, 25, 2)                                         # h_chan_stride = T V + 4, h_seg_stride = C h_chan_stride + 8
NORM_LARGE = (48, 3, 300, 25, 2)                                        # 2.16 M elements: more than the 8192 x 256 threads of a launch
NORM_GRID_THREADS = 8192 * 256
FRAMES_R = (1, 3, 8)                                                    # csk_input_norm_frames_f32
FRAMES_SHAPES = ((2, 3, 25, 2), (1, 4, 18, 1))                          # (N, C, V, M)
WRAPPER_SHAPE = (3, 8, 25, 2)                                           # StGcn input_shape (C, T, V, M) of the wrapper cases
WRAPPER_N = 2

INT_AMP = 3        # exact tier: activations, features and weights are integers in [-INT_AMP, INT_AMP]
K_AMP = 4          # exact tier, rows with an exact mean: the mean is an integer in [-K_AMP, K_AMP]
BIAS_AMP = 8       # exact tier: integer bias in [-BIAS_AMP, BIAS_AMP]


def head_steps(window):
    """The steps of one continual-head case: (step, head, count, emit, zero) for 2 window + 3 steps -- a filling window, a full
    one and two wraps -- with one zero feature (h = NULL, the window's end padding) on the way and every fifth step silent."""
    out = []
    for step in range(2 * window + 3):
        out.append((step, step % window, min(step + 1, window), int(step % 5 != 2), step == window + 1))
    return out


def window_states(window):
    """(head, count) of a pooling window that fills, is full and wraps twice"""
    return [(step % window, min(step + 1, window)) for step in range(2 * window + 3)]


def frames_p(n, m, v):
    """row length of a channel-major frame: N M V rounded up to a multiple of 4, plus 8 columns no kernel may touch"""
    return (n * m * v + 3) // 4 * 4 + 8


def spatial_p(n, mv):
    """row length of the spatial-pool frames: N MV rounded up to a multiple of 4, and strictly more than N MV"""
    return (n * mv + 4) // 4 * 4


# ---- operands ---------------------------------------------------------------------------------------------------------------
def exact_operand(rng, shape, amp=INT_AMP):
    """exact tier: integers in [-amp, amp] as fp32"""
    return rng.integers(-amp, amp + 1, size=shape).astype(np.float32)


def float_operand(rng, shape):
    """float tier: uniform in [0.5, 1.5) as fp32"""
    return (rng.random(size=shape, dtype=np.float32) + np.float32(0.5)).astype(np.float32)


def zero_sum(n):
    """n distinct-magnitude integers that sum to zero: +-1 .. +-(n // 2), and a 0 when n is odd"""
    half = np.arange(1, n // 2 + 1)
    return np.concatenate([half, -half, np.zeros(n % 2, dtype=half.dtype)]).astype(np.float32)


def exact_mean_rows(rng, rows, n):
    """exact tier rows with an exact mean: (k [rows], x [rows, n]) with x[r] = k[r] + a permutation of zero_sum(n), so that
    sum(x[r]) = n k[r] and the mean is the integer k[r] whatever the order of the sum"""
    k = rng.integers(-K_AMP, K_AMP + 1, size=rows).astype(np.float32)
    z = zero_sum(n)
    x = np.stack([k[r] + rng.permutation(z) for r in range(rows)]).astype(np.float32)
    return k, x


def head_operands(tier, n, c, mv, classes, window, seed):
    """One continual-head case -> (w [classes, c], b [classes], frames): a channel-major frame [c, P] per step of
    head_steps(window), None for the zero feature.  The columns from n mv on are NaN: a read past a stream's positions poisons
    the sum.  Exact tier: every (row, stream) is exact_mean_rows, weights and bias are integers."""
    rng = np.random.default_rng(seed)
    p = spatial_p(n, mv)
    if tier == "exact":
        w, b = exact_operand(rng, (classes, c)), exact_operand(rng, (classes,), BIAS_AMP)
    else:
        w, b = float_operand(rng, (classes, c)), float_operand(rng, (classes,))
    frames = []
    for _, _, _, _, zero in head_steps(window):
        if zero:
            frames.append(None)
            continue
        h = np.full((c, p), np.nan, dtype=np.float32)
        if tier == "exact":
            h[:, : n * mv] = exact_mean_rows(rng, c * n, mv)[1].reshape(c, n * mv)
        else:
            h[:, : n * mv] = float_operand(rng, (c, n * mv))
        frames.append(h)
    return w, b, frames


# ---- fp64 references --------------------------------------------------------------------------------------------------------
def f64(a):
    return np.asarray(a, dtype=np.float64)


def ref_pool_sum(h, n, m):
    """h [(n m), c, tv] -> S [n, c]: the sum over the m bodies and the tv positions of sample n, channel c"""
    nm, c, tv = h.shape
    assert nm == n * m
    return np.einsum("nmcp->nc", f64(h).reshape(n, m, c, tv))


def ref_pool(h, n, m, scale=1.0):
    """mean over (m, tv), times scale (models/st_gcn/st_gcn.py:60-63)"""
    return ref_pool_sum(h, n, m) / (m * h.shape[2]) * float(np.float32(scale))


def exact_pool_bits(s, divisor, scale=1.0):
    """exact tier: the fp32 value of a pool whose exact integer sum is s: fp32(fp32(s) / fp32(divisor)) * fp32(scale), both
    operations correctly rounded"""
    s = np.asarray(s)
    assert np.all(np.abs(s) < 2 ** 24) and np.all(s == np.round(s))
    return (s.astype(np.float32) / np.float32(divisor)) * np.float32(scale)


def ref_fc(feat, w, b):
    """logits [n, k] = sum_c feat[n, c] w[k, c] + b[k]"""
    return np.einsum("nc,kc->nk", f64(feat), f64(w)) + f64(b)[None, :]


def ref_spatial_sum(h, n, mv):
    """channel-major frame h [c, P] -> S [n, c]: the sum of the mv positions [n mv, (n + 1) mv) of row c"""
    c = h.shape[0]
    return np.einsum("cnp->nc", f64(h)[:, : n * mv].reshape(c, n, mv))


def ref_window_sum(ring, head, count, window):
    """ring [window, ...] -> the sum of the `count` newest entries, the newest in slot `head` (co.AvgPool1d over a
    zero-initialised window: the caller divides by `window`, not by `count`)"""
    assert ring.shape[0] == window and 0 <= head < window and 0 <= count <= window
    s = np.zeros(ring.shape[1:], dtype=np.float64)
    for age in range(count):
        s += f64(ring[(head - age) % window])
    return s


def fma_f32(x, scale, shift):
    """fp32(x * scale + shift) with ONE rounding, for fp32 operands: the product is exact in fp64, the sum is split into its fp64
    value r and the exact remainder e (two-sum); fp32(r) is the answer unless r sits exactly half way between two fp32 values
    and e is not zero, where e decides."""
    x, scale, shift = (np.asarray(a, dtype=np.float32) for a in (x, scale, shift))
    p = f64(x) * f64(scale)
    t = f64(shift) + np.zeros_like(p)
    r = p + t
    bb = r - p
    e = (p - (r - bb)) + (t - bb)
    r32 = r.astype(np.float32)
    d = r - f64(r32)                                                    # exact
    toward = np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    nb = np.nextafter(r32, toward)
    tie = (d != 0) & (2 * np.abs(d) == np.abs(f64(nb) - f64(r32)))
    return np.where(tie & (e != 0) & (np.sign(e) == np.sign(d)), nb, r32).astype(np.float32)


def norm_channel(c_dim, v_dim, m, v, c):
    """data_bn channel of body m, joint v, coordinate c: the position in the (M, V, C) order of st_gcn.py:50"""
    return (m * v_dim + v) * c_dim + c


def ref_input_norm(x, scale, shift, combine=fma_f32):
    """x [N, C, T, V, M], per-channel scale / shift [M V C] -> [N M, C, T, V] (st_gcn.py:49-57: permute to (N, M V C, T), one
    affine map per channel, back to (N M, C, T, V))"""
    n, c, t, v, m = x.shape
    y = np.transpose(x, (0, 4, 3, 1, 2)).reshape(n, m * v * c, t)
    y = combine(y, np.asarray(scale)[None, :, None], np.asarray(shift)[None, :, None])
    return np.ascontiguousarray(np.transpose(y.reshape(n, m, v, c, t), (0, 1, 3, 4, 2))).reshape(n * m, c, t, v)


def ref_input_norm_frame(x, scale, shift, p, fill=np.nan):
    """one continual frame x [N, C, V, M] -> channel-major [C, P]: column (n M + m) V + v of row c (models/base.py:73-82); the
    columns from N M V on keep `fill`"""
    n, c, v, m = x.shape
    y = ref_input_norm(x[:, :, None], scale, shift)                     # [N M, C, 1, V]
    out = np.full((c, p), fill, dtype=np.float32)
    out[:, : n * m * v] = np.transpose(y[:, :, 0], (1, 0, 2)).reshape(c, n * m * v)
    return out


def distinct_affine(rng, channels):
    """scale / shift with a value of their own for every channel (a permuted channel index cannot pass): random fp32"""
    scale = (0.5 + np.arange(channels) / channels + rng.random(channels) / (4 * channels)).astype(np.float32)
    shift = (rng.standard_normal(channels) + np.arange(channels) * 0.125).astype(np.float32)
    assert len(set(scale.tolist())) == channels and len(set(shift.tolist())) == channels
    return scale, shift


# ---- the derived bound ------------------------------------------------------------------------------------------------------
def bound(abs_term_sum, n_terms):
    """(n_terms + 4) 2^-24 sum |term_i|, per output, in fp64"""
    return (n_terms + 4) * U * f64(abs_term_sum)


def margin(terms):
    """terms [..., n_terms] of a float-tier output -> (n_terms, min |term|, bound): a zero term (the window's zero feature) adds
    nothing to the sum and is not looked at"""
    a = np.abs(f64(terms))
    n = a.shape[-1]
    return n, float(np.where(a > 0, a, np.inf).min()), float(bound(a.sum(-1), n).max())


def check_bound(got, want64, bnd, **info):
    """assert |got - want64| <= bnd element by element (a NaN fails) and append {test, worst err / bound, n_terms, ...} to the
    parity report of tests/helpers.py"""
    assert "n_terms" in info, "a float-tier check records its n_terms"
    got, want64 = f64(got), f64(want64)
    bnd = np.broadcast_to(f64(bnd), want64.shape)
    assert got.shape == want64.shape, (got.shape, want64.shape, info)
    err = np.abs(got - want64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    if np.isnan(err).any():
        worst = float("inf")
    from tests.helpers import _report_path
    path = _report_path()
    if path:
        try:
            with open(path, "a") as f:
                f.write(json.dumps(dict(test=os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], kind="derived_bound",
                                        worst_err_over_bound=worst, outputs=int(want64.size),
                                        **{k: (v if isinstance(v, (int, float, str, bool)) else str(v)) for k, v in info.items()})) + "\n")
        except OSError:
            pass
    assert bool(np.all(err <= bnd)), f"worst err / bound = {worst:.3g} {info}"
    return worst
