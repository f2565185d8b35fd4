"""The kernels either side of the block stack against references of their own: csrc/head.hip (input permute + data_bn, clip pool,
FC, the continual head in one launch) and the spatial pool and window mean of csrc/step.hip.  Cases, operands, fp64 references
and the error bound come from tests/head_fixture.py: the exact tier (integer operands, order-independent sums) is compared bit for
bit, the float tier (positive terms) against fp64 under the derived bound (n_terms + 4) 2^-24 sum |term_i|, which
tests/test_head_fixture_cpu.py shows to be smaller than half of any term.  Every launch goes through the C ABI; every output lies
inside a NaN-filled buffer whose bands on either side must still be NaN afterwards, and every input lies between NaN bands, so a
read outside an operand poisons a sum."""
import ctypes

import numpy as np
import pytest
import torch

import _bootstrap
from tests import head_fixture as fx

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
DEV = "cuda:0"
PAD = 64                      # floats in a guard band: a multiple of 4, so that the tensor inside is 16-byte aligned
SENTINEL = -777.0
f32 = np.float32


class Guarded:
    """A float32 device tensor of ``shape`` in the middle of a NaN-filled buffer (``offset`` floats further in: offset = 1 gives
    a tensor that is only 4-byte aligned).  Without ``data`` the tensor itself is NaN as well: an output nobody wrote shows."""

    def __init__(self, shape, data=None, offset=0):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD + offset,), float("nan"), device=DEV, dtype=torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.n = PAD + offset, n
        self.t = self.buf[self.lo: self.lo + n].view(tuple(shape))
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=f32).reshape(tuple(shape))))

    def ptr(self):
        return native.ptr(self.t)

    def numpy(self):
        return self.t.cpu().numpy()

    def assert_bands(self):
        b = self.buf.cpu().numpy()
        assert np.isnan(b[: self.lo]).all() and np.isnan(b[self.lo + self.n:]).all(), "a guard band was written"


def _stream():
    return native.stream_of(torch.empty(1, device=DEV))


def _same_bits(got, want, what):
    want = np.asarray(want)
    assert np.array_equal(want.astype(f32).astype(np.float64), want.astype(np.float64)), ("expected value is no fp32", what)
    assert np.array_equal(got, want.astype(f32)), what


# ---- clip pool ----------------------------------------------------------------------------------------------------------------
def _pool_both_entries(lib, stream, hd, n, m, c, tv):
    """csk_pool_fc_f32 with logits = NULL (scale 1) and csk_pool_scaled_f32 at every scale -> {scale: feat}, bands checked"""
    out = {}
    feat = Guarded((n, c))
    native.check(lib.csk_pool_fc_f32(hd.ptr(), None, None, feat.ptr(), None, n, m, c, tv, 0, stream), "csk_pool_fc_f32")
    out["fc", 1.0] = feat.numpy()
    feat.assert_bands()
    for scale in fx.POOL_SCALES:
        feat = Guarded((n, c))
        native.check(lib.csk_pool_scaled_f32(hd.ptr(), feat.ptr(), n, m, c, tv, scale, stream), "csk_pool_scaled_f32")
        out["scaled", scale] = feat.numpy()
        feat.assert_bands()
    return out


@pytest.mark.parametrize("tv", fx.POOL_TV)
def test_pool_exact(tv):
    """feat[n, c] = mean over (m, tv) of h[(n m), c, tv], times scale: integer operands, expected bits
    fp32(fp32(S) / fp32(m tv)) * fp32(scale) from the exact sum S.  TV on either side of every multiple of 64 the lane-strided
    walk cares about (449 .. 511: some lanes keep eight loads in flight, the others do not), row counts that leave waves of the
    last block without a row."""
    lib, stream = native.lib(), _stream()
    for m in fx.POOL_M:
        for n, c in fx.POOL_NC:
            h = fx.exact_operand(np.random.default_rng(tv * 100 + m * 10 + n), (n * m, c, tv))
            s = fx.ref_pool_sum(h, n, m)
            got = _pool_both_entries(lib, stream, Guarded(h.shape, h), n, m, c, tv)
            for (entry, scale), feat in got.items():
                _same_bits(feat, fx.exact_pool_bits(s, m * tv, scale), (entry, scale, tv, m, n, c))


@pytest.mark.parametrize("tv", fx.POOL_FLOAT_TV)
def test_pool_float(tv):
    lib, stream, m = native.lib(), _stream(), fx.POOL_FLOAT_M
    for n, c in fx.POOL_NC:
        h = fx.float_operand(np.random.default_rng(tv + n), (n * m, c, tv))
        got = _pool_both_entries(lib, stream, Guarded(h.shape, h), n, m, c, tv)
        for (entry, scale), feat in got.items():
            want = fx.ref_pool(h, n, m, scale)                            # positive terms: the sum of |term| is the result
            fx.check_bound(feat, want, fx.bound(want, m * tv), n_terms=m * tv, kernel="pool_" + entry, scale=scale, tv=tv, n=n, c=c)


def test_pool_fc_with_logits_exact():
    """csk_pool_fc_f32 with logits: rows with an exact integer mean, integer weights and bias -> feat and logits bit for bit"""
    lib, stream = native.lib(), _stream()
    n, m, c, tv, classes = (fx.POOL_FC_CASE[k] for k in ("n", "m", "c", "tv", "classes"))
    rng = np.random.default_rng(50)
    k, x = fx.exact_mean_rows(rng, n * c, m * tv)
    h = np.ascontiguousarray(np.transpose(x.reshape(n, c, m, tv), (0, 2, 1, 3))).reshape(n * m, c, tv)
    w, b = fx.exact_operand(rng, (classes, c)), fx.exact_operand(rng, (classes,), fx.BIAS_AMP)
    assert np.array_equal(fx.ref_pool(h, n, m), k.reshape(n, c))
    hd, wd, bd, feat, logits = Guarded(h.shape, h), Guarded(w.shape, w), Guarded(b.shape, b), Guarded((n, c)), Guarded((n, classes))
    native.check(lib.csk_pool_fc_f32(hd.ptr(), wd.ptr(), bd.ptr(), feat.ptr(), logits.ptr(), n, m, c, tv, classes, stream), "csk_pool_fc_f32")
    _same_bits(feat.numpy(), k.reshape(n, c), "feat")
    _same_bits(logits.numpy(), fx.ref_fc(k.reshape(n, c), w, b), "logits")
    feat.assert_bands()
    logits.assert_bands()


# ---- FC -----------------------------------------------------------------------------------------------------------------------
def _fc_operands(tier, n, c, classes):
    rng = np.random.default_rng(c * 1000 + classes + n)
    if tier == "exact":
        return fx.exact_operand(rng, (n, c)), fx.exact_operand(rng, (classes, c)), fx.exact_operand(rng, (classes,), fx.BIAS_AMP)
    return fx.float_operand(rng, (n, c)), fx.float_operand(rng, (classes, c)), fx.float_operand(rng, (classes,))


@pytest.mark.parametrize("tier", ["exact", "float"])
@pytest.mark.parametrize("c", fx.FC_C)
def test_fc(c, tier):
    """logits = feat . fc_w^T + fc_b for class counts on either side of the 64 classes of a wave and wave counts that leave the
    last block short.  C % 4 != 0: the feature pointer is only 4-byte aligned (the scalar path must take it); C % 4 == 0: the
    same pointer is refused before any launch, and the logits stay unwritten."""
    lib, stream = native.lib(), _stream()
    for classes in fx.FC_CLASSES:
        for n in fx.FC_N:
            feat, w, b = _fc_operands(tier, n, c, classes)
            wd, bd = Guarded(w.shape, w), Guarded(b.shape, b)
            skew = Guarded(feat.shape, feat, offset=1)
            assert skew.t.data_ptr() % 16 == 4 and wd.t.data_ptr() % 16 == 0
            logits = Guarded((n, classes))
            if c % 4 == 0:
                assert lib.csk_fc_f32(skew.ptr(), wd.ptr(), bd.ptr(), logits.ptr(), n, c, classes, stream) == -1
                assert b"16-byte aligned" in lib.csk_last_error()
                assert np.isnan(logits.numpy()).all()
                fd = Guarded(feat.shape, feat)
            else:
                fd = skew
            native.check(lib.csk_fc_f32(fd.ptr(), wd.ptr(), bd.ptr(), logits.ptr(), n, c, classes, stream), "csk_fc_f32")
            want = fx.ref_fc(feat, w, b)
            if tier == "exact":
                _same_bits(logits.numpy(), want, (c, classes, n))
            else:
                fx.check_bound(logits.numpy(), want, fx.bound(want, c + 1), n_terms=c + 1, kernel="fc", c=c, classes=classes, n=n)
            logits.assert_bands()


# ---- continual head, the separate launches ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv", fx.SPATIAL_MV)
def test_co_spatial_pool(mv):
    """feat[n, c] = mean of the mv positions of stream n in row c of a channel-major frame [c, P], P > n mv: the columns behind
    the last stream are NaN"""
    lib, stream = native.lib(), _stream()
    for n, c in fx.SPATIAL_NC:
        p = fx.spatial_p(n, mv)
        for tier in ("exact", "float"):
            h = (fx.exact_operand if tier == "exact" else fx.float_operand)(np.random.default_rng(mv + n), (c, p))
            h[:, n * mv:] = np.nan
            hd, feat = Guarded(h.shape, h), Guarded((n, c))
            native.check(lib.csk_co_spatial_pool_f32(hd.ptr(), feat.ptr(), n, c, mv, p, stream), "csk_co_spatial_pool_f32")
            s = fx.ref_spatial_sum(h, n, mv)
            if tier == "exact":
                _same_bits(feat.numpy(), fx.exact_pool_bits(s, mv), (mv, n, c))
            else:
                fx.check_bound(feat.numpy(), s / mv, fx.bound(s / mv, mv), n_terms=mv, kernel="co_spatial_pool", n=n, c=c)
            feat.assert_bands()


@pytest.mark.parametrize("window", fx.WINDOWS)
def test_co_window_mean(window):
    """pooled = (sum of the `count` newest ring entries) / window -- the FIXED divisor of an average over a zero-initialised window
    -- for a window that fills, is full and wraps twice.  Every slot of the ring holds data, so an entry taken from a slot
    outside the `count` newest shows."""
    lib, stream, n_elem = native.lib(), _stream(), fx.WINDOW_ELEMS
    for tier in ("exact", "float"):
        ring = (fx.exact_operand if tier == "exact" else fx.float_operand)(np.random.default_rng(window), (window, n_elem))
        rd = Guarded(ring.shape, ring)
        for head, count in fx.window_states(window):
            pooled = Guarded((n_elem,))
            native.check(lib.csk_co_window_mean_f32(rd.ptr(), pooled.ptr(), n_elem, window, head, count, stream), "csk_co_window_mean_f32")
            s = fx.ref_window_sum(ring, head, count, window)
            if tier == "exact":
                _same_bits(pooled.numpy(), fx.exact_pool_bits(s, window), (window, head, count))
            else:
                fx.check_bound(pooled.numpy(), s / window, fx.bound(s / window, count), n_terms=count, kernel="co_window_mean",
                               window=window, head=head)
            pooled.assert_bands()


# ---- continual head in one launch ---------------------------------------------------------------------------------------------
def _head_case(tier, n, c, mv, classes, window):
    lib, stream = native.lib(), _stream()
    w, b, frames = fx.head_operands(tier, n, c, mv, classes, window, seed=c + window)
    p = fx.spatial_p(n, mv)
    wd, bd = Guarded(w.shape, w), Guarded(b.shape, b)
    ring = Guarded((window, n, c), np.zeros((window, n, c), dtype=f32))
    pooled, logits = Guarded((n, c)), Guarded((n, classes))
    before = np.zeros((window, n, c), dtype=f32)
    ring64 = np.zeros((window, n, c))                                   # exact tier: the ring as the definition gives it
    info = dict(n=n, c=c, mv=mv, classes=classes, window=window)
    for (step, head, count, emit, zero), h in zip(fx.head_steps(window), frames):
        hd = None if zero else Guarded(h.shape, h)
        pooled.t.fill_(SENTINEL)
        logits.t.fill_(SENTINEL)
        native.check(lib.csk_co_head_step_f32(None if zero else hd.ptr(), ring.ptr(), pooled.ptr(), wd.ptr(), bd.ptr(), logits.ptr(), n, c, mv,
                                              p, window, head, count, emit, classes, stream), "csk_co_head_step_f32")
        got_ring, got_pooled, got_logits = ring.numpy(), pooled.numpy(), logits.numpy()
        others = np.arange(window) != head
        assert np.array_equal(got_ring[others], before[others]), ("a ring slot other than `head` changed", step)
        before = got_ring
        mean = np.zeros((n, c)) if zero else fx.ref_spatial_sum(h, n, mv) / mv
        ring64[head] = mean
        if tier == "exact" or zero:
            _same_bits(got_ring[head], mean, ("ring", step))
        else:
            fx.check_bound(got_ring[head], mean, fx.bound(mean, mv), n_terms=mv, kernel="co_head/ring", step=step, **info)
        if not emit:                                                    # a silent step: the slot is written, nothing else
            assert np.all(got_pooled == f32(SENTINEL)) and np.all(got_logits == f32(SENTINEL)), step
            continue
        if tier == "exact":
            want = fx.ref_window_sum(ring64, head, count, window) / window
            _same_bits(got_pooled, want, ("pooled", step))
            _same_bits(got_logits, fx.ref_fc(want, w, b), ("logits", step))
        else:                                                           # stage by stage, each a sum of at most 600 terms
            want = fx.ref_window_sum(got_ring, head, count, window) / window
            fx.check_bound(got_pooled, want, fx.bound(want, count), n_terms=count, kernel="co_head/pooled", step=step, **info)
            want = fx.ref_fc(got_pooled, w, b)
            fx.check_bound(got_logits, want, fx.bound(want, c + 1), n_terms=c + 1, kernel="co_head/logits", step=step, **info)
    for g in (ring, pooled, logits):
        g.assert_bands()


@pytest.mark.parametrize("n,c,mv,classes,window", fx.HEAD_EXACT)
def test_co_head_step_exact(n, c, mv, classes, window):
    """csk_co_head_step_f32 against the definition (models/base.py:84-101: spatial mean -> average over a zero-initialised window
    -> linear), bit for bit: every (row, stream) of a frame is an integer k plus a zero-sum permutation, so the ring entry is k,
    the pooled value a multiple of 1 / window and the logits exact.  Over 2 window + 3 steps, one of them a zero feature
    (h = NULL), every fifth silent (emit = 0: pooled and logits keep their sentinel, the ring slot is still written); at every
    step only the slot `head` of the ring changes.  C = 65, 70: rows past a multiple of 64 and of 4; C = 516: a third pass of the
    256 threads over the channels."""
    _head_case("exact", n, c, mv, classes, window)


@pytest.mark.parametrize("n,c,mv,classes,window", fx.HEAD_FLOAT)
def test_co_head_step_float(n, c, mv, classes, window):
    """the same steps on positive operands against fp64 under the derived bound, stage by stage: the ring entry from the frame
    (mv terms), pooled from the ring the launch left (count terms), the logits from the pooled values it left (C + 1 terms).
    Windows 10, 17 and 75: entries older than the newest are taken eight at a time, here in two, two and ten passes."""
    _head_case("float", n, c, mv, classes, window)


# ---- input permute + data_bn --------------------------------------------------------------------------------------------------
def _input_norm_case(shape, chan_gap=0, seg_gap=0):
    """One fma per element, correctly rounded: the reference is x scale + shift rounded ONCE to fp32, compared bit for bit over the
    whole output buffer -- the gaps between channels and segments, NaN before, are NaN after."""
    n, c, t, v, m = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape).astype(f32)
    scale, shift = fx.distinct_affine(rng, m * v * c)
    chan = t * v + chan_gap
    seg = c * chan + seg_gap
    want = np.full(n * m * seg, np.nan, dtype=f32)
    np.lib.stride_tricks.as_strided(want, (n * m, c, t * v), (4 * seg, 4 * chan, 4))[...] = fx.ref_input_norm(x, scale, shift).reshape(n * m, c, t * v)
    xd, sd, td, out = Guarded(x.shape, x), Guarded(scale.shape, scale), Guarded(shift.shape, shift), Guarded(want.shape)
    native.check(native.lib().csk_input_norm_f32(xd.ptr(), sd.ptr(), td.ptr(), out.ptr(), n, c, t, v, m, seg, chan, _stream()), "csk_input_norm_f32")
    assert np.array_equal(out.numpy(), want, equal_nan=True), shape
    out.assert_bands()


@pytest.mark.parametrize("shape", fx.NORM_DENSE)
def test_input_norm_dense(shape):
    _input_norm_case(shape)


def test_input_norm_strided_output_leaves_the_gaps_alone():
    _input_norm_case(fx.NORM_STRIDED, chan_gap=4, seg_gap=8)


def test_input_norm_beyond_one_grid_of_threads():
    """2.16 M elements: more than the threads a launch starts, every thread takes a second element"""
    _input_norm_case(fx.NORM_LARGE)


@pytest.mark.parametrize("shape", fx.FRAMES_SHAPES)
@pytest.mark.parametrize("r", fx.FRAMES_R)
def test_input_norm_frames(r, shape):
    """r frames (N, C, V, M) of a launch cycle -> channel-major ring slots [C, P] in one launch: a frame of its own data per slot,
    the slots in ring order across the wrap (not ascending addresses), the padding columns from N M V on and the slots no frame
    goes to still NaN."""
    n, c, v, m = shape
    rng = np.random.default_rng(r * 10 + c)
    p, depth = fx.frames_p(n, m, v), r + 2
    scale, shift = fx.distinct_affine(rng, m * v * c)
    xs = [rng.standard_normal(shape).astype(f32) for _ in range(r)]
    slots = [(depth - 2 + f) % depth for f in range(r)]
    assert r < 3 or slots != sorted(slots)
    want = np.full((depth, c, p), np.nan, dtype=f32)
    for x, slot in zip(xs, slots):
        want[slot] = fx.ref_input_norm_frame(x, scale, shift, p)
    xds, sd, td, ring = [Guarded(shape, x) for x in xs], Guarded(scale.shape, scale), Guarded(shift.shape, shift), Guarded(want.shape)
    srcs = (ctypes.c_void_p * r)(*[xd.t.data_ptr() for xd in xds])
    dsts = (ctypes.c_void_p * r)(*[ring.t[slot].data_ptr() for slot in slots])
    native.check(native.lib().csk_input_norm_frames_f32(srcs, dsts, r, sd.ptr(), td.ptr(), n, c, v, m, p, _stream()), "csk_input_norm_frames_f32")
    assert np.array_equal(ring.numpy(), want, equal_nan=True), (r, shape)
    ring.assert_bands()


# ---- the Python wrappers ------------------------------------------------------------------------------------------------------
def _wrapper_net():
    net = pkg.StGcn(pkg.ntu_graph().A, input_shape=fx.WRAPPER_SHAPE).eval()
    g = torch.Generator().manual_seed(11)
    bn = net.data_bn
    with torch.no_grad():
        bn.weight.copy_(torch.rand(bn.weight.shape, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(bn.bias.shape, generator=g))
        bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=g))
        bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=g) + 0.5)
        net.fc.weight.copy_(torch.rand(net.fc.weight.shape, generator=g) + 0.5)
        net.fc.bias.copy_(torch.rand(net.fc.bias.shape, generator=g) + 0.5)
    return net, g


def test_stgcn_input_norm_wrapper():
    """StGcn.input_norm against torch's fp64 BatchNorm1d on the reference's permute / view (st_gcn.py:49-57), data_bn with
    running statistics and an affine map of its own per channel.  Folding data_bn into fp32 scale / shift rounds each once more:
    4 * 2^-24 (|x scale| + |shift|) per element."""
    c, t, v, m = fx.WRAPPER_SHAPE
    n = fx.WRAPPER_N
    net, g = _wrapper_net()
    x = torch.randn((n, c, t, v, m), generator=g)
    bn64 = torch.nn.BatchNorm1d(m * v * c).double().eval()
    bn64.load_state_dict(net.data_bn.state_dict())
    with torch.no_grad():
        y = bn64(x.double().permute(0, 4, 3, 1, 2).contiguous().view(n, m * v * c, t))
        want = y.view(n, m, v, c, t).permute(0, 1, 3, 4, 2).contiguous().view(n * m, c, t, v).numpy()
        scale = (bn64.weight / torch.sqrt(bn64.running_var + bn64.eps))
        shift = (bn64.bias - bn64.running_mean * scale).abs().numpy()
    room = fx.ref_input_norm(np.abs(x.numpy()), np.abs(scale.numpy()), shift, combine=lambda a, s, b: fx.f64(a) * s + b)
    got = net.to(DEV).input_norm(x.to(DEV)).cpu().numpy()
    assert got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= 4 * fx.U * room), float((err / (4 * fx.U * room)).max())


def test_stgcn_head_wrapper():
    """StGcn.head against fp64 mean + linear on positive operands.  Two nested sums -- m T V terms per feature, then 256 products
    and the bias -- whose relative errors add: the derived bound with n_terms = m T V + 256 + 1."""
    c, t, v, m = fx.WRAPPER_SHAPE
    n = fx.WRAPPER_N
    net, g = _wrapper_net()
    h = torch.rand((n * m, 256, t, v), generator=g) + 0.5
    with torch.no_grad():
        feat = h.double().view(n, m, 256, -1).mean(3).mean(1)
        want = torch.nn.functional.linear(feat, net.fc.weight.double(), net.fc.bias.double()).numpy()
    net = net.to(DEV)
    with torch.no_grad():
        got = net.head(h.to(DEV), n, m).cpu().numpy()
    n_terms = m * t * v + 256 + 1
    fx.check_bound(got, want, fx.bound(want, n_terms), n_terms=n_terms, kernel="StGcn.head")
