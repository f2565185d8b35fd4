"""GPU tests of the frame-wise adaptive graph-conv stage (csk_agcn_stage_framewise_f32, csrc/agcn_framewise.hip) and of the clip pass
built on it (AdaptiveGraphConvolution.forward_framewise, CoAGcn.features_clip_as_steps / forward_clip_as_steps): the kernel against the
fp64 per-frame definition of tests/agcn_framewise_fixture.py -- under the derived bound on positive operands, bit for bit on the exact
tier -- between NaN guard bands; frame independence, bitwise; the kernel against the composed existing launches; and the model against
``clean_state(); forward_steps(x)``."""
import ctypes

import numpy as np
import pytest
import torch

import _bootstrap
from tests import agcn_attention_fixture as att
from tests import agcn_framewise_fixture as fx
from tests.helpers import randomise_unit_
from tests.test_gpu_dense_gcn import Guarded, _stream

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
DEV = "cuda:0"
f32 = np.float32


def _layout(c, T=None):
    T = c.T if T is None else T
    chan = T * c.V
    return chan, c.c_in * chan + c.seg_pad, c.c_out * chan + c.seg_pad


def _strided(a, seg_stride):
    """[n, C, T, V] -> flat with `seg_stride` floats per segment, the gaps NaN"""
    n = a.shape[0]
    flat = np.full((n, seg_stride), np.nan, dtype=f32)
    flat[:, : a[0].size] = a.reshape(n, -1)
    return flat.reshape(-1)


class Device:
    """the packed operands of a case on the device, each between guard bands"""

    def __init__(self, c, ops):
        self.c, inter = c, fx.inter_of(c)
        w_img, b_img = fx.stage_image(ops["W"], ops["bias"])
        e_img, eb_img = att.pair_major(ops["we"], ops["be"], inter)
        self.w, self.b, self.we, self.be, self.a = Guarded(w_img), Guarded(b_img), Guarded(e_img), Guarded(eb_img), Guarded(ops["a_sum"])

    def run(self, x):
        """one launch on x [n, c_in, T, V] -> y [n, c_out, T, V]; guards and the gaps behind the segments asserted"""
        c, (n, _, T, V) = self.c, x.shape
        chan, xs, ys = _layout(c, T)
        xd, yd = Guarded(_strided(x, xs)), Guarded(size=n * ys)
        res = 2 if c.conv_res else 1
        lib = native.lib()
        assert lib.csk_agcn_stage_framewise_f32_route(xd.ptr(), n, c.c_in, c.c_out, fx.inter_of(c), T, V, xs, chan, res) == fx.route_of(c)
        native.check(lib.csk_agcn_stage_framewise_f32(xd.ptr(), yd.ptr(), self.w.ptr(), self.b.ptr(), self.we.ptr(), self.be.ptr(), self.a.ptr(),
                                                      n, c.c_in, c.c_out, fx.inter_of(c), T, V, xs, chan, ys, chan, res, _stream()),
                     "csk_agcn_stage_framewise_f32")
        torch.cuda.synchronize()
        for g in (xd, yd, self.w, self.b, self.we, self.be, self.a):
            g.assert_bands()
        out = yd.numpy().reshape(n, ys)
        assert np.isnan(out[:, c.c_out * chan:]).all(), "the gap behind a segment of y was written"
        return out[:, : c.c_out * chan].reshape(n, c.c_out, T, V)

    def run_composed(self, x):
        """the existing launches on the same operands: csk_agcn_embed_attention_f32 (per frame) + csk_gcn_stage_f32 (adj_per_frame)"""
        c, (n, _, T, V) = self.c, x.shape
        chan, xs, ys = _layout(c, T)
        xd, yd, adj = Guarded(_strided(x, xs)), Guarded(size=n * ys), Guarded(size=n * T * 3 * V * V)
        lib, inter = native.lib(), fx.inter_of(c)
        native.check(lib.csk_agcn_embed_attention_f32(xd.ptr(), self.we.ptr(), self.be.ptr(), self.a.ptr(), adj.ptr(), None, n, c.c_in, inter, T,
                                                      V, 1, xs, chan, _stream()), "csk_agcn_embed_attention_f32")
        src = torch.arange(V, dtype=torch.int32).repeat(3, V, 1).contiguous().to(DEV)
        cnt = (ctypes.c_int32 * 3)(V, V, V)
        native.check(lib.csk_gcn_stage_f32(xd.ptr(), yd.ptr(), self.w.ptr(), self.b.ptr(), native.ptr(src), adj.ptr(),
                                           ctypes.cast(cnt, ctypes.c_void_p), V, 3 * V * V, 1, n, c.c_in, c.c_out, T, V, xs, chan, ys, chan,
                                           2 if c.conv_res else 1, _stream()), "csk_gcn_stage_f32")
        torch.cuda.synchronize()
        return yd.numpy().reshape(n, ys)[:, : c.c_out * chan].reshape(n, c.c_out, T, V)


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


@pytest.mark.parametrize("c", fx.CASES, ids=lambda c: c.name)
def test_kernel_against_the_fp64_definition_and_the_composed_launches(c):
    inter = fx.inter_of(c)
    # exact tier: uniform logit columns by construction, every sum exact -> bit for bit
    ops = fx.operands(c, "exact")
    fx.admissible(c, ops)
    want = fx.definition(ops, inter, c.conv_res, adj=ops["adj_exact"]).astype(f32)
    got = Device(c, ops).run(ops["x"])
    assert np.array_equal(_bits(got), _bits(want)), (c.name, float(np.abs(got - want).max()))
    # positive tier: the derived bound, for the kernel against the definition and against the composed launches
    ops = fx.operands(c, "positive")
    y = fx.definition(ops, inter, c.conv_res)
    b = fx.bound(c, ops, y)
    dev = Device(c, ops)
    got, comp = dev.run(ops["x"]), dev.run_composed(ops["x"])
    r_def, r_comp = float((np.abs(got - y) / b).max()), float((np.abs(got - comp) / b).max())
    print(f"{c.name}: largest err / bound = {r_def:.3f} against the definition, {r_comp:.3f} against the composed launches "
          f"(bound / y = {float((b / y).max()):.2e})")
    assert r_def <= 1.0, (c.name, r_def)
    assert r_comp <= 1.0, (c.name, r_comp)


@pytest.mark.parametrize("c", list(fx.PER_INSTANTIATION.values()), ids=lambda c: c.name)
def test_frames_are_independent_bitwise(c):
    """Frame t of a T-frame launch equals the T = 1 launch on that frame alone, for every t; a NaN placed in frame t reaches the
    outputs of frame t only."""
    ops = fx.operands(c, "positive")
    dev = Device(c, ops)
    full = dev.run(ops["x"])
    for t in range(c.T):
        one = dev.run(np.ascontiguousarray(ops["x"][:, :, t:t + 1]))
        assert np.array_equal(_bits(full[:, :, t:t + 1]), _bits(one)), (c.name, t)
    t = c.T // 2
    x = ops["x"].copy()
    x[c.n_seg - 1, c.c_in // 2, t, c.V // 3] = np.nan
    bad = dev.run(x)
    keep = np.ones(full.shape, dtype=bool)
    keep[c.n_seg - 1, :, t] = False
    assert np.array_equal(_bits(bad[keep]), _bits(full[keep])) and np.isnan(bad[c.n_seg - 1, :, t]).all(), c.name


@pytest.mark.parametrize("ci,co,t,v", [(64, 64, 9, 18), (64, 128, 8, 25), (3, 64, 11, 18), (16, 24, 7, 25), (40, 40, 5, 20)])
def test_forward_framewise_routes_agree_and_chunking_keeps_the_bits(ci, co, t, v):
    """The module: the kernel route against the composed route (class attribute off) within 1e-4 of the largest value; the composed
    route gives the same bits whatever the byte budget cuts the clip into; shapes the kernel is not built for take the composition."""
    A = pkg.kinetics_graph().A if v == 18 else (pkg.ntu_graph().A if v == 25 else np.random.default_rng(0).random((3, v, v)).astype(f32))
    m = pkg.AdaptiveGraphConvolution(ci, co, torch.as_tensor(A)).eval()
    randomise_unit_(m, 5 + ci + t, attn_scale=1 / v)
    m = m.to(DEV)
    x = torch.rand(3, ci, t, v, generator=torch.Generator().manual_seed(3)).to(DEV)
    built = v in (18, 25) and co // 4 in (16, 32, 64) and co % 4 == 0
    cls = type(m)
    shipped = m.forward_framewise(x)                  # the default: the kernel where it measured faster, else the composition
    assert m.framewise_route(x) in (0, m.inter_c * 1000 + v * 10 + int(ci != co)) and (built or m.framewise_route(x) == 0)
    try:
        cls.framewise_everywhere = True
        assert bool(m.framewise_route(x)) == built
        y = m.forward_framewise(x)
        cls.fuse_framewise = False
        assert m.framewise_route(x) == 0
        comp = m.forward_framewise(x)
        cls.framewise_budget_bytes = 4 * 3 * (3 * v * v + 6 * m.inter_c * v) * 2          # two frames per chunk
        chunked = m.forward_framewise(x)
    finally:
        cls.fuse_framewise, cls.framewise_budget_bytes, cls.framewise_everywhere = True, 256 << 20, False
    assert torch.equal(comp, chunked) and (torch.equal(shipped, y) or torch.equal(shipped, comp))
    assert float((y - comp).abs().max()) <= 1e-4 * float(comp.abs().max())
    if not built:
        assert torch.equal(y, comp)
    # per frame: the step form on that frame alone (T = 1 clip) gives the composed route's bits
    one = torch.cat([m.forward_framewise(x[:, :, k:k + 1].contiguous()) for k in range(t)], dim=2)
    assert torch.equal(one, shipped)


def _net(V, seed=11):
    A = pkg.kinetics_graph().A if V == 18 else pkg.ntu_graph().A
    net = pkg.CoAGcn(A, input_shape=(3, 300, V, 2), num_classes=400 if V == 18 else 60, pool_size=4, pool_padding=0).eval()
    randomise_unit_(net, seed, attn_scale=1 / V)
    return net.to(DEV)


def _close(got, want, what):
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"{what}: {tuple(got.shape)}, largest err {err:.3e} = {err / scale:.2e} of the largest value")
    assert scale > 0 and err <= 1e-4 * scale, (what, err, scale)


@pytest.mark.parametrize("V", [18, 25])
@pytest.mark.parametrize("variant", ["joint", "bone_motion", "keypoints"])
def test_model_clip_as_steps_equals_the_steps(V, variant):
    """T = 96, N = 2, pool_size 4, pool_padding 0, randomised BN: forward_clip_as_steps(x) against clean_state(); forward_steps(x) --
    the same prediction count and the same values within 1e-4 of the largest value, pad_end False and True -- with the model's continual
    state and counters bitwise untouched by the call; the plain clip form forward(x) is NOT that (the test that fails without the
    feature: the method does not exist, and the clip form differs by far more than the tolerance)."""
    net = _net(V)
    g = torch.Generator().manual_seed(4 + V)
    if variant == "bone_motion":
        pkg.set_input_modality(net, "bone_motion")
    if variant == "keypoints":
        pkg.keypoints.set_keypoint_intake(net)
        x = torch.rand(net.stage("keypoints").fed_shape(2, 96), generator=g).to(DEV)
    else:
        x = torch.rand(2, 3, 96, V, 2, generator=g).to(DEV)
    for pad_end in (False, True):
        net.clean_state()
        want = net.forward_steps(x, pad_end=pad_end)
        net.clean_state()
        net.forward_steps(x[:, :40] if variant == "keypoints" else x[:, :, :40])        # a live state the call must not touch
        tensors, position = [t.clone() for t in net._state_tensors()], net._position()
        got = net.forward_clip_as_steps(x, pad_end=pad_end)
        assert all(torch.equal(a, b) for a, b in zip(net._state_tensors(), tensors)) and net._position() == position
        assert want.shape[2] == len(net.clip_as_steps_map(96, pad_end)[1]) and want.shape[2] >= 2
        _close(got, want, f"V={V} {variant} pad_end={pad_end}")
    # needs no bound slab
    fresh = _net(V)
    if variant == "bone_motion":
        pkg.set_input_modality(fresh, "bone_motion")
    if variant == "keypoints":
        pkg.keypoints.set_keypoint_intake(fresh)
    assert torch.equal(fresh.forward_clip_as_steps(x, pad_end=True), got) and fresh._n is None
    # the feature frames: as many as the clip has, the first ones are what the steps emit
    h = net.features_clip_as_steps(x)
    assert h.shape == (4, 256, net.prime_clip_frames(96)[-1], V)
    # not the old clip form in disguise: forward(x) is the first window of the per-SEGMENT attention
    net.clean_state()
    first = net.forward_steps(x)[:, :, 0]
    clip = net(x)
    gap = float((clip - first).abs().max()) / float(first.abs().max())
    print(f"V={V} {variant}: forward(x) against the first prediction of the steps: {gap:.2e} of the largest value")
    assert gap > 10 * 1e-4
