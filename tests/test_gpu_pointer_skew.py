"""Every clip kernel at activation, residual and output pointers OFF the 16-byte boundary (tests/skew_fixture.py; the fixture's
tables and its defect model are proven on the CPU by tests/test_skew_fixture_cpu.py).

Kernel level, per takes_any entry x launch x (x, x_res, out) skew: each caller-visible tensor is a view at GUARD + s floats of a
16-byte aligned buffer, NaN bands around the inputs, a finite sentinel around and under the output.  The operands are exact
(unique ids under one-hot weights, or small integers), so the result must equal the fixture's fp64 reference BIT FOR BIT whatever
the summation order, be finite, and leave every band word as it was.  The Winograd launches get a direct weight image full of NaN: a
fall-back to the direct kernels fails.  Rerouting and refusing entries: the route the classification predicts, the fp64 result either
way; -1 with the message and an untouched output.

Through the package: a module's forward on an offset-s view (and into an offset ``out=`` view) is bitwise its forward on an aligned
copy -- GraphConvolution, SpatioTemporalBlock in its residual / stride / fused / valid-Winograd forms, the S-TR unit, the StGcn clip
forward, forward_cycle with every frame at its own skew; the adaptive graph conv at V = 18 leaves its fused path at an odd offset and
agrees with it within the parity tolerance of tests/test_gpu_agcn_parity.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _bootstrap
from tests import dense_gcn_fixture as dx
from tests import skew_fixture as sk
from tests import agcn_attention_fixture as af
from tests import split_fixture as sf
from tests import str_unit_fixture as su
from tests import tcn_wino_fixture as tw
from tests import test_skew_fixture_cpu as cpu
from tests.helpers import TOL, max_err, randomise_unit_

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native, fold = pkg.native, pkg.fold
DEV = "cuda:0"
NAN = float("nan")


def _stream():
    return native.stream_of(torch.empty(1, device=DEV))


def _launch(unit, skew):
    """one launch of the unit with its operands at the skew -> (output on the host, every band intact)"""
    h, off = sk.host_operands(unit), sk.skew_of(unit, skew)
    d, c = h["ops"], unit.case
    x = sk.Skewed(h["x"].shape, off["x"], DEV, src=h["x"])
    xr = sk.Skewed(h["x_res"].shape, off["x_res"], DEV, src=h["x_res"]) if "x_res" in off else None
    out = sk.Skewed(sk.out_shape(unit), off["out"], DEV)
    if unit.kind in ("tcn", "wino"):
        ones = torch.ones(c.co, dtype=torch.float64)
        w = fold.pack_conv_weight(d["w"], ones)
        kw = dict(relu=bool(c.relu), res_mode={"none": 0, "identity": 1, "conv": 2}[c.res], x_res=xr.t if xr else None,
                  w_res=fold.pack_conv_weight(d["wres"], ones).to(DEV) if "wres" in d else None, res_off=c.res_off, out=out.t)
        if unit.kind == "wino":
            kw[tw.ENTRY_KW[c.entry]] = (fold.pack_conv_weight_wino_s2 if c.stride == 2 else fold.pack_conv_weight_wino)(d["w"], ones).to(DEV)
            w = torch.full_like(w, NAN)                                 # the direct kernels must not run
        elif c.ksplit > 1:
            kw.update(ksplit=c.ksplit, scratch=pkg.blocks.SplitScratch())
        pkg.blocks.tcn_stage(x.t, w.to(DEV), fold.pad_vec(d["bias"]).to(DEV), c.co, 9, c.stride, c.pad, **kw)
    elif unit.kind == "bf":
        w_img, r_img = sf.pack_images(d, fold)
        r_img = None if r_img is None else r_img.to(DEV)
        bias = fold.pad_vec(torch.zeros(c.co)).to(DEV)
        res = {"none": 0, "ident": 1, "conv": 2}[c.res]
        if c.kernel == "tcn":
            pkg.blocks.tcn_stage(x.t, w_img.to(DEV), bias, c.co, sf.K_TCN, c.stride, sf.PAD_TCN, relu=False, res_mode=res,
                                 x_res=xr.t if xr else None, w_res=r_img, out=out.t, split=True)
        else:
            src, val, cnt, ew = fold.ell_from_dense(d.adj)
            src, val = src.to(DEV), val.to(DEV)
            native.check(native.lib().csk_gcn_stage_bf16x3(native.ptr(x.t), native.ptr(out.t), native.ptr(w_img.to(DEV)), native.ptr(r_img), native.ptr(bias),
                                                           native.ptr(src), native.ptr(val), native.ptr(cnt), ew, c.N, c.ci, c.co, c.T, c.V, res,
                                                           _stream()), unit.entry)
    elif unit.kind == "str":
        lib = native.lib()
        xs, ys = su.xy_strides(c)
        g = {k: (None if d[k] is None else torch.from_numpy(np.ascontiguousarray(d[k], dtype=np.float32)).to(DEV))
             for k in ("w_qkv", "b_qkv", "s_in", "t_in", "w_out", "b_out", "res_scale")}
        scratch = torch.full((su.scratch_floats(c),), NAN, device=DEV)
        native.check(lib.csk_str_unit_f32(native.ptr(x.t), native.ptr(out.t), native.ptr(scratch), su.scratch_floats(c), native.ptr(g["w_qkv"]),
                                          native.ptr(g["b_qkv"]), native.ptr(g["s_in"]), native.ptr(g["t_in"]), native.ptr(g["w_out"]),
                                          native.ptr(g["b_out"]), native.ptr(g["res_scale"]), c.n_seg, c.c_in, c.c_out, c.frames, c.V,
                                          xs[0], xs[1], ys[0], ys[1], _stream()), unit.entry)
    elif unit.kind == "att":
        a = torch.from_numpy(np.ascontiguousarray(d["a_sum"], dtype=np.float32)).to(DEV)
        scratch = torch.full((c.n * 3 * 4 * c.V * c.V,), NAN, device=DEV)
        chan = c.T * c.V
        native.check(native.lib().csk_agcn_attention_f32(native.ptr(x.t), native.ptr(a), native.ptr(out.t), native.ptr(scratch), c.n, c.inter, c.T, c.V,
                                                         6 * c.inter * chan, chan, c.n, 0, _stream()), unit.entry)
    elif unit.kind == "norm":
        sc, sh = (torch.from_numpy(d[k]).to(DEV) for k in ("scale", "shift"))
        native.check(native.lib().csk_input_norm_f32(native.ptr(x.t), native.ptr(sc), native.ptr(sh), native.ptr(out.t), c.n, c.c, c.t, c.v, c.m,
                                                     c.c * c.t * c.v, c.t * c.v, _stream()), unit.entry)
    elif unit.kind == "pool":
        lib = native.lib()
        if unit.entry == "csk_pool_fc_f32":
            rc = lib.csk_pool_fc_f32(native.ptr(x.t), None, None, native.ptr(out.t), None, c.n, c.m, c.c, c.t * c.v, 0, _stream())
        else:
            rc = lib.csk_pool_scaled_f32(native.ptr(x.t), native.ptr(out.t), c.n, c.m, c.c, c.t * c.v, c.scale, _stream())
        native.check(rc, unit.entry)
    else:
        lib = native.lib()
        xc, xs, yc, ys = dx.strides(c)
        assert (xc, yc) == (c.frames * c.V,) * 2                        # packed rows: the row class follows from T * V
        w_img, b_img = dx.pack_w(d["w"], d["bias"])
        w, b = torch.from_numpy(w_img).to(DEV), torch.from_numpy(b_img).to(DEV)
        if unit.kind == "conv":
            rc = lib.csk_conv1x1_f32(native.ptr(x.t), native.ptr(out.t), native.ptr(w), native.ptr(b), c.n_seg, c.c_in, c.c_out, c.frames, c.V,
                                     xs, xc, ys, yc, _stream())
        else:
            src = torch.from_numpy(d["ell_src"].reshape(-1)).to(DEV)
            ell = torch.from_numpy(d["ell_val"]).to(DEV)
            cnt = ctypes.cast((ctypes.c_int32 * 3)(*c.ell_cnt), ctypes.c_void_p)
            if unit.ksplit > 1:
                part = torch.full((c.n_seg * unit.ksplit * c.c_out * yc,), NAN, device=DEV)
                rc = lib.csk_gcn_stage_splitk_f32(native.ptr(x.t), native.ptr(out.t), native.ptr(w), native.ptr(b), native.ptr(src), native.ptr(ell),
                                                  cnt, c.ell_w, c.n_seg, c.c_in, c.c_out, c.frames, c.V, xs, xc, ys, yc, c.res, unit.ksplit,
                                                  native.ptr(part), _stream())
            else:
                rc = lib.csk_gcn_stage_f32(native.ptr(x.t), native.ptr(out.t), native.ptr(w), native.ptr(b), native.ptr(src), native.ptr(ell), cnt,
                                           c.ell_w, 0, 0, c.n_seg, c.c_in, c.c_out, c.frames, c.V, xs, xc, ys, yc, c.res, _stream())
        native.check(rc, unit.entry)
    torch.cuda.synchronize()
    return out.host(), all(g.bands_intact() for g in (x, xr, out) if g is not None)


@functools.lru_cache(maxsize=None)
def _control(unit):
    """the (0, 0, 0) launch of a unit of a non-exact tier, once"""
    got, intact = _launch(unit, sk.CONTROL)
    assert intact and sk.matches(unit, got), unit.name
    return got


@pytest.mark.parametrize("skew", sk.ALL_SKEWS, ids=lambda s: "skew" + "".join(map(str, s)))
@pytest.mark.parametrize("unit", sk.UNITS, ids=lambda u: f"{u.entry}-{u.name}".replace(" ", "_"))
def test_takes_any(unit, skew):
    """exact tier: fp64's bits; bf16x3 and the attention: the fixture's own bound and the bits of the (0, 0, 0) launch"""
    assert sk.ENTRIES[unit.entry].cls == sk.TAKES_ANY
    got, intact = _launch(unit, skew)
    assert intact, f"a guard band was written: {unit.name} {skew}"
    assert bool(torch.isfinite(got).all()), f"a read outside the operand, or an output left unwritten: {unit.name} {skew}"
    assert sk.matches(unit, got), f"outputs differ from fp64: {unit.name} {skew}"
    if not unit.exact:
        assert sk.same_bits(got, _control(unit)), f"not the bits of the aligned launch: {unit.name} {skew}"


# ---- reroutes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("co", sorted(dx.LEAVE_BASE))
def test_dense_route_follows_the_pointer_and_meets_fp64_either_way(co):
    """the dense V = 18 stage: dense2 at 0 and 8 bytes, dense128 (c_out 128) / general (64) at 4 and 12; exact operands, so fp64's bits"""
    lib, c = native.lib(), dx.LEAVE_BASE[co]
    ops = dx.operands(c, "exact")
    want = torch.from_numpy(dx.reference(c, ops)[0].astype(np.float32))
    xc, xs, yc, ys = dx.strides(c)
    w_img, b_img = dx.pack_w(ops["w"], ops["bias"])
    w, b = torch.from_numpy(w_img).to(DEV), torch.from_numpy(b_img).to(DEV)
    src, ell = torch.from_numpy(ops["ell_src"].reshape(-1)).to(DEV), torch.from_numpy(ops["ell_val"]).to(DEV)
    cnt = ctypes.cast((ctypes.c_int32 * 3)(*c.ell_cnt), ctypes.c_void_p)
    stride, per_frame = dx.adj_args(c)
    for s in (0, 1, 2, 3):
        x = sk.Skewed(ops["x"].shape, s, DEV, src=torch.from_numpy(ops["x"]))
        y = sk.Skewed(want.shape, (s + 1) % 4, DEV)
        route = dx.route_query(lib, c, x.t.data_ptr(), y.t.data_ptr(), ell.data_ptr())
        assert (route == c.route) if s % 2 == 0 else (route == (dx.DENSE128 * dx.UNIT if co == 128 else dx.GENERAL * dx.UNIT + 645)), (s, route)
        native.check(lib.csk_gcn_stage_f32(native.ptr(x.t), native.ptr(y.t), native.ptr(w), native.ptr(b), native.ptr(src), native.ptr(ell), cnt,
                                           c.ell_w, stride, per_frame, c.n_seg, c.c_in, c.c_out, c.frames, c.V, xs, xc, ys, yc, c.res, _stream()),
                     "csk_gcn_stage_f32")
        torch.cuda.synchronize()
        assert x.bands_intact() and y.bands_intact() and sk.same_bits(y.host(), want), s


# ---- refuses ----------------------------------------------------------------------------------------------------------------------
def test_fc_refuses_and_leaves_the_output_alone():
    lib = native.lib()
    w, b = torch.ones(5, 8, device=DEV), torch.ones(5, device=DEV)
    for s in (1, 2, 3):
        feat, logits = sk.Skewed((2, 8), s, DEV, src=torch.ones(2, 8)), sk.Skewed((2, 5), s, DEV)
        rc = lib.csk_fc_f32(native.ptr(feat.t), native.ptr(w), native.ptr(b), native.ptr(logits.t), 2, 8, 5, _stream())
        torch.cuda.synchronize()
        assert rc == -1 and sk.ENTRIES["csk_fc_f32"].message in lib.csk_last_error().decode()
        assert logits.bands_intact() and bool((logits.host() == sk.OUT_SENTINEL).all())
    feat, logits = sk.Skewed((2, 8), 0, DEV, src=torch.ones(2, 8)), sk.Skewed((2, 5), 3, DEV)          # the output may sit anywhere
    native.check(lib.csk_fc_f32(native.ptr(feat.t), native.ptr(w), native.ptr(b), native.ptr(logits.t), 2, 8, 5, _stream()), "csk_fc_f32")
    torch.cuda.synchronize()
    assert logits.bands_intact() and bool((logits.host() == 9.0).all())


@pytest.mark.parametrize("entry", sorted(cpu.GUARDS))
def test_refusing_entries_write_nothing(entry):
    """real device pointers: every operand a region of one large aligned buffer full of the sentinel, the guarded operand moved off the
    boundary -> -1 with the entry's message, and afterwards no word of the buffer has changed"""
    call, offsets, _, _ = cpu.GUARDS[entry]
    big = torch.full((1 << 22,), sk.OUT_SENTINEL, device=DEV)
    assert big.data_ptr() % 16 == 0
    old, cpu.FAKE = cpu.FAKE, big.data_ptr()
    try:
        for s in offsets:
            rc = call(big.data_ptr() + (1 << 22) + 4 * s)                  # 1 Mi floats in, s floats off
            torch.cuda.synchronize()
            assert rc == -1 and sk.ENTRIES[entry].message in cpu._err(), (entry, s, rc, cpu._err())
            assert bool((big.view(torch.int32) == big.view(torch.int32)[0]).all()) and float(big[0]) == sk.OUT_SENTINEL, (entry, s)
    finally:
        cpu.FAKE = old


@pytest.mark.parametrize("v", (18, 25))
def test_framewise_stage_follows_its_route(v):
    """csk_agcn_stage_framewise_f32 at every offset of x: where its route query answers (V = 25 everywhere, V = 18 at 0 and 8 bytes) the
    launch gives the exact tier's fp64 bits; where it answers 0 the stage returns -1 with its message and y keeps every word"""
    from tests import agcn_framewise_fixture as fw
    lib = native.lib()
    c = next(c for c in fw.CASES if c.V == v and c.seg_pad % 2 == 0)
    inter, ops = fw.inter_of(c), fw.operands(c, "exact")
    fw.admissible(c, ops)
    want = torch.from_numpy(fw.definition(ops, inter, c.conv_res, adj=ops["adj_exact"]).astype(np.float32))
    w_img, b_img = fw.stage_image(ops["W"], ops["bias"])
    e_img, eb_img = af.pair_major(ops["we"], ops["be"], inter)
    dev = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV) for a in (w_img, b_img, e_img, eb_img, ops["a_sum"])]
    n, _, T, V = ops["x"].shape
    chan, res = T * V, 2 if c.conv_res else 1
    for s in (0, 1, 2, 3):
        x = sk.Skewed(ops["x"].shape, s, DEV, src=torch.from_numpy(ops["x"]))
        y = sk.Skewed(tuple(want.shape), (s + 2) % 4, DEV)
        route = lib.csk_agcn_stage_framewise_f32_route(native.ptr(x.t), n, c.c_in, c.c_out, inter, T, V, c.c_in * chan, chan, res)
        assert route == (fw.route_of(c) if v == 25 or s % 2 == 0 else 0), (s, route)
        rc = lib.csk_agcn_stage_framewise_f32(native.ptr(x.t), native.ptr(y.t), *(native.ptr(t) for t in dev), n, c.c_in, c.c_out, inter, T, V,
                                              c.c_in * chan, chan, c.c_out * chan, chan, res, _stream())
        torch.cuda.synchronize()
        assert x.bands_intact() and y.bands_intact(), s
        if route:
            native.check(rc, "csk_agcn_stage_framewise_f32")
            assert sk.same_bits(y.host(), want), s
        else:
            assert rc == -1 and sk.ENTRIES["csk_agcn_stage_framewise_f32"].message in lib.csk_last_error().decode(), (s, rc)
            assert bool((y.host() == sk.OUT_SENTINEL).all()), s


# ---- through the package ------------------------------------------------------------------------------------------------------------
def _graph(v):
    return (pkg.ntu_graph() if v == 25 else pkg.kinetics_graph()).A


def _view(t, s):
    """a contiguous copy of `t` on the device at s floats off the 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, device=DEV, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    v = buf[s: s + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * s and v.is_contiguous()
    return v


def _x(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


SHAPES = [(16, 25), (21, 25), (16, 18), (21, 18)]


@pytest.mark.parametrize("t,v", SHAPES)
@pytest.mark.parametrize("ci,co", [(3, 64), (64, 64), (64, 128)])
def test_graph_convolution_on_a_view(ci, co, t, v):
    m = pkg.GraphConvolution(ci, co, _graph(v)).eval()
    randomise_unit_(m, 11 + ci + co)
    m = m.to(DEV)
    x = _x((3, ci, t, v), t + v)
    want = m(_view(x, 0))
    for s in (1, 2, 3):
        assert torch.equal(m(_view(x, s)), want), s


BLOCKS = [("identity", 64, 64, 1, {}), ("conv", 64, 128, 2, {}), ("conv-s1", 64, 128, 1, {}), ("none", 64, 64, 1, dict(residual=False)),
          ("none-s2", 64, 64, 2, dict(residual=False)), ("few", 3, 64, 1, dict(residual=False)), ("few-fused", 3, 64, 1, dict(residual=False)),
          ("valid", 64, 64, 1, dict(temporal_padding=0)), ("valid-direct", 64, 64, 1, dict(temporal_padding=0)),
          ("valid-conv", 64, 128, 1, dict(temporal_padding=0))]


@pytest.mark.parametrize("t,v", SHAPES)
@pytest.mark.parametrize("tag,ci,co,stride,kw", BLOCKS, ids=[b[0] for b in BLOCKS])
def test_block_on_a_view_and_into_a_view(tag, ci, co, stride, kw, t, v):
    m = pkg.SpatioTemporalBlock(ci, co, _graph(v), stride=stride, **kw).eval()
    randomise_unit_(m, 5 + ci + co + stride)
    m.fuse_few_channels = tag == "few-fused"
    if tag == "valid-direct":
        m.wino_valid = False
    if tag == "valid-conv":
        m.wino_valid_res = True
    m = m.to(DEV)
    x = _x((3, ci, t, v), 2 * t + v)
    if tag.startswith("few"):
        assert m._few_channels_fusable(_view(x, 1)) == (tag == "few-fused")           # the fused entry runs, resp. the two launches
    if tag in ("valid", "valid-conv"):                                                 # the Winograd entry takes the shape: no -2 fall-back
        c_res = co if tag == "valid" else ci
        assert not tw.select("valid" if tag == "valid" else "valid_res", co, co, c_res, t, v, 9, 1, 0, 1 if tag == "valid" else 2, 4, n_seg=3).reject
    want = m(_view(x, 0))
    assert bool(torch.isfinite(want).all())
    for sx_, so in ((1, 1), (2, 3), (3, 2), (0, 1), (3, 0)):
        out = sk.Skewed(tuple(want.shape), so, DEV)
        got = m(_view(x, sx_), out=out.t)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.t.data_ptr() and out.bands_intact() and torch.equal(out.t, want), (sx_, so)


@pytest.mark.parametrize("t", (16, 21))
@pytest.mark.parametrize("ci,co", [(64, 64), (64, 128)])
def test_adaptive_graph_conv_leaves_the_fused_path_at_an_odd_offset(ci, co, t):
    """V = 18: the fused entries ask for 8-byte aligned rows (agcn.py mirrors the guard); an odd offset takes the two-launch path, another
    order of summation, the same parity tolerance"""
    m = pkg.AdaptiveGraphConvolution(ci, co, _graph(18)).eval()
    randomise_unit_(m, 3 + ci + co, attn_scale=1.0 / 18)
    m = m.to(DEV)
    x = _x((3, ci, t, 18), t)
    strides = (ci * t * 18, t * 18)
    want = m(_view(x, 0))
    even = _view(x, 2)
    assert m._fused_ok(18, even.data_ptr(), *strides) and torch.equal(m(even), want)          # 8 bytes: the fused path again
    for s in (1, 3):
        v = _view(x, s)
        assert not m._fused_ok(18, v.data_ptr(), *strides)
        got = m(v)
        err = max_err(got.cpu(), want.cpu())
        print(f"agcn V=18 {ci}->{co} T={t} offset {s}: two-launch path against the fused path, max err {err:.3e}")
        assert bool(torch.isfinite(got).all()) and err <= TOL, (s, err)


@pytest.mark.parametrize("t,v", SHAPES)
@pytest.mark.parametrize("ci,co", [(64, 64), (64, 128)])
def test_str_unit_on_a_view(ci, co, t, v):
    m = pkg.GcnUnitAttention(ci, co, _graph(v), num_point=v).eval()
    randomise_unit_(m, 9 + ci + co)
    m = m.to(DEV)
    x = _x((3, ci, t, v), t * v)
    want = m(_view(x, 0))
    assert bool(torch.isfinite(want).all())
    for s in (1, 2, 3):
        assert torch.equal(m(_view(x, s)), want), s


@pytest.mark.parametrize("t,v", SHAPES)
def test_stgcn_clip_forward_on_a_view(t, v):
    net = pkg.StGcn(_graph(v), input_shape=(3, 300, v, 2), num_classes=10).eval()
    randomise_unit_(net, 21 + v)
    net = net.to(DEV)
    x = _x((3, 3, t, v, 2), t + 3 * v)
    with torch.no_grad():
        want = net(_view(x, 0))
        assert bool(torch.isfinite(want).all())
        for s in (1, 2, 3):
            assert torch.equal(net(_view(x, s)), want), s


def test_forward_cycle_with_every_frame_at_its_own_skew():
    A = _graph(25)
    nets = []
    for _ in range(2):
        net = pkg.CoStGcn(A, pool_size=4, pool_padding=1).eval()
        randomise_unit_(net, 33)
        nets.append(net.to(DEV))
    x = _x((3, 3, 120, 25, 2), 77)
    got, want = [], []
    with torch.no_grad():
        for t0 in range(0, 120, 8):
            want += nets[0].forward_cycle([_view(x[:, :, t0 + f], 0) for f in range(8)])
            got += nets[1].forward_cycle([_view(x[:, :, t0 + f], (t0 // 8 + f) % 4) for f in range(8)])
    assert len(want) >= 2 and len(got) == len(want)
    assert all(bool(torch.isfinite(w).all()) and torch.equal(g, w) for g, w in zip(got, want))
