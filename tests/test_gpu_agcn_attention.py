"""The A-GCN attention kernels (csrc/agcn.hip) against an fp64 softmax under a derived bound, through the C ABI: csk_agcn_attention_f32
in its clip form (chunks of 64 frames, four channel ranges) and its step form (one wave per pair), and all twelve instantiations of
the fused csk_agcn_embed_attention_f32.  Operands, reference and bound come from tests/agcn_attention_fixture.py: integer embeddings
make every logit sum exact in fp32, the bound covers the division, the exponential, the column sum, the reciprocal and the last add.
E, x, weights and a_sum lie between NaN bands, the adjacency is NaN before the launch."""
import ctypes

import numpy as np
import pytest
import torch

import _bootstrap
from tests import agcn_attention_fixture as fx
from tests.head_fixture import check_bound
from tests.test_gpu_dense_gcn import Guarded, _stream
from tests.dense_gcn_fixture import strided

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
native = pkg.native
f32 = np.float32


def _attention(E_flat, off, a_sum, n, inter, T, V, e_seg, e_chan, spg, e_group):
    lib = native.lib()
    E, a, adj = Guarded(E_flat, offset=off), Guarded(a_sum), Guarded(size=n * 3 * V * V)
    scratch = Guarded(size=n * 3 * 4 * V * V) if T > 1 else None
    native.check(lib.csk_agcn_attention_f32(E.ptr(), a.ptr(), adj.ptr(), scratch.ptr() if scratch else None, n, inter, T, V, e_seg, e_chan,
                                            spg, e_group, _stream()), "csk_agcn_attention_f32")
    torch.cuda.synchronize()
    for g in (E, a, adj) + ((scratch,) if scratch else ()):
        g.assert_bands()
    return adj.numpy().reshape(n, 3, V, V)


@pytest.mark.parametrize("c", fx.ATT_CLIP, ids=lambda c: c.name)
def test_attention_clip_form(c):
    """T = 1 (the step kernel), 2, 63 / 64 / 65 around the 64-frame chunk, 130 (a partial third chunk); inter 3 and 6 (channel ranges
    of unequal and of zero length), 16, 20; V 2 .. 32; the NaN band starts right behind E's last element"""
    E, a_sum = fx.att_operands(c.n, c.inter, c.T, c.V, 0)
    fx.admissible(E, c.inter)
    chan = c.T * c.V + c.chan_pad
    seg = 6 * c.inter * chan
    got = _attention(strided(E, chan, seg), c.off, a_sum, c.n, c.inter, c.T, c.V, seg, chan, c.n, 0)
    want, bnd = fx.reference(E, a_sum, c.inter)
    check_bound(got, want, bnd, n_terms=c.V, kernel="agcn_attention", case=c.name)


@pytest.mark.parametrize("c", fx.ATT_STEP, ids=lambda c: c.name)
def test_attention_step_form(c):
    """groups of several skeletons in channel-major frames, a gap between the groups, pair counts that leave a workgroup short"""
    n = c.groups * c.spg
    E, a_sum = fx.att_operands(n, c.inter, 1, c.V, 1)
    fx.admissible(E, c.inter)
    P = (c.spg * c.V + 3 + 3) // 4 * 4
    group = 6 * c.inter * P + c.group_pad
    flat = np.full((c.groups - 1) * group + 6 * c.inter * P, np.nan, dtype=f32)
    for g in range(c.groups):
        for ch in range(6 * c.inter):
            for s in range(c.spg):
                o = g * group + ch * P + s * c.V
                flat[o: o + c.V] = E[g * c.spg + s, ch, 0]
    got = _attention(flat, 0, a_sum, n, c.inter, 1, c.V, c.V, P, c.spg, group)
    want, bnd = fx.reference(E, a_sum, c.inter)
    check_bound(got, want, bnd, n_terms=c.V, kernel="agcn_attention_step", case=c.name)


def _fused(c, x, w, b, a_sum):
    lib = native.lib()
    xc = c.frames * c.V + c.x_pad
    xs = c.c_in * xc + (2 if c.V == 18 else 1)
    img, bias = fx.pair_major(w, b, c.inter)
    n_adj = c.n * (c.frames if c.per_frame else 1)
    parts = -(-c.frames // fx.FT[c.V])
    xd, wd, bd, a, adj = Guarded(strided(x, xc, xs)), Guarded(img), Guarded(bias), Guarded(a_sum), Guarded(size=n_adj * 3 * c.V * c.V)
    scratch = None if c.per_frame else Guarded(size=c.n * 3 * parts * c.V * c.V)
    native.check(lib.csk_agcn_embed_attention_f32(xd.ptr(), wd.ptr(), bd.ptr(), a.ptr(), adj.ptr(), scratch.ptr() if scratch else None, c.n,
                                                  c.c_in, c.inter, c.frames, c.V, c.per_frame, xs, xc, _stream()), "csk_agcn_embed_attention_f32")
    torch.cuda.synchronize()
    for g in (xd, wd, bd, a, adj) + ((scratch,) if scratch else ()):
        g.assert_bands()
    return adj.numpy().reshape(n_adj, 3, c.V, c.V)


def _two_launches(c, x, w, b, a_sum):
    """csk_conv1x1_f32 into an E tensor, then csk_agcn_attention_f32 (per frame: every frame a segment of a group)"""
    lib = native.lib()
    rows, xc, ec = 6 * c.inter, c.frames * c.V + c.x_pad, c.frames * c.V
    xs, es = c.c_in * xc, rows * ec
    img, bias = fx.conv_image(w, b)
    xd, wd, bd = Guarded(strided(x, xc, xs)), Guarded(img), Guarded(bias)
    E = Guarded(size=c.n * es)
    native.check(lib.csk_conv1x1_f32(xd.ptr(), E.ptr(), wd.ptr(), bd.ptr(), c.n, c.c_in, rows, c.frames, c.V, xs, xc, es, ec, _stream()),
                 "csk_conv1x1_f32")
    torch.cuda.synchronize()
    E.assert_bands()
    if c.per_frame:
        return _attention(E.numpy(), 0, a_sum, c.n * c.frames, c.inter, 1, c.V, c.V, ec, c.frames, es)
    return _attention(E.numpy(), 0, a_sum, c.n, c.inter, c.frames, c.V, es, ec, c.n, 0)


@pytest.mark.parametrize("inter", (16, 32, 64))
@pytest.mark.parametrize("V", (18, 25))
@pytest.mark.parametrize("per_frame", (1, 0))
def test_fused_embed_attention(per_frame, V, inter):
    """one instantiation per test, at 1, 128 / V, 128 / V + 1 and 3 (128 / V) + 2 frames (several partial-logit parts in the clip
    form): the fused entry and the two-launch route each within the bound of the same fp64 reference"""
    for c in fx.EMB_CASES:
        if (c.inter, c.V, c.per_frame) != (inter, V, per_frame):
            continue
        x, w, b, a_sum = fx.emb_operands(c)
        E = fx.embed(x, w, b)
        E = fx.per_frame_view(E) if c.per_frame else E
        fx.admissible(E, c.inter)
        want, bnd = fx.reference(E, a_sum, c.inter)
        check_bound(_fused(c, x, w, b, a_sum), want, bnd, n_terms=c.V, kernel="agcn_embed_attention", case=c.name)
        check_bound(_two_launches(c, x, w, b, a_sum), want, bnd, n_terms=c.V, kernel="conv1x1+agcn_attention", case=c.name)
