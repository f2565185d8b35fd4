"""fold.pack_conv_weight_wino (operand image of csk_tcn_stage_wino_f32): the transformed weights, pushed through an fp64
emulation of the kernel's grouped F(2, 3) -- input transform, 12 products, output transform -- reproduce the direct 9-tap conv
(stride 1, pad 4), odd and even T; the packed layout pads channels / rows with zeros; the block fold carries the image exactly
for the layers the kernel takes."""
import numpy as np
import pytest
import torch

import _bootstrap

pkg = _bootstrap.load()
from continual_skeletons_amd import fold  # noqa: E402


def _direct(y, w):
    """(C, T, V) fp64 input, (Co, C, 9) fp64 weight -> (Co, T, V): out[t] = sum_r w[r] y[t + r - 4]."""
    c, t, v = y.shape
    yp = np.zeros((c, t + 8, v))
    yp[:, 4:4 + t] = y
    return sum(np.einsum("oc,ctv->otv", w[:, :, r], yp[:, r:r + t]) for r in range(9))


def _wino(y, img, co):
    """The kernel's arithmetic in fp64 from the packed image [12][Cpad][Mpad]: pairs j, d = y[2 j + 3 g - 4 ...]."""
    c, t, v = y.shape
    npair = (t + 1) // 2
    yp = np.zeros((c, 2 * npair + 10, v))
    yp[:, 4:4 + t] = y
    u = img[:, :c, :co]                                       # [4 g + i][c][co]
    m = np.zeros((4, co, npair, v))
    for g in range(3):
        d = [yp[:, 3 * g + f: 3 * g + f + 2 * npair: 2] for f in range(4)]     # frames 2 j + 3 g - 4 + f, (c, npair, v)
        b = (d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3])
        for i in range(4):
            m[i] += np.einsum("co,cjv->ojv", u[4 * g + i], b[i])
    out = np.zeros((co, 2 * npair, v))
    out[:, 0::2] = m[0] + m[1] + m[2]
    out[:, 1::2] = m[1] - m[2] - m[3]
    return out[:, :t]


@pytest.mark.parametrize("c", [8, 64, 256])
@pytest.mark.parametrize("t", [9, 17, 40, 75])
@pytest.mark.parametrize("v", [25, 18])
def test_wino_image_reproduces_the_direct_conv(c, t, v):
    rng = np.random.default_rng(c + 7 * t + v)
    co = 64 if c != 8 else 40
    w = torch.from_numpy(rng.standard_normal((co, c, 9, 1)))
    scale = torch.from_numpy(rng.random(co) + 0.5)
    img = fold.pack_conv_weight_wino(w, scale).double().numpy()
    assert img.shape == (12, (c + 15) // 16 * 16, (co + 63) // 64 * 64)
    # fp64 emulation on the fp64 transform (the packed image is its fp32 rounding: compare the exact transform too)
    wf = w.numpy()[:, :, :, 0] * scale.numpy()[:, None, None]
    g = np.array(fold.WINO_G)
    exact = np.einsum("ir,ocgr->gico", g, wf.reshape(co, c, 3, 3)).reshape(12, c, co)
    assert np.array_equal(img[:, :c, :co], exact.astype(np.float32).astype(np.float64))
    assert not img[:, c:].any() and not img[:, :, co:].any()
    y = rng.random((c, t, v))
    want = _direct(y, wf)
    full = np.zeros_like(img)
    full[:, :c, :co] = exact
    got = _wino(y, full, co)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # and with the fp32-rounded image: fp32-level agreement (the rounding of the transformed weights)
    got32 = _wino(y, img, co)
    assert np.abs(got32 - want).max() <= 1e-5 * np.abs(want).max()


def test_block_fold_carries_the_image_for_stride_one_nine_tap_convs():
    a = pkg.ntu_graph().A
    blk = pkg.SpatioTemporalBlock(64, 64, a, stride=1, residual=True).eval()
    import bench
    bench.randomise_(blk, 2)
    ops = blk._fold()
    sd = blk.state_dict()
    s, _ = fold.bn_affine(sd["tcn.bn.weight"], sd["tcn.bn.bias"], sd["tcn.bn.running_mean"], sd["tcn.bn.running_var"])
    assert torch.equal(ops["w_wino"], fold.pack_conv_weight_wino(sd["tcn.t_conv.weight"], s))
    assert ops["w_wino"].shape == (12, 64, 64) and ops["w_wino"].dtype == torch.float32
    assert pkg.SpatioTemporalBlock(64, 128, a, stride=2).eval()._fold()["w_wino"] is None
    with pytest.raises(ValueError):
        fold.pack_conv_weight_wino(torch.zeros(4, 4, 3, 1), torch.ones(4, dtype=torch.float64))


def test_refold_after_weight_edit_refreshes_the_image():
    """The image lives in the block's fold cache: an in-place weight edit is seen on the next call and the image is rebuilt."""
    a = pkg.ntu_graph().A
    blk = pkg.SpatioTemporalBlock(16, 64, a, stride=1).eval()
    first = blk._packed_ops("cpu")["w_wino"].clone()
    with torch.no_grad():
        blk.tcn.t_conv.weight.mul_(2.0)
    again = blk._packed_ops("cpu")["w_wino"]
    assert not torch.equal(first, again)
    assert torch.allclose(again, 2 * first, rtol=1e-6, atol=0)
