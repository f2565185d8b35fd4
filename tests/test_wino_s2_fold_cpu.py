"""fold.pack_conv_weight_wino_s2 (operand image of csk_tcn_stage_wino_ext_f32, stride 2): the 13-row polyphase image pushed
through an fp64 model of the kernel's arithmetic (tests/wino_s2_model.py) reproduces the direct 9-tap stride-2 conv plus the
1 x 1 stride-2 residual; the same model in float32 gives the rounding error to expect of the kernel; the block fold carries the
images under ``w_wino_ext`` and leaves ``w_wino`` as it was."""
import numpy as np
import pytest
import torch

import _bootstrap
from tests.wino_s2_model import direct_s2, wino_s2

pkg = _bootstrap.load()
from continual_skeletons_amd import fold  # noqa: E402


def _exact_image(wf):
    """The fp64 transform the packed image is the fp32 rounding of, written out tap by tap."""
    co, c, _ = wf.shape
    g = np.array(fold.WINO_G)
    z = np.zeros((co, c))
    groups = [(wf[:, :, 0], wf[:, :, 2], wf[:, :, 4]), (wf[:, :, 6], wf[:, :, 8], z), (wf[:, :, 1], wf[:, :, 3], z),
              (wf[:, :, 5], wf[:, :, 7], z)]
    rows = []
    for n, taps in enumerate(groups):
        for i in range(4 if n == 0 else 3):
            rows.append(sum(g[i][r] * taps[r] for r in range(3)).T)          # (c, co)
    return np.stack(rows)


@pytest.mark.parametrize("c", [3, 64])
@pytest.mark.parametrize("t", [9, 10, 17, 20])
@pytest.mark.parametrize("v", [25, 18])
def test_s2_image_reproduces_the_direct_conv_and_residual(c, t, v):
    rng = np.random.default_rng(c + 7 * t + v)
    co, cr = 64, 5
    w = torch.from_numpy(rng.standard_normal((co, c, 9, 1)))
    scale = torch.from_numpy(rng.random(co) + 0.5)
    img = fold.pack_conv_weight_wino_s2(w, scale).double().numpy()
    assert img.shape == (13, (c + 15) // 16 * 16, 64)
    wf = w.numpy()[:, :, :, 0] * scale.numpy()[:, None, None]
    exact = _exact_image(wf)
    assert np.array_equal(img[:, :c, :co], exact.astype(np.float32).astype(np.float64))
    assert not img[:, c:].any()
    y, x, wres = rng.random((c, t, v)), rng.random((cr, t, v)), rng.standard_normal((co, cr))
    full = np.zeros_like(img)
    full[:, :c, :co] = exact
    for xr, wr in ((None, None), (x, wres)):
        want = direct_s2(y, wf, xr, wr)
        assert want.shape == (co, (t - 1) // 2 + 1, v)
        got = wino_s2(y, full, co, xr, wr)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # the model's direct form is F.conv2d (stride 2, pad 4) + the 1 x 1 stride-2 conv
    ref = torch.nn.functional.conv2d(torch.from_numpy(y)[None], torch.from_numpy(wf)[..., None], stride=(2, 1), padding=(4, 0))
    ref = ref + torch.nn.functional.conv2d(torch.from_numpy(x)[None], torch.from_numpy(wres)[..., None, None], stride=(2, 1))
    assert np.abs(ref[0].numpy() - direct_s2(y, wf, x, wres)).max() <= 1e-12 * float(ref.abs().max())


# the shapes of tests/test_gpu_winograd_s2.py::test_s2_vs_forced_direct_path
@pytest.mark.parametrize("c,co,t,v", [(64, 128, 150, 25), (128, 256, 75, 25), (64, 128, 20, 18)])
def test_float32_model_rounding_error(c, co, t, v):
    """The kernel's arithmetic held in float32 (image, operands, transforms, sums) against the fp64 direct conv, O(1) outputs:
    the error to expect of the kernel.  Bound: the project's 1e-5 for the stride-1 Winograd kernel (same points, same transforms).
    Measured: max |err| 8.8e-07 / 1.1e-06 / 7.1e-07 at max |want| 4.1 / 3.2 / 3.0 for the three shapes."""
    rng = np.random.default_rng(c + t + v)
    cr = c // 2
    w = torch.from_numpy(rng.standard_normal((co, c, 9, 1)) / np.sqrt(9 * c))
    wres = rng.standard_normal((co, cr)) / np.sqrt(cr)
    img = fold.pack_conv_weight_wino_s2(w, torch.ones(co, dtype=torch.float64)).numpy()
    y, x = rng.random((c, t, v)).astype(np.float32), rng.random((cr, t, v)).astype(np.float32)
    want = direct_s2(y.astype(np.float64), w.numpy()[:, :, :, 0], x.astype(np.float64), wres.astype(np.float32).astype(np.float64))
    got = wino_s2(y, img, co, x, wres.astype(np.float32), dtype=np.float32)
    assert got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"float32 model {c}->{co} T={t} V={v}: max |err| {err:.3e}, max |want| {np.abs(want).max():.3f}")
    assert err <= 1e-5 * max(1.0, np.abs(want).max())


def test_block_fold_carries_the_ext_images():
    a = pkg.ntu_graph().A
    import bench
    s2 = pkg.SpatioTemporalBlock(64, 128, a, stride=2).eval()
    bench.randomise_(s2, 2)
    ops, sd = s2._fold(), s2.state_dict()
    s, _ = fold.bn_affine(sd["tcn.bn.weight"], sd["tcn.bn.bias"], sd["tcn.bn.running_mean"], sd["tcn.bn.running_var"])
    assert ops["w_wino"] is None
    assert torch.equal(ops["w_wino_ext"], fold.pack_conv_weight_wino_s2(sd["tcn.t_conv.weight"], s))
    assert ops["w_wino_ext"].shape == (13, 128, 128) and ops["w_wino_ext"].dtype == torch.float32
    nores = pkg.SpatioTemporalBlock(64, 64, a, stride=1, residual=False).eval()._fold()
    assert nores["w_wino_ext"] is not None and torch.equal(nores["w_wino_ext"], nores["w_wino"])
    ident = pkg.SpatioTemporalBlock(64, 64, a, stride=1, residual=True).eval()._fold()
    assert ident["w_wino_ext"] is None and ident["w_wino"] is not None
    assert pkg.SpatioTemporalBlock(64, 128, a, stride=1).eval()._fold()["w_wino_ext"] is None      # stride 1, conv residual
    assert pkg.SpatioTemporalBlock(64, 64, a, stride=2, temporal_kernel_size=3).eval()._fold()["w_wino_ext"] is None
    with pytest.raises(ValueError):
        fold.pack_conv_weight_wino_s2(torch.zeros(4, 4, 3, 1), torch.ones(4, dtype=torch.float64))
