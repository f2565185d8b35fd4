"""The valid (pad 0) form of the Winograd clip temporal conv, csk_tcn_stage_wino_valid_f32, against the padded Winograd entries on
the same operands: the valid result equals the padded result cropped to the frames [4, T - 4) BIT FOR BIT (the valid form is the
padded kernel restricted to those output frames; per accumulator element the same products in the same order), with the centred
identity residual (against csk_tcn_stage_wino_f32) and without residual (against csk_tcn_stage_wino_ext_f32).  The output buffer
sits between guard values that must survive.  The entry does not exist before this form was added: the test fails there."""
import pytest
import torch

import _bootstrap

pytestmark = pytest.mark.gpu
pkg = _bootstrap.load()
blocks = pkg.blocks
DEV = "cuda:0"
N = 2                                  # two sequences: a tile boundary meets a sequence boundary
TS = (9, 10, 12, 13, 40, 41)           # T_out = 1, 2, 4, 5 (odd and even, one tile) and 32, 33 (several tiles per sequence)
GUARD, PAD = 7.25, 4096


def _ops(c, v):
    torch.manual_seed(100 + c + v)
    a = (pkg.ntu_graph() if v == 25 else pkg.kinetics_graph()).A
    m = pkg.SpatioTemporalBlock(c, c, a).eval()
    with torch.no_grad():
        for name, prm in m.tcn.named_parameters():
            prm.copy_(torch.rand_like(prm) - 0.5)
        m.tcn.bn.weight.add_(1.0)
        m.tcn.bn.running_var.copy_(torch.rand(c) + 0.5)
        m.tcn.bn.running_mean.copy_(torch.rand(c) - 0.5)
    return m._packed_ops(DEV)


@pytest.mark.parametrize("res", ["identity", "none"])
@pytest.mark.parametrize("v", [25, 18])
@pytest.mark.parametrize("c", [64, 128, 72, 192])      # wide tile; tall tile; c_out % 64 != 0 (both entries: the direct kernel); wide, c_out % 128 != 0
def test_valid_form_equals_the_cropped_padded_form_bitwise(c, v, res):
    ops = _ops(c, v)
    assert ops["w_wino"] is not None and tuple(ops["w_wino"].shape[:1]) == (12,)
    g = torch.Generator().manual_seed(c * v)
    for t in TS:
        y = (torch.rand((N, c, t, v), generator=g) - 0.5).to(DEV)
        x = (torch.rand((N, c, t, v), generator=g) - 0.5).to(DEV)
        if res == "identity":
            padded = blocks.tcn_stage(y, ops["w"], ops["bias"], c, 9, 1, 4, relu=True, res_mode=1, x_res=x, w_wino=ops["w_wino"])
        else:
            padded = blocks.tcn_stage(y, ops["w"], ops["bias"], c, 9, 1, 4, relu=True, w_wino_ext=ops["w_wino"])
        numel = N * c * (t - 8) * v
        buf = torch.full((numel + 2 * PAD,), GUARD, device=DEV)
        out = buf[PAD: PAD + numel].view(N, c, t - 8, v)
        got = blocks.tcn_stage(y, ops["w"], ops["bias"], c, 9, 1, 0, relu=True, res_mode=1 if res == "identity" else 0,
                               x_res=x if res == "identity" else None, res_off=4 if res == "identity" else 0, out=out,
                               w_wino_valid=ops["w_wino"])
        assert got is out and tuple(padded.shape) == (N, c, t, v)
        assert torch.equal(got, padded[:, :, 4: t - 4]), (t, float((got - padded[:, :, 4: t - 4]).abs().max()))
        assert bool((buf[:PAD] == GUARD).all()) and bool((buf[PAD + numel:] == GUARD).all()), t
        assert float(got.abs().max()) > 0.1                      # not all clipped by the ReLU: the comparison means something


def test_the_block_routes_identity_residual_unpadded_blocks_through_it():
    """SpatioTemporalBlock(temporal_padding=0) with the identity residual: the block's output is the valid entry's on its graph
    conv's output, and switching ``wino_valid`` off gives the direct kernels' (equal within 1e-5, not bit for bit)."""
    torch.manual_seed(5)
    m = pkg.SpatioTemporalBlock(64, 64, pkg.ntu_graph().A, temporal_padding=0).eval()
    with torch.no_grad():
        m.gcn.bn.weight.fill_(1.0)
        m.tcn.bn.running_var.copy_(torch.rand(64) + 0.5)
    m = m.to(DEV)
    x = torch.rand((2, 64, 21, 25), generator=torch.Generator().manual_seed(6)).to(DEV)
    ops = m._packed_ops(DEV)
    got = m(x)
    want = blocks.tcn_stage(m.gcn(x), ops["w"], ops["bias"], 64, 9, 1, 0, relu=True, res_mode=1, x_res=x, res_off=4,
                            w_wino_valid=ops["w_wino"])
    assert tuple(got.shape) == (2, 64, 13, 25) and torch.equal(got, want)
    m.wino_valid = False
    direct = m(x)
    assert not torch.equal(direct, got) and float((direct - got).abs().max()) <= 1e-5 * max(1.0, float(direct.abs().max()))
